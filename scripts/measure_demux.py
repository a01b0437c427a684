#!/usr/bin/env python3
"""fq-demux on device-resident input, in ONE process: the 2 x 150 bp input of scripts/measure_trim.py (2 M pairs, built the same way from
the same seed), with inline barcodes of 8 + 8 letters planted over the first bases of both mates for a sheet of 96 and one of 1024
samples; one unit in a hundred gets one substitution in barcode 1, one in a hundred a random pair of barcodes.  Measured per sheet:
 - X1, the assignment kernel, beside fq-trim's T1 on the same R1 (single-end, default probes) in the same process,
 - the radix sort, X2 with its scans,
 - X3, the gather-write kernel, with the bytes it reads and writes: clipped records (four pieces each) and, with the barcodes kept,
   whole records (one copy each); the latter beside fq-screen's S4 on the same inputs in the same process, with a reference no read
   shares a k-mer with — both echo every record, S4 in input order, X3 in destination order: the ratio is the price of the gather,
 - the whole call with device outputs sized by a sizing call.
Writes profiles/demux/measure.json (--out).

Run it under a time limit of its own:  timeout -k 10 600 python scripts/measure_demux.py
"""
import argparse
import json
import os
import sys

for name in ("SCFQ_DEMUX_TIMING", "SCFQ_SCREEN_TIMING", "SCFQ_TRIM_TIMING"):      # the library brackets its stages with HIP events
    os.environ[name] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "seq-collection_amd", "pyhost"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from measure_insert_size import best, paired      # noqa: E402  (the same inputs)
from measure_merge import random_qualities      # noqa: E402

BARCODE = 8


def spread(v):
    s = sorted(v)
    return {"best": s[0], "median": s[len(s) // 2], "worst": s[-1]}


def make_sheet(np, rng, n):
    """n distinct pairs of barcodes"""
    letters = np.frombuffer(b"ACGT", np.uint8)
    seen, out = set(), []
    while len(out) < n:
        pair = (letters[rng.integers(0, 4, BARCODE)].tobytes().decode(), letters[rng.integers(0, 4, BARCODE)].tobytes().decode())
        if pair not in seen:
            seen.add(pair)
            out.append(("s%d" % len(out),) + pair)
    return out


def planted(np, rng, rec1, rec2, pairs, length, samples):
    """copies of the two inputs with a sample's barcodes over the first bases of every pair"""
    rows1, rows2 = rec1.copy().reshape(pairs, 2 * length + 7), rec2.copy().reshape(pairs, 2 * length + 7)
    letters = np.frombuffer(b"ACGT", np.uint8)
    b1 = np.array([np.frombuffer(s[1].encode(), np.uint8) for s in samples])
    b2 = np.array([np.frombuffer(s[2].encode(), np.uint8) for s in samples])
    pick = rng.integers(0, len(samples), pairs)
    rows1[:, 3:3 + BARCODE], rows2[:, 3:3 + BARCODE] = b1[pick], b2[pick]
    kind = rng.integers(0, 100, pairs)
    sub = np.flatnonzero(kind == 0)
    at = rng.integers(0, BARCODE, sub.size)
    rows1[sub, 3 + at] = letters[(np.searchsorted(letters, rows1[sub, 3 + at]) + rng.integers(1, 4, sub.size)) % 4]
    rnd = np.flatnonzero(kind == 1)
    rows1[rnd, 3:3 + BARCODE] = letters[rng.integers(0, 4, (rnd.size, BARCODE))]
    rows2[rnd, 3:3 + BARCODE] = letters[rng.integers(0, 4, (rnd.size, BARCODE))]
    return rows1.reshape(-1), rows2.reshape(-1)


def demux_runs(scfq, torch, sheet, t1, t2, reps, **kw):
    opts = scfq.demux_opts(**kw)
    args = (sheet, t1.data_ptr(), t1.numel(), t2.data_ptr(), t2.numel(), opts)
    size, _ = scfq.demux_device(*args)
    outs = [torch.empty(max(int(b), 1), dtype=torch.uint8, device="cuda:0") for b in (size.out1_bytes, size.out2_bytes)]
    stages = []

    def call():
        s, rows = scfq.demux_device(*args, *[(o.data_ptr(), o.numel()) for o in outs])
        stages.append(scfq.demux_stages())
        return s

    call()
    stages.clear()
    b, m, s = best(call, reps)
    assert s.units_in == s.assigned + s.undetermined and s.bases_in == s.bases_out + s.bases_clipped
    st = [[x[j] for x in stages[:reps]] for j in range(4)]
    written = int(s.out1_bytes + s.out2_bytes)      # X3 reads what it writes, and a line-index entry and 8 bytes of the table per record
    x3 = min(st[3])
    return {"call_ms": {"best": b, "median": m}, "x1_ms": spread(st[0]), "sort_ms": spread(st[1]), "x2_scans_ms": spread(st[2]), "x3_ms": spread(st[3]),
            "x3_bytes_read": written, "x3_bytes_written": written, "x3_GBps": 2 * written / (x3 * 1e-3) / 1e9 if x3 > 0 else 0.0,
            "stats": {k: int(getattr(s, k)) for k in ("units_in", "assigned", "perfect", "mismatched", "unmatched", "ambiguous", "no_barcode", "bases_clipped",
                                                      "out1_bytes", "out2_bytes")}}


def screen_echo(scfq, torch, t1, t2, reps, np):
    """fq-screen's S4 echoing every pair: a reference of random letters that no read shares a 31-mer with"""
    ref = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(20261021).integers(0, 4, 5400)]
    index = scfq.screen_index_host([("none", b">none\n" + ref.tobytes())], 31)
    size = scfq.screen_device(index, t1.data_ptr(), t1.numel(), t2.data_ptr(), t2.numel())
    outs = [torch.empty(max(int(b), 1), dtype=torch.uint8, device="cuda:0") for b in (size.out1_bytes, size.out2_bytes)]
    s4 = []
    for _ in range(reps + 1):
        s = scfq.screen_device(index, t1.data_ptr(), t1.numel(), t2.data_ptr(), t2.numel(), None, *[(o.data_ptr(), o.numel()) for o in outs])
        s4.append(scfq.screen_stages()[3])
    index.close()
    moved = int(s.out1_bytes + s.out2_bytes)
    assert s.dropped_reads == 0 and moved == t1.numel() + t2.numel()
    return {"s4_ms": spread(s4[1:]), "s4_bytes_read": moved, "s4_bytes_written": moved, "s4_GBps": 2 * moved / (min(s4[1:]) * 1e-3) / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--block", type=int, default=250_000)
    ap.add_argument("--repeat", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "demux", "measure.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import scfq

    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    rng = np.random.default_rng(20261019)
    length, classes = 150, (100, 180, 260, 350)
    r1, r2, _ = paired(np, rng, args.block, length, classes, 0.1)
    r1, r2 = random_qualities(np, rng, r1, args.block, length), random_qualities(np, rng, r2, args.block, length)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "read_length": length, "pairs": args.block * args.repeat, "block_pairs": args.block,
              "repeat": args.repeat, "barcode_letters": [BARCODE, BARCODE], "substituted": "one unit in 100, one letter of barcode 1",
              "random_barcodes": "one unit in 100",
              "timing": "ms; whole calls: host clock around the synchronous call, best and median of reps after one warm-up; X1, sort, X2 + scans, X3, T1, "
                        "S4: HIP events, best / median / worst of the repeats",
              "sheets": {}}
    sheet_rng = np.random.default_rng(20261020)
    for n in (96, 1024):
        samples = make_sheet(np, sheet_rng, n)
        p1, p2 = planted(np, rng, r1, r2, args.block, length, samples)
        t1 = torch.from_numpy(p1).to("cuda:0").repeat(args.repeat)
        t2 = torch.from_numpy(p2).to("cuda:0").repeat(args.repeat)
        torch.cuda.synchronize()
        per = {"n_samples": n, "input_bytes": [t1.numel(), t2.numel()]}
        t1_ms = []
        for _ in range(args.reps + 1):      # the yardstick of X1: fq-trim's T1 on R1, single-end, default probes
            scfq.trim_device(t1.data_ptr(), t1.numel(), None, 0, scfq.trim_opts())
            t1_ms.append(scfq.trim_stages()[1])
        per["trim_t1_single_end_ms"] = spread(t1_ms[1:])
        with scfq.demux_sheet(samples) as sheet:
            per["clipped"] = demux_runs(scfq, torch, sheet, t1, t2, args.reps)
            per["barcodes_kept"] = demux_runs(scfq, torch, sheet, t1, t2, args.reps, keep_barcode=True)
        per["x1_over_trim_t1"] = per["clipped"]["x1_ms"]["best"] / min(t1_ms[1:]) if min(t1_ms[1:]) > 0 else 0.0
        per["screen_s4_echo"] = screen_echo(scfq, torch, t1, t2, args.reps, np)
        per["x3_kept_over_screen_s4"] = per["barcodes_kept"]["x3_ms"]["best"] / per["screen_s4_echo"]["s4_ms"]["best"]
        result["sheets"]["n%d" % n] = per
        print(n, json.dumps(per), flush=True)
        del t1, t2
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)
    scfq.lib().scfq_shutdown()


if __name__ == "__main__":
    main()

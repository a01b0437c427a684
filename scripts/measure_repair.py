#!/usr/bin/env python3
"""fq-repair on device-resident input, in ONE process: the 2 M pairs of 2 x 150 bp of scripts/measure_rmdup.py (built the same way from the
same seed: every record under a name of its own, "@<8 digits>/1" and "/2"), with a sample's barcode of 8 letters over the first bases of
R1 for fq-demux.  Cases:
 - in_step:       R2 as it is: the positional check answers (path 0)
 - nearly:        R1 without every 100th record, R2 without another every 100th: the realistic case, nearly in order
 - permuted:      R2's records in a random permutation
Measured per case: the whole call of scfq_repair_buffers with four device outputs sized by a sizing call, and its stages by HIP events.
In the same process on the same R1: fq-rmdup's call (single-end, the defaults) and fq-demux's X3 with the barcodes kept (single-end, a
sheet of 96 samples), and the whole call and every stage as multiples of those two.  Writes profiles/repair/measure.json (--out).

Run it under a time limit of its own:  timeout -k 10 900 python scripts/measure_repair.py
"""
import argparse
import json
import os
import sys
import time

for name in ("SCFQ_REPAIR_TIMING", "SCFQ_RMDUP_TIMING", "SCFQ_DEMUX_TIMING"):      # the library brackets its stages with HIP events
    os.environ[name] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "seq-collection_amd", "pyhost"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from measure_demux import BARCODE, make_sheet      # noqa: E402
from measure_insert_size import best      # noqa: E402
from measure_merge import spread      # noqa: E402
from measure_rmdup import EVERY, LENGTH, blocks      # noqa: E402  (the same inputs)

WIDTH = 2 * LENGTH + 7 + 9
STAGES = ("index_ms", "p1_names_ms", "positional_check_ms", "p2_hash_ms", "sort_ms", "rounds_ms", "mates_ms", "lengths_scans_ms", "w1_w2_write_ms")
DROP = 100


def repair_run(scfq, torch, t1, t2, reps):
    """the whole call with outputs that fit, and its stages"""
    args = (t1.data_ptr(), t1.numel(), t2.data_ptr(), t2.numel(), None)
    size = scfq.repair_resident(*args)
    outs = [torch.empty(max(int(getattr(size, n + "_bytes")), 1), dtype=torch.uint8, device="cuda:0") for n in scfq.REPAIR_OUTPUTS]
    stages = []

    def call():
        s = scfq.repair_resident(*args, [(o.data_ptr(), o.numel()) for o in outs])
        stages.append(scfq.repair_stages())
        return s

    call()                                  # warm-up: pool growth, first launches
    stages.clear()
    b, m, s = best(call, reps)
    again = call()
    assert all(getattr(s, k) == getattr(again, k) for k in scfq.REPAIR_STATS_FIELDS) and s.pairs + s.singles1 == s.reads1
    st = {name: {k: v for k, v in spread([x[j] for x in stages[:reps]]).items() if k != "all"} for j, name in enumerate(STAGES)}
    written = sum(int(getattr(s, n + "_bytes")) for n in scfq.REPAIR_OUTPUTS)
    w = st["w1_w2_write_ms"]["best"]
    return dict(st, call_ms={"best": b, "median": m}, bytes_written=written, write_GBps=2 * written / (w * 1e-3) / 1e9 if w > 0 else 0.0,
                stats={k: int(getattr(s, k)) for k in scfq.REPAIR_STATS_FIELDS[2:]}, row=scfq.format_repair_stats_tsv(s))


def rmdup_run(scfq, torch, t1, reps):
    size, _ = scfq.rmdup_resident(t1.data_ptr(), t1.numel(), None, 0, None)
    out = torch.empty(max(int(size.out1_bytes), 1), dtype=torch.uint8, device="cuda:0")
    stages = []

    def call():
        s, _ = scfq.rmdup_resident(t1.data_ptr(), t1.numel(), None, 0, None, (out.data_ptr(), out.numel()))
        stages.append(scfq.rmdup_stages())
        return s

    call()
    stages.clear()
    b, m, s = best(call, reps)
    names = ("index_ms", "u1_hash_ms", "sort_ms", "u2_u3_rounds_ms", "class_sizes_ms", "u4_scans_ms", "u5_write_ms")
    return dict({n: min(x[j] for x in stages[:reps]) for j, n in enumerate(names)}, call_ms={"best": b, "median": m}, units_in=int(s.units_in), units_out=int(s.units_out),
                bytes_written=int(s.out1_bytes))


def demux_run(scfq, torch, sheet, t1, reps):
    opts = scfq.demux_opts(keep_barcode=True)
    args = (sheet, t1.data_ptr(), t1.numel(), None, 0, opts)
    size, _ = scfq.demux_device(*args)
    out = torch.empty(max(int(size.out1_bytes), 1), dtype=torch.uint8, device="cuda:0")
    stages = []

    def call():
        s, rows = scfq.demux_device(*args, (out.data_ptr(), out.numel()))
        stages.append(scfq.demux_stages())
        return s

    call()
    stages.clear()
    b, m, s = best(call, reps)
    x3 = min(x[3] for x in stages[:reps])
    return {"call_ms": {"best": b, "median": m}, "x3_ms": x3, "bytes_written": int(s.out1_bytes), "x3_GBps": 2 * int(s.out1_bytes) / (x3 * 1e-3) / 1e9 if x3 > 0 else 0.0,
            "units_in": int(s.units_in), "assigned": int(s.assigned)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--block", type=int, default=250_000)
    ap.add_argument("--repeat", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repair", "measure.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import scfq

    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    t0 = time.perf_counter()
    rng = np.random.default_rng(20261019)
    b1, b2 = blocks(np, rng, args.block, args.repeat)
    pairs = args.block * args.repeat
    r1, r2 = np.concatenate(b1).reshape(pairs, WIDTH), np.concatenate(b2).reshape(pairs, WIDTH)
    del b1, b2
    # a sample's barcode over the first bases of R1, one sample per group of EVERY pairs: the planted duplicates stay duplicates
    samples, seen = [], set()
    for s in make_sheet(np, rng, 200):              # (distinct pairs of barcodes: the first ones of 96 of them that differ)
        if s[1] not in seen and len(samples) < 96:
            seen.add(s[1])
            samples.append(s[:2])
    codes = np.array([np.frombuffer(s[1].encode(), np.uint8) for s in samples])
    r1[:, 12:12 + BARCODE] = codes[rng.integers(0, len(samples), (pairs + EVERY - 1) // EVERY)][np.arange(pairs) // EVERY]
    keep1, keep2 = np.arange(pairs) % DROP != 0, np.arange(pairs) % DROP != DROP // 2
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to("cuda:0")
    d1 = dev(r1)
    inputs = {"in_step": (d1, dev(r2)), "nearly": (dev(r1[keep1]), dev(r2[keep2])), "permuted": (d1, dev(r2[rng.permutation(pairs)]))}
    del r1, r2
    torch.cuda.synchronize()
    print("inputs built in %.1f s" % (time.perf_counter() - t0), flush=True)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "pairs": pairs, "read_length": LENGTH, "record_bytes": WIDTH,
              "cases": {"in_step": "R2 as it is", "nearly": "R1 without every %dth record, R2 without another every %dth" % (DROP, DROP),
                        "permuted": "R2's records in a random permutation"},
              "timing": "ms; whole calls: host clock around the synchronous call, best and median of reps after one warm-up; the stages: HIP events (the "
                        "line indexes: host clock), best, median and worst of the repeats.  Nothing is pinned: a first measurement",
              "not_measured": ["hardware counters of any kernel", "names longer than 10 bytes, comments behind the names", "repeated names", "host and file outputs, the command",
                               "inputs of different sizes", "hash_bits other than the default", "the name hash fused into the index pass"],
              "workloads": {}}
    for name, (t1, t2) in inputs.items():
        result["workloads"][name] = repair_run(scfq, torch, t1, t2, args.reps)
        print(name, json.dumps(result["workloads"][name]["call_ms"]), result["workloads"][name]["row"], flush=True)
    t1 = inputs["in_step"][0]
    rm = result["rmdup_on_r1"] = rmdup_run(scfq, torch, t1, args.reps)
    with scfq.demux_sheet(samples) as sheet:
        dx = result["demux_keep_barcode_on_r1"] = demux_run(scfq, torch, sheet, t1, args.reps)
    print(json.dumps({"rmdup": rm["call_ms"], "demux_x3_ms": dx["x3_ms"]}), flush=True)
    yard = {"rmdup_call": rm["call_ms"]["best"], "demux_x3": dx["x3_ms"]}
    result["multiples"] = {name: {what: {k: (w[k]["best"] / v if v > 0 else 0.0) for k in ("call_ms",) + STAGES[1:]} for what, v in yard.items()}
                           for name, w in result["workloads"].items()}
    result["call_over_rmdup_plus_x3"] = {name: w["call_ms"]["best"] / (yard["rmdup_call"] + yard["demux_x3"]) for name, w in result["workloads"].items()}
    print(json.dumps(result["call_over_rmdup_plus_x3"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)
    scfq.lib().scfq_shutdown()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""fq-insert-size on device-resident paired input, in ONE process: 2 x 150 bp and 2 x 250 bp, two files each.  The input is built on
the host without a Python loop: a block of --block pairs whose fragments come from a few insert classes (read-through, overlapping,
too long to overlap) plus unrelated mates and 1 % N, repeated --repeat times (the kernel treats every pair alike, whatever its
neighbours hold).  Measured: the whole call of scfq_insert_size_buffers (no table, histogram wanted) and its stages (line indexes,
P1 the overlap kernel, P2 the pass over the bins), and in the same process on the same R1 bytes scfq_cycles_buffer: its counting
kernel C1 makes one pass over the input and is the yardstick of P1.
Writes profiles/insert_size/measure.json (--out).

Run it under a time limit of its own:  timeout -k 10 600 python scripts/measure_insert_size.py
"""
import argparse
import json
import os
import sys
import time

os.environ["SCFQ_INSERT_TIMING"] = "1"      # the library brackets its stages with HIP events (read before its first call)
os.environ["SCFQ_CYCLES_TIMING"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "seq-collection_amd", "pyhost"))


def best(fn, reps):
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t) * 1e3)
    return min(out), sorted(out)[len(out) // 2], r


def paired(np, rng, pairs, length, classes, unrelated, errors=0.01):
    """(r1, r2, inserts): `pairs` records each of `length` bases; pair i is cut from a fragment of inserts[i] bases (0: unrelated)"""
    pad = length
    width = pad + max(classes) + length
    letters = np.frombuffer(b"ACGT", np.uint8)
    g = rng.integers(0, 4, (pairs, width), dtype=np.uint8)
    ins = rng.choice(np.array(classes), pairs)
    ins = np.where(rng.random(pairs) < unrelated, 0, ins + rng.integers(-10, 11, pairs))
    rows = np.arange(pairs)[:, None]
    cols = np.arange(length)[None, :]
    a = g[rows, pad + cols]                                        # mate 1: the fragment's first bases (and what follows it)
    c = g[rows, (pad + ins - length)[:, None] + cols]              # the reverse complement of mate 2: its last bases
    c[ins == 0] = rng.integers(0, 4, (int((ins == 0).sum()), length), dtype=np.uint8)
    b = (3 - c)[:, ::-1]

    def records(codes):
        text = letters[codes]
        text[rng.random(text.shape) < errors] = ord("N")
        rec = np.empty((pairs, 2 * length + 7), np.uint8)
        rec[:, :3] = np.frombuffer(b"@p\n", np.uint8)
        rec[:, 3:3 + length] = text
        rec[:, 3 + length:6 + length] = np.frombuffer(b"\n+\n", np.uint8)
        rec[:, 6 + length:6 + 2 * length] = ord("I")
        rec[:, 6 + 2 * length] = 10
        return rec.reshape(-1)

    return records(a), records(b), ins


def measure(scfq, torch, np, rng, length, classes, block, repeat, reps):
    r1, r2, ins = paired(np, rng, block, length, classes, 0.1)
    t1 = torch.from_numpy(r1).to("cuda:0").repeat(repeat)
    t2 = torch.from_numpy(r2).to("cuda:0").repeat(repeat)
    torch.cuda.synchronize()
    n1, n2, pairs = t1.numel(), t2.numel(), block * repeat
    stages = []

    def call():
        s, hist = scfq.insert_size_device(t1.data_ptr(), n1, t2.data_ptr(), n2)
        stages.append(scfq.insert_size_stages())
        return s, hist

    call()                                  # warm-up: pool growth, first launches
    stages.clear()
    b, m, (s, hist) = best(call, reps)
    assert s.pairs == pairs and s.pairs == s.overlapped + s.not_overlapped + s.too_long
    st = [[x[j] for x in stages] for j in range(4)]
    med = lambda v: sorted(v)[len(v) // 2]
    cst = []

    def cycles():
        scfq.cycles_device(t1.data_ptr(), n1, 1000)
        cst.append(scfq.cycles_stages())

    cycles()
    cst.clear()
    cb, cm, _ = best(cycles, reps)
    c1 = [x[2] for x in cst]
    p1 = min(st[1])
    return {"read_length": length, "pairs": pairs, "block_pairs": block, "repeat": repeat, "input_bytes": [n1, n2],
            "insert_classes": list(classes), "class_jitter": 10, "unrelated_share": 0.1, "n_share": 0.01,
            "call_ms": {"best": b, "median": m}, "index_ms": {"best": min(st[0]), "median": med(st[0])},
            "p1_ms": {"best": p1, "median": med(st[1])}, "p2_ms": {"best": min(st[2]), "median": med(st[2])},
            "pairs_per_s": pairs / (p1 * 1e-3) if p1 > 0 else 0.0, "p1_input_GBps": (n1 + n2) / (p1 * 1e-3) / 1e9 if p1 > 0 else 0.0,
            "cycles_r1": {"call_ms": {"best": cb, "median": cm}, "c1_ms": {"best": min(c1), "median": med(c1)}},
            "p1_over_c1_same_r1": p1 / min(c1) if min(c1) > 0 else 0.0,
            "overlapped": s.overlapped, "not_overlapped": s.not_overlapped, "read_through": s.read_through, "mismatches": s.mismatches,
            "overlap_bases": s.overlap_bases, "median_insert": s.median_insert, "mode_insert": s.mode_insert,
            "row": scfq.format_insert_size_tsv(s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--block", type=int, default=250_000)
    ap.add_argument("--repeat", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "insert_size", "measure.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import scfq

    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    rng = np.random.default_rng(20261019)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
              "timing": "ms; whole calls: host clock around the synchronous call, best and median of reps after one warm-up; index: host "
                        "clock around the two synchronous index calls inside the call; P1 / P2 and the fq-cycles kernel C1: HIP events",
              "workloads": {}}
    for name, length, classes in (("2x150", 150, (100, 180, 260, 350)), ("2x250", 250, (150, 300, 440, 600))):
        r = measure(scfq, torch, np, rng, length, classes, args.block, args.repeat, args.reps)
        result["workloads"][name] = r
        print(name, json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)
    scfq.lib().scfq_shutdown()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""fq-complexity on device-resident input, in ONE process: R1 of the 2 x 150 bp workload of scripts/measure_trim.py (2 M reads, built the
same way from the same seed), once as it is and once with a 20-base poly-A tail on every tenth read.  Measured: the whole call of
scfq_cplx_buffers with a device output sized by a sizing call and its stages (D1 the interval kernel, D2 with its scans, D3 the write
kernel), and in the same process on the same buffer fq-trim single-end with its default probes: T1 beside D1, T3 beside D3.
Writes profiles/complexity/measure.json (--out).

Run it under a time limit of its own:  timeout -k 10 600 python scripts/measure_complexity.py
"""
import argparse
import json
import os
import sys

for name in ("SCFQ_CPLX_TIMING", "SCFQ_TRIM_TIMING"):      # the library brackets its stages with HIP events
    os.environ[name] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "seq-collection_amd", "pyhost"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from measure_insert_size import best, paired      # noqa: E402  (the same inputs)
from measure_merge import random_qualities, spread      # noqa: E402

LENGTH, CLASSES, TAIL = 150, (100, 180, 260, 350), 20


def cplx_run(scfq, torch, t1, reps, **kw):
    """the whole call with an output that fits, and its stages, every repeat kept"""
    opts = scfq.cplx_opts(**kw)
    size, _ = scfq.cplx_resident(t1.data_ptr(), t1.numel(), opts=opts)
    out = torch.empty(max(int(size.out1_bytes), 1), dtype=torch.uint8, device="cuda:0")
    stages = []

    def call():
        s, _ = scfq.cplx_resident(t1.data_ptr(), t1.numel(), opts=opts, out1=(out.data_ptr(), out.numel()))
        stages.append(scfq.cplx_stages())
        return s

    call()                                  # warm-up: pool growth, first launches
    stages.clear()
    b, m, s = best(call, reps)
    assert bytes(s) == bytes(call()) and s.reads_in == s.reads_out + s.dropped_reads
    st = [[x[j] for x in stages[:reps]] for j in range(4)]
    d1, d3 = min(st[1]), min(st[3])
    return {"call_ms": {"best": b, "median": m}, "d1_ms": spread(st[1]), "d2_scans_ms": spread(st[2]), "d3_ms": spread(st[3]),
            "d1_ns_per_read": d1 * 1e6 / s.reads_in if s.reads_in else 0.0, "d3_bytes_written": int(s.out1_bytes),
            "d3_written_GBps": s.out1_bytes / (d3 * 1e-3) / 1e9 if d3 > 0 else 0.0,
            "stats": {k: int(getattr(s, k)) for k in scfq.CPLX_STATS_FIELDS[2:]}, "row": scfq.format_cplx_stats_tsv(s)}


def trim_run(scfq, torch, t1, reps):
    size = scfq.trim_device(t1.data_ptr(), t1.numel())
    out = torch.empty(max(int(size.out1_bytes), 1), dtype=torch.uint8, device="cuda:0")
    stages = []

    def call():
        s = scfq.trim_device(t1.data_ptr(), t1.numel(), out1=(out.data_ptr(), out.numel()))
        stages.append(scfq.trim_stages())
        return s

    call()
    stages.clear()
    b, m, s = best(call, reps)
    st = [[x[j] for x in stages[:reps]] for j in range(4)]
    t3 = min(st[3])
    return {"call_ms": {"best": b, "median": m}, "t1_ms": spread(st[1]), "t2_scans_ms": spread(st[2]), "t3_ms": spread(st[3]),
            "t3_bytes_written": int(s.out1_bytes), "t3_written_GBps": s.out1_bytes / (t3 * 1e-3) / 1e9 if t3 > 0 else 0.0}


def ratios(c, t):
    t1, t3, call = t["t1_ms"]["best"], t["t3_ms"]["best"], t["call_ms"]["best"]
    return {"d1_over_t1": c["d1_ms"]["best"] / t1 if t1 > 0 else None, "d3_over_t3": c["d3_ms"]["best"] / t3 if t3 > 0 else None,
            "call_over_trim_call": c["call_ms"]["best"] / call if call > 0 else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--block", type=int, default=250_000)
    ap.add_argument("--repeat", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "complexity", "measure.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import scfq

    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    rng = np.random.default_rng(20261019)
    r1, _, _ = paired(np, rng, args.block, LENGTH, CLASSES, 0.1)
    r1 = random_qualities(np, rng, r1, args.block, LENGTH)
    tailed = r1.copy()
    tailed.reshape(args.block, 2 * LENGTH + 7)[::10, 3 + LENGTH - TAIL:3 + LENGTH] = ord("A")
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "reads": args.block * args.repeat, "read_length": LENGTH,
              "block_reads": args.block, "repeat": args.repeat,
              "timing": "ms; whole calls: host clock around the synchronous call, best and median of reps after one warm-up; D1, D2 + scans, D3, T1, "
                        "T2 + scans, T3: HIP events, every repeat kept",
              "not_measured": ["hardware counters (LDS bank conflicts, VALU utilisation) of D1", "paired and interleaved input", "reads longer than 150 bases",
                               "the file form and the command", "a DPP row shift in place of the shuffle of D1's inner loop",
                               "skipping a round whose near words are all zero"],
              "workloads": {}}
    for name, block in (("as_they_are", r1), ("poly_a_tail_every_tenth", tailed)):
        t1 = torch.from_numpy(block).to("cuda:0").repeat(args.repeat)
        torch.cuda.synchronize()
        w = {"input_bytes": t1.numel()}
        w["defaults"] = cplx_run(scfq, torch, t1, args.reps)
        w["mask_none"] = cplx_run(scfq, torch, t1, args.reps, mask="none")
        w["window_32"] = cplx_run(scfq, torch, t1, args.reps, window=32)
        w["drop_above_10_pct"] = cplx_run(scfq, torch, t1, args.reps, max_masked_pct=10)
        w["trim_single_end"] = trim_run(scfq, torch, t1, args.reps)
        w.update(ratios(w["defaults"], w["trim_single_end"]))
        result["workloads"][name] = w
        print(name, json.dumps(w), flush=True)
        del t1
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)
    scfq.lib().scfq_shutdown()


if __name__ == "__main__":
    main()

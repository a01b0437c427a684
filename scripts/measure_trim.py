#!/usr/bin/env python3
"""fq-trim on device-resident input, in ONE process: the inputs of scripts/measure_merge.py (2 x 150 bp and 2 x 250 bp, 2 M pairs each,
built the same way from the same seed, random quality bytes '!' .. 'I').  Measured: the whole call of scfq_trim_buffers with device
outputs sized by a sizing call and its stages (P1 the overlap kernel, T1 the decision kernel, T2 with its scans, T3 the write kernel)
 - for R1 alone as single-end reads with the default probes,
 - for the pair with the overlap step on,
 - and for both with poly-G and the quality window on as well (not the default; what the two further steps of T1 cost),
the bytes T3 reads and writes and the rate that gives, and in the same process on the same buffers two yardsticks whose code fq-trim
does not touch: scfq_adapters_buffer with the same five probes on R1 (its matching kernel A1 against T1 single-end) and the whole call of
scfq_merge_buffers on the pair (against the paired whole call).
Writes profiles/trim/measure.json (--out).

Run it under a time limit of its own:  timeout -k 10 600 python scripts/measure_trim.py
"""
import argparse
import json
import os
import sys

for name in ("SCFQ_TRIM_TIMING", "SCFQ_MERGE_TIMING", "SCFQ_ADAPTERS_TIMING"):      # the library brackets its stages with HIP events
    os.environ[name] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "seq-collection_amd", "pyhost"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from measure_insert_size import best, paired      # noqa: E402  (the same inputs)
from measure_merge import random_qualities, spread      # noqa: E402

PROBES = ["AGATCGGAAGAG", "TGGAATTCTCGG", "GATCGTCGGACT", "CTGTCTCTTATA", "CGCCTTGGCCGT"]      # the default set of fq-trim


def trim_run(scfq, torch, t1, t2, reps, **kw):
    """the whole call with outputs that fit, and its stages, every repeat kept"""
    opts = scfq.trim_opts(**kw)
    p2, n2 = (t2.data_ptr(), t2.numel()) if t2 is not None else (None, 0)
    size = scfq.trim_device(t1.data_ptr(), t1.numel(), p2, n2, opts)
    outs = [torch.empty(max(int(b), 1), dtype=torch.uint8, device="cuda:0") for b in (size.out1_bytes, size.out2_bytes)]
    args = [(outs[0].data_ptr(), outs[0].numel()), (outs[1].data_ptr(), outs[1].numel()) if t2 is not None else None]
    stages = []

    def call():
        s = scfq.trim_device(t1.data_ptr(), t1.numel(), p2, n2, opts, *args)
        stages.append(scfq.trim_stages())
        return s

    call()                                  # warm-up: pool growth, first launches
    stages.clear()
    b, m, s = best(call, reps)
    assert bytes(s) == bytes(call()) and s.reads_in == s.reads_out + s.dropped_reads
    st = [[x[j] for x in stages[:reps]] for j in range(4)]
    # T3 reads every kept record's header and separator whole and e bases and at most e quality bytes of it, and writes the outputs
    written = s.out1_bytes + s.out2_bytes
    read = written - 4 * s.reads_out          # (the four '\n' of a record are stored, not copied; no read is too long here)
    t3 = min(st[3])
    return {"call_ms": {"best": b, "median": m}, "p1_ms": spread(st[0]), "t1_ms": spread(st[1]), "t2_scans_ms": spread(st[2]), "t3_ms": spread(st[3]),
            "t3_bytes_read": read, "t3_bytes_written": written, "t3_GBps": (read + written) / (t3 * 1e-3) / 1e9 if t3 > 0 else 0.0,
            "t1_ns_per_read": min(st[1]) * 1e6 / s.reads_in if s.reads_in else 0.0,
            "stats": {k: int(getattr(s, k)) for k in ("reads_in", "reads_out", "dropped_reads", "short_reads", "overlapped_pairs", "bases_in", "bases_out",
                                                      "cut_overlap", "cut_adapter", "cut_polyg", "cut_quality", "bases_overlap", "bases_adapter",
                                                      "bases_polyg", "bases_quality", "out1_bytes", "out2_bytes")},
            "row": scfq.format_trim_stats_tsv(s)}


def measure(scfq, torch, np, rng, length, classes, block, repeat, reps):
    r1, r2, _ = paired(np, rng, block, length, classes, 0.1)
    r1, r2 = random_qualities(np, rng, r1, block, length), random_qualities(np, rng, r2, block, length)
    t1 = torch.from_numpy(r1).to("cuda:0").repeat(repeat)
    t2 = torch.from_numpy(r2).to("cuda:0").repeat(repeat)
    torch.cuda.synchronize()
    n1, n2, pairs = t1.numel(), t2.numel(), block * repeat
    out = {"read_length": length, "pairs": pairs, "block_pairs": block, "repeat": repeat, "input_bytes": [n1, n2], "insert_classes": list(classes),
           "class_jitter": 10, "unrelated_share": 0.1, "n_share": 0.01, "qualities": "uniform in '!' .. 'I'"}
    out["single_end"] = trim_run(scfq, torch, t1, None, reps)
    out["paired"] = trim_run(scfq, torch, t1, t2, reps)
    more = dict(poly_g=10, window=4, window_quality=15)
    out["single_end_all_steps"] = dict(trim_run(scfq, torch, t1, None, reps, **more), parameters=more)
    out["paired_all_steps"] = dict(trim_run(scfq, torch, t1, t2, reps, **more), parameters=more)
    # the yardsticks: fq-adapters with the same probes on R1, fq-merge on the pair
    ast = []

    def adapters():
        r = scfq.adapters_device(t1.data_ptr(), n1, PROBES, 0)
        ast.append(scfq.adapters_stages())
        return r

    adapters()
    ast.clear()
    ab, am, _ = best(adapters, reps)
    out["adapters_same_probes"] = {"call_ms": {"best": ab, "median": am}, "a1_ms": spread([x[1] for x in ast])}
    size = scfq.merge_device(t1.data_ptr(), n1, t2.data_ptr(), n2)
    outs = [torch.empty(max(int(b), 1), dtype=torch.uint8, device="cuda:0") for b in (size.merged_bytes, size.unmerged1_bytes, size.unmerged2_bytes)]
    mst = []

    def merge():
        r = scfq.merge_device(t1.data_ptr(), n1, t2.data_ptr(), n2, None, 33, *[(o.data_ptr(), o.numel()) for o in outs])
        mst.append(scfq.merge_stages())
        return r

    merge()
    mst.clear()
    mb, mm, _ = best(merge, reps)
    out["merge"] = {"call_ms": {"best": mb, "median": mm}, "p1_ms": spread([x[1] for x in mst]), "m2_ms": spread([x[3] for x in mst])}
    a1 = out["adapters_same_probes"]["a1_ms"]["best"]
    out["t1_single_end_over_a1"] = out["single_end"]["t1_ms"]["best"] / a1 if a1 > 0 else 0.0
    out["paired_call_over_merge_call"] = out["paired"]["call_ms"]["best"] / mb if mb > 0 else 0.0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--block", type=int, default=250_000)
    ap.add_argument("--repeat", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trim", "measure.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import scfq

    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    rng = np.random.default_rng(20261019)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
              "timing": "ms; whole calls: host clock around the synchronous call, best and median of reps after one warm-up; P1, T1, T2 + scans, T3, "
                        "A1, M2: HIP events, every repeat kept",
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

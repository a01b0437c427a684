#!/usr/bin/env python3
"""fq-merge on device-resident paired input, in ONE process: the inputs of scripts/measure_insert_size.py (2 x 150 bp and 2 x 250 bp,
2 M pairs each, built the same way from the same seed) with random quality bytes '!' .. 'I' patched in.  Measured: the whole call of
scfq_merge_buffers with three device outputs sized by a sizing call, its stages (line indexes, P1 the overlap kernel, M1 with the
three scans, M2 the write kernel), the bytes M2 reads and writes and the rate that gives, and in the same process on the same buffers
the whole call and P1 of scfq_insert_size_buffers: the yardstick, every repeat kept so that P1's run-to-run spread can be read.
--ab-dir: a folder of parent_*.json and branch_*.json that scripts/measure_insert_size.py wrote in the same session on the same
device, run in turn with the parent commit's library and with this one; their P1 times are copied in: the parent's own run-to-run
spread is the margin this build's P1 has to stay inside.
Writes profiles/merge/measure.json (--out).

Run it under a time limit of its own:  timeout -k 10 600 python scripts/measure_merge.py
"""
import argparse
import json
import os
import sys

os.environ["SCFQ_MERGE_TIMING"] = "1"       # the library brackets its stages with HIP events (read before its first call)
os.environ["SCFQ_INSERT_TIMING"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "seq-collection_amd", "pyhost"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from measure_insert_size import best, paired      # noqa: E402  (the same inputs)


def random_qualities(np, rng, rec, pairs, length):
    """the quality line of every record of the block drawn from '!' .. 'I'"""
    rows = rec.reshape(pairs, 2 * length + 7)
    rows[:, 6 + length:6 + 2 * length] = rng.integers(ord("!"), ord("I") + 1, (pairs, length), dtype=np.uint8)
    return rec


def spread(v):
    s = sorted(v)
    return {"best": s[0], "median": s[len(s) // 2], "worst": s[-1], "all": list(v)}


def measure(scfq, torch, np, rng, length, classes, block, repeat, reps):
    r1, r2, _ = paired(np, rng, block, length, classes, 0.1)
    r1, r2 = random_qualities(np, rng, r1, block, length), random_qualities(np, rng, r2, block, length)
    t1 = torch.from_numpy(r1).to("cuda:0").repeat(repeat)
    t2 = torch.from_numpy(r2).to("cuda:0").repeat(repeat)
    torch.cuda.synchronize()
    n1, n2, pairs = t1.numel(), t2.numel(), block * repeat
    size = scfq.merge_device(t1.data_ptr(), n1, t2.data_ptr(), n2)
    outs = [torch.empty(max(int(b), 1), dtype=torch.uint8, device="cuda:0") for b in (size.merged_bytes, size.unmerged1_bytes, size.unmerged2_bytes)]
    stages = []

    def call():
        s = scfq.merge_device(t1.data_ptr(), n1, t2.data_ptr(), n2, None, 33, *[(o.data_ptr(), o.numel()) for o in outs])
        stages.append(scfq.merge_stages())
        return s

    call()                                  # warm-up: pool growth, first launches
    stages.clear()
    b, m, s = best(call, reps)
    assert s.pairs == pairs == s.merged + s.not_overlapped + s.too_long and bytes(s) == bytes(call())
    st = [[x[j] for x in stages[:reps]] for j in range(4)]
    sizing = []

    def size_only():
        scfq.merge_device(t1.data_ptr(), n1, t2.data_ptr(), n2)
        sizing.append(scfq.merge_stages())

    size_only()
    sizing.clear()
    sb, sm, _ = best(size_only, reps)
    ist = []

    def insert():
        r = scfq.insert_size_device(t1.data_ptr(), n1, t2.data_ptr(), n2)
        ist.append(scfq.insert_size_stages())
        return r

    insert()
    ist.clear()
    ib, im, (isum, _) = best(insert, reps)
    assert (isum.overlapped, isum.overlap_bases, isum.mismatches) == (s.merged, s.overlap_bases, s.mismatches)
    # M2 reads a base and a quality byte for every position a mate covers, the merged pairs' headers, and every unmerged record;
    # it writes the three outputs
    header_bytes = s.merged_bytes - 2 * s.merged_bases - 5 * s.merged
    read = header_bytes + 2 * (s.merged_bases + s.overlap_bases) + s.unmerged1_bytes + s.unmerged2_bytes
    written = s.merged_bytes + s.unmerged1_bytes + s.unmerged2_bytes
    m2 = min(st[3])
    return {"read_length": length, "pairs": pairs, "block_pairs": block, "repeat": repeat, "input_bytes": [n1, n2],
            "insert_classes": list(classes), "class_jitter": 10, "unrelated_share": 0.1, "n_share": 0.01, "qualities": "uniform in '!' .. 'I'",
            "call_ms": {"best": b, "median": m}, "sizing_call_ms": {"best": sb, "median": sm},
            "index_ms": spread(st[0]), "p1_ms": spread(st[1]), "m1_scans_ms": spread(st[2]), "m2_ms": spread(st[3]),
            "m2_sizing_ms": spread([x[3] for x in sizing]),
            "m2_bytes_read": read, "m2_bytes_written": written, "m2_GBps": (read + written) / (m2 * 1e-3) / 1e9 if m2 > 0 else 0.0,
            "insert_size": {"call_ms": {"best": ib, "median": im}, "p1_ms": spread([x[1] for x in ist])},
            "m1_m2_over_p1": (min(st[2]) + m2) / min(st[1]) if min(st[1]) > 0 else 0.0,
            "merged": s.merged, "not_overlapped": s.not_overlapped, "merged_bases": s.merged_bases, "overlap_bases": s.overlap_bases,
            "mismatches": s.mismatches, "took_mate1": s.took_mate1, "took_mate2": s.took_mate2, "neither_valid": s.neither_valid,
            "merged_bytes": s.merged_bytes, "unmerged1_bytes": s.unmerged1_bytes, "unmerged2_bytes": s.unmerged2_bytes,
            "row": scfq.format_merge_stats_tsv(s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--block", type=int, default=250_000)
    ap.add_argument("--repeat", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ab-dir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge", "measure.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import scfq

    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    rng = np.random.default_rng(20261019)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
              "timing": "ms; whole calls: host clock around the synchronous call, best and median of reps after one warm-up; index: host "
                        "clock around the two synchronous index calls inside the call; P1, M1 + scans, M2: HIP events, every repeat kept",
              "workloads": {}}
    for name, length, classes in (("2x150", 150, (100, 180, 260, 350)), ("2x250", 250, (150, 300, 440, 600))):
        r = measure(scfq, torch, np, rng, length, classes, args.block, args.repeat, args.reps)
        result["workloads"][name] = r
        print(name, json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    if args.ab_dir:
        import glob
        ab = {}
        for side in ("parent", "branch"):
            runs = [json.load(open(p)) for p in sorted(glob.glob(os.path.join(args.ab_dir, side + "_*.json")))]
            ab[side] = {w: {"p1_ms_best_of_each_run": [r["workloads"][w]["p1_ms"]["best"] for r in runs],
                            "p1_ms_median_of_each_run": [r["workloads"][w]["p1_ms"]["median"] for r in runs]} for w in ("2x150", "2x250")}
        result["insert_size_p1_parent_vs_branch"] = ab
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)
    scfq.lib().scfq_shutdown()


if __name__ == "__main__":
    main()

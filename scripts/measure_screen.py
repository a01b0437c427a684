#!/usr/bin/env python3
"""fq-screen on device-resident input, in ONE process: the inputs of scripts/measure_trim.py (2 x 150 bp and 2 x 250 bp, 2 M pairs each,
built the same way from the same seed), with every 100th pair replaced by a fragment of the small reference.  Reference sets: (a) one
synthetic reference of 5.4 kb, (b) that one and a synthetic one of 4.6 Mb.  Measured per set:
 - S1, the build kernel, for every prefilter setting (off, 16, 32 and 64 KiB), with the table's and the bitmap's fill,
 - S2, the lookup kernel, alone (a sizing call: no S4) on R1 as single-end reads and on the pair, for every prefilter setting,
 - the whole call with device outputs sized by a sizing call and its stages, S4 with the bytes it reads and writes, at the library's
   default setting,
and in the same process on the same R1 the yardstick whose code fq-screen does not touch: T1, the decision kernel of fq-trim, single-end
with its default probes.  S2 is reported as a multiple of it.
Writes profiles/screen/measure.json (--out).

Run it under a time limit of its own:  timeout -k 10 900 python scripts/measure_screen.py
"""
import argparse
import json
import math
import os
import sys

for name in ("SCFQ_SCREEN_TIMING", "SCFQ_TRIM_TIMING"):      # the library brackets its stages with HIP events
    os.environ[name] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "seq-collection_amd", "pyhost"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from measure_insert_size import best, paired      # noqa: E402  (the same inputs)
from measure_merge import random_qualities      # noqa: E402

SETTINGS = (("off", dict(SCFQ_SCREEN_PREFILTER="0")), ("16KiB", dict(SCFQ_SCREEN_PREFILTER="1", SCFQ_SCREEN_PREFILTER_KB="16")),
            ("32KiB", dict(SCFQ_SCREEN_PREFILTER="1", SCFQ_SCREEN_PREFILTER_KB="32")), ("64KiB", dict(SCFQ_SCREEN_PREFILTER="1", SCFQ_SCREEN_PREFILTER_KB="64")))
KNOBS = ("SCFQ_SCREEN_PREFILTER", "SCFQ_SCREEN_PREFILTER_KB")


def spread(v):
    s = sorted(v)
    return {"best": s[0], "median": s[len(s) // 2], "worst": s[-1]}


def with_contaminants(np, rng, rec1, rec2, pairs, length, small):
    """every 100th pair becomes a fragment of `small`: mate 1 its first bases, mate 2 the reverse complement of its last ones"""
    rows1, rows2 = rec1.reshape(pairs, 2 * length + 7), rec2.reshape(pairs, 2 * length + 7)
    comp = np.zeros(256, np.uint8)
    for a, b in zip(b"ACGT", b"TGCA"):
        comp[a] = b
    for p in range(0, pairs, 100):
        frag = int(rng.integers(length, 2 * length))
        at = int(rng.integers(0, small.size - frag))
        rows1[p, 3:3 + length] = small[at:at + length]
        rows2[p, 3:3 + length] = comp[small[at + frag - length:at + frag]][::-1]
    return rec1, rec2


def build(scfq, refs, env, reps):
    """the index under the setting `env`: S1's time over `reps` builds, the last index kept"""
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    times, index = [], None
    for _ in range(reps):
        if index is not None:
            index.close()
        index = scfq.screen_index_host(refs, 31)
        times.append(index.build_ms())
    for k in KNOBS:
        os.environ.pop(k, None)
    return index, spread(times)


def lookups(scfq, index, t1, t2, reps):
    """sizing calls: S2 alone.  (R1 single-end, the pair)"""
    out = {}
    for name, args in (("single_end", (t1.data_ptr(), t1.numel())), ("paired", (t1.data_ptr(), t1.numel(), t2.data_ptr(), t2.numel()))):
        s2 = []
        for _ in range(reps + 1):
            s = scfq.screen_device(index, *args)
            s2.append(scfq.screen_stages()[1])
        s2 = s2[1:]                           # (one warm-up)
        out[name] = dict(s2_ms=spread(s2), s2_ns_per_read=min(s2) * 1e6 / s.reads_in)
    return out


def whole_call(scfq, torch, index, t1, t2, reps):
    size = scfq.screen_device(index, t1.data_ptr(), t1.numel(), t2.data_ptr(), t2.numel())
    outs = [torch.empty(max(int(b), 1), dtype=torch.uint8, device="cuda:0") for b in (size.out1_bytes, size.out2_bytes)]
    stages = []

    def call():
        s = scfq.screen_device(index, t1.data_ptr(), t1.numel(), t2.data_ptr(), t2.numel(), None, *[(o.data_ptr(), o.numel()) for o in outs])
        stages.append(scfq.screen_stages())
        return s

    call()
    stages.clear()
    b, m, s = best(call, reps)
    assert bytes(s) == bytes(call()) and s.reads_in == s.reads_out + s.dropped_reads
    st = [[x[j] for x in stages[:reps]] for j in range(4)]
    moved = int(s.out1_bytes + s.out2_bytes)      # S4 copies every kept record once: as many bytes read as written
    s4 = min(st[3])
    return {"call_ms": {"best": b, "median": m}, "index_lines_ms": spread(st[0]), "s2_ms": spread(st[1]), "s3_scans_ms": spread(st[2]), "s4_ms": spread(st[3]),
            "s4_bytes_read": moved, "s4_bytes_written": moved, "s4_GBps": 2 * moved / (s4 * 1e-3) / 1e9 if s4 > 0 else 0.0,
            "stats": {k: int(getattr(s, k)) for k in ("reads_in", "reads_out", "dropped_reads", "matched_reads", "matched_pairs", "multi_reads", "windows",
                                                      "kmers", "skipped", "hit_kmers", "out1_bytes", "out2_bytes")},
            "rows": [scfq.format_screen_row_tsv(s, index, r) for r in range(len(index.names) + 1)]}


def measure(scfq, torch, np, rng, ref_sets, small, length, classes, block, repeat, reps):
    r1, r2, _ = paired(np, rng, block, length, classes, 0.1)
    r1, r2 = random_qualities(np, rng, r1, block, length), random_qualities(np, rng, r2, block, length)
    r1, r2 = with_contaminants(np, rng, r1, r2, block, length, small)
    t1 = torch.from_numpy(r1).to("cuda:0").repeat(repeat)
    t2 = torch.from_numpy(r2).to("cuda:0").repeat(repeat)
    torch.cuda.synchronize()
    out = {"read_length": length, "pairs": block * repeat, "block_pairs": block, "repeat": repeat, "input_bytes": [t1.numel(), t2.numel()],
           "contaminated_pairs": "every 100th of the block", "n_share": 0.01, "k": 31, "sets": {}}
    # the yardstick: fq-trim's T1 on R1, single-end, default probes
    t1_ms = []
    for _ in range(reps + 1):
        scfq.trim_device(t1.data_ptr(), t1.numel(), None, 0, scfq.trim_opts())
        t1_ms.append(scfq.trim_stages()[1])
    out["trim_t1_single_end_ms"] = spread(t1_ms[1:])
    yard = min(t1_ms[1:])
    for set_name, refs in ref_sets:
        per = {"settings": {}}
        for name, env in SETTINGS:
            index, s1 = build(scfq, refs, env, 3)
            bits = 8 * 1024 * int(env.get("SCFQ_SCREEN_PREFILTER_KB", 0))
            distinct, slots = int(index.summary.distinct), int(index.summary.slots)
            row = dict(s1_ms=s1, distinct=distinct, slots=slots, table_fill=distinct / slots,
                       bitmap_fill_expected=(1 - math.exp(-distinct / bits)) if bits else None, **lookups(scfq, index, t1, t2, reps))
            row["s2_single_end_over_trim_t1"] = row["single_end"]["s2_ms"]["best"] / yard if yard > 0 else 0.0
            per["settings"][name] = row
            index.close()
        index, _ = build(scfq, refs, {}, 1)          # the library's default
        per["default_whole_call_paired"] = whole_call(scfq, torch, index, t1, t2, reps)
        index.close()
        out["sets"][set_name] = per
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--block", type=int, default=250_000)
    ap.add_argument("--repeat", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "screen", "measure.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import scfq

    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    rng = np.random.default_rng(20261019)
    ref_rng = np.random.default_rng(20261020)
    letters = np.frombuffer(b"ACGT", np.uint8)
    small, large = letters[ref_rng.integers(0, 4, 5400)], letters[ref_rng.integers(0, 4, 4_600_000)]
    ref_sets = (("a_5.4kb", [("small", b">small\n" + small.tobytes())]),
                ("b_5.4kb_and_4.6Mb", [("small", b">small\n" + small.tobytes()), ("large", b">large\n" + large.tobytes())]))
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
              "timing": "ms; whole calls: host clock around the synchronous call, best and median of reps after one warm-up; S1, S2, S3 + scans, S4, "
                        "T1: HIP events, best / median / worst of the repeats; S1: three builds per setting",
              "workloads": {}}
    for name, length, classes in (("2x150", 150, (100, 180, 260, 350)), ("2x250", 250, (150, 300, 440, 600))):
        r = measure(scfq, torch, np, rng, ref_sets, small, length, classes, args.block, args.repeat, args.reps)
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

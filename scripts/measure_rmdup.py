#!/usr/bin/env python3
"""fq-rmdup on device-resident input, in ONE process: the 2 x 150 bp pairs of scripts/measure_trim.py (built the same way from the same
seed, 2 M pairs in eight blocks that are each drawn anew: a repeated block would be nothing but duplicates), every record under a name of
its own, and every sixth pair carrying the sequences of the pair five in front of it.  Measured: the whole call of scfq_rmdup_buffers with
device outputs sized by a sizing call and its stages (U1 the key hash, the radix sort, the rounds of U2 + U3, the class sizes, U4 with its
scans, U5 the write kernel), for R1 alone and for the pair, with hash_bits 32, 40 and 64, and in the same process on the same R1 buffer
fq-dedup (by ID) as the yardstick.  Writes profiles/rmdup/measure.json (--out).

Run it under a time limit of its own:  timeout -k 10 900 python scripts/measure_rmdup.py
"""
import argparse
import json
import os
import sys
import time

os.environ["SCFQ_RMDUP_TIMING"] = "1"      # the library brackets its stages with HIP events
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "seq-collection_amd", "pyhost"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from measure_insert_size import best, paired      # noqa: E402  (the same inputs)
from measure_merge import random_qualities, spread      # noqa: E402

LENGTH, CLASSES, EVERY = 150, (100, 180, 260, 350), 6
STAGES = ("index_ms", "u1_hash_ms", "sort_ms", "u2_u3_rounds_ms", "class_sizes_ms", "u4_scans_ms", "u5_write_ms")
HASH_BITS = (32, 40, 64)


def named(np, rec, pairs, first, mate):
    """the block's records under names of their own: "@p\\n" becomes "@<8 digits>/<mate>\\n" """
    rows = rec.reshape(pairs, 2 * LENGTH + 7)
    out = np.empty((pairs, 2 * LENGTH + 7 + 9), np.uint8)
    out[:, 0] = ord("@")
    number = first + np.arange(pairs, dtype=np.int64)
    out[:, 1:9] = (number[:, None] // 10 ** np.arange(7, -1, -1)[None, :]) % 10 + ord("0")
    out[:, 9] = ord("/")
    out[:, 10] = ord("1") + mate
    out[:, 11:] = rows[:, 2:]
    return out


def blocks(np, rng, block, repeat):
    """R1 and R2 as lists of blocks; in each, pair EVERY k + EVERY - 1 has the sequences of pair EVERY k"""
    out = ([], [])
    for r in range(repeat):
        r1, r2, _ = paired(np, rng, block, LENGTH, CLASSES, 0.1)
        recs = [named(np, random_qualities(np, rng, x, block, LENGTH), block, r * block, mate) for mate, x in enumerate((r1, r2))]
        copies = np.arange(EVERY - 1, block, EVERY)
        for rows in recs:
            rows[copies, 12:12 + LENGTH] = rows[copies - (EVERY - 1), 12:12 + LENGTH]
        for k in range(2):
            out[k].append(recs[k].reshape(-1))
    return out


def rmdup_run(scfq, torch, t1, t2, reps, **kw):
    """the whole call with outputs that fit, and its stages"""
    opts = scfq.rmdup_opts(**kw)
    p2, n2 = (t2.data_ptr(), t2.numel()) if t2 is not None else (None, 0)
    size, _ = scfq.rmdup_resident(t1.data_ptr(), t1.numel(), p2, n2, opts)
    outs = [torch.empty(max(int(b), 1), dtype=torch.uint8, device="cuda:0") for b in ((size.out1_bytes, size.out2_bytes) if t2 is not None else (size.out1_bytes,))]
    stages = []

    def call():
        s, _ = scfq.rmdup_resident(t1.data_ptr(), t1.numel(), p2, n2, opts, *[(o.data_ptr(), o.numel()) for o in outs])
        stages.append(scfq.rmdup_stages())
        return s

    call()                                  # warm-up: pool growth, first launches
    stages.clear()
    b, m, s = best(call, reps)
    again = call()
    assert all(getattr(s, k) == getattr(again, k) for k in scfq.RMDUP_STATS_FIELDS) and s.units_in == s.units_out + s.duplicate_units
    st = {name: {k: v for k, v in spread([x[j] for x in stages[:reps]]).items() if k != "all"} for j, name in enumerate(STAGES)}
    written = int(s.out1_bytes + s.out2_bytes)
    u5 = st["u5_write_ms"]["best"]
    return dict(st, call_ms={"best": b, "median": m}, bytes_written=written, u5_written_GBps=written / (u5 * 1e-3) / 1e9 if u5 > 0 else 0.0,
                u1_ns_per_unit=st["u1_hash_ms"]["best"] * 1e6 / s.units_in if s.units_in else 0.0,
                stats={k: int(getattr(s, k)) for k in ("collisions", "rounds", "hash_bits", "prefix", "flags")}, row=scfq.format_rmdup_stats_tsv(s))


def dedup_run(scfq, torch, t1, reps):
    """fq-dedup (by ID) on the same buffer: every name is its own, nothing is removed"""
    size, _ = scfq.dedup_device(t1.data_ptr(), t1.numel())
    out = torch.empty(max(int(size), 1), dtype=torch.uint8, device="cuda:0")

    def call():
        return scfq.dedup_device(t1.data_ptr(), t1.numel(), out.data_ptr(), out.numel())

    call()
    b, m, (nbytes, st) = best(call, reps)
    return {"call_ms": {"best": b, "median": m}, "bytes_written": int(nbytes), "records_in": int(st.total_reads), "records_out": int(st.records_out),
            "duplicates": int(st.duplicates)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--block", type=int, default=250_000)
    ap.add_argument("--repeat", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rmdup", "measure.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import scfq

    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    t0 = time.perf_counter()
    rng = np.random.default_rng(20261019)
    b1, b2 = blocks(np, rng, args.block, args.repeat)
    t1 = torch.cat([torch.from_numpy(b).to("cuda:0") for b in b1])
    t2 = torch.cat([torch.from_numpy(b).to("cuda:0") for b in b2])
    del b1, b2
    torch.cuda.synchronize()
    print("inputs built in %.1f s" % (time.perf_counter() - t0), flush=True)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "pairs": args.block * args.repeat, "read_length": LENGTH,
              "block_pairs": args.block, "blocks": args.repeat, "planted": "pair %d k + %d has the sequences of pair %d k" % (EVERY, EVERY - 1, EVERY),
              "input_bytes": [t1.numel(), t2.numel()],
              "timing": "ms; whole calls: host clock around the synchronous call, best and median of reps after one warm-up; the stages: HIP events (the "
                        "line indexes of paired input: host clock), best, median and worst of the repeats",
              "not_measured": ["hardware counters of U1 and U3", "reads longer than 150 bases", "interleaved input", "host and file outputs, the command",
                               "a class of hundreds of thousands of members beside the planted pairs", "U1 fused into the index pass"],
              "workloads": {}}
    for name, second in (("r1_alone", None), ("pairs", t2), ("pairs_swapped", t2)):
        w = {}
        for bits in HASH_BITS:
            w["hash_bits_%d" % bits] = rmdup_run(scfq, torch, t1, second, args.reps, hash_bits=bits, swapped=name == "pairs_swapped")
            print(name, bits, json.dumps(w["hash_bits_%d" % bits]["call_ms"]), flush=True)
        result["workloads"][name] = w
    result["workloads"]["r1_alone"]["prefix_50"] = rmdup_run(scfq, torch, t1, None, args.reps, prefix=50)
    d = dedup_run(scfq, torch, t1, args.reps)
    result["dedup_by_id_on_r1"] = d
    calls = {bits: result["workloads"]["r1_alone"]["hash_bits_%d" % bits]["call_ms"]["best"] for bits in HASH_BITS}
    result["r1_call_over_dedup_call"] = {str(bits): v / d["call_ms"]["best"] for bits, v in calls.items()}
    result["fastest_hash_bits"] = {name: min(HASH_BITS, key=lambda bits: w["hash_bits_%d" % bits]["call_ms"]["best"]) for name, w in result["workloads"].items()}
    print(json.dumps({"dedup": d["call_ms"], "ratio": result["r1_call_over_dedup_call"], "fastest": result["fastest_hash_bits"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)
    scfq.lib().scfq_shutdown()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""fq-kcount on the device-resident synthetic Illumina workload (150 bp), in ONE process: H1 (the counting kernel of the last
pass), H2 (finish) and the whole call at k = 13, 21 and 31, plain and canonical, with the automatic table; at k = 21 with
table_bits one step below and one step above the automatic size; H3 (the histogram at 10002 bins); and on the same buffer
scfq_kmers_buffer at k = 12, the yardstick (tier B: a no-return 64-bit add per run on a dense table).  Two buffers: the 10 GB
one of the other measurements, and its first GB — the synthetic reads are random letters, so nearly every 21-mer of 10 GB is
distinct (3.6 G keys) and does not fit a table of 2^32 slots within the probe bound; what the library answers then (SCFQ_EFULL,
after how many passes and milliseconds) is recorded instead of a time.
Writes profiles/kcount/measure.json (--out).

Run it under a time limit of its own:  timeout -k 10 900 python scripts/measure_kcount.py
"""
import argparse
import json
import os
import sys
import time

os.environ["SCFQ_KCOUNT_TIMING"] = "1"     # the library brackets its stages with HIP events (read before its first call)
os.environ["SCFQ_KMERS_TIMING"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "seq-collection_amd", "pyhost"))


def stats(ms):
    return {"best": min(ms), "median": sorted(ms)[len(ms) // 2]}


def measure_kcount(scfq, ptr, n, k, flags, table_bits, reps, hist=False):
    """the whole call without the table's readers; H1 / H2 from the library's events"""
    calls, h1, h2, h3 = [], [], [], []
    s = None
    for rep in range(reps + 1):            # (the first one is the warm-up: pool growth, first launches)
        t0 = time.perf_counter()
        try:
            s, t = scfq.kcount_device(ptr, n, k=k, flags=flags, table_bits=table_bits, table=hist)
        except scfq.ScfqError as e:
            return {"rc": e.rc, "error": str(e), "call_ms": (time.perf_counter() - t0) * 1e3}
        ms = (time.perf_counter() - t0) * 1e3
        st = scfq.kcount_stages()
        if hist:
            t.hist(10002)
            h3.append(scfq.kcount_stages()[3])
            t.close()
        if rep:
            calls.append(ms), h1.append(st[1]), h2.append(st[2])
    assert s.windows == s.kmers + s.skipped
    out = {"rc": 0, "call_ms": stats(calls), "h1_count_ms": stats(h1), "h2_finish_ms": stats(h2), "index_ms": st[0],
           "windows": s.windows, "kmers": s.kmers, "skipped": s.skipped, "distinct": s.distinct, "unique": s.unique, "max_count": s.max_count,
           "slots": s.slots, "passes": s.passes, "load": s.distinct / s.slots, "table_bytes": 16 * s.slots,
           "h1_kmers_per_s": s.kmers / (min(h1) * 1e-3) if min(h1) > 0 else 0.0, "h1_scanned_GBps": n / (min(h1) * 1e-3) / 1e9 if min(h1) > 0 else 0.0}
    if hist:
        out["h3_hist_10002_bins_ms"] = stats(h3[1:])
    return out


def measure_tier_b(scfq, ptr, n, reps):
    ms = []
    for rep in range(reps + 1):
        s, _ = scfq.kmers_device(ptr, n, 12, 0)
        if rep:
            ms.append(scfq.kmers_stages()[1])
    return {"k": 12, "count_ms": stats(ms), "kmers": s.kmers, "distinct": s.distinct}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=10_000_000_000)
    ap.add_argument("--small-bytes", type=int, default=1_000_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kcount", "measure.json"))
    args = ap.parse_args()
    import torch
    import scfq

    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    kind, seed = 0, 20260101
    plan = scfq.synth_plan(kind, seed, args.bytes)
    buf = torch.empty(plan.bytes + 4096, dtype=torch.uint8, device="cuda:0")
    info = scfq.synth_device(kind, seed, plan.records, buf.data_ptr(), plan.bytes)
    torch.cuda.synchronize()
    small = scfq.synth_plan(kind, seed, args.small_bytes)       # (the same records from the start: a prefix of the buffer)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
              "timing": "ms; best and median of reps after one warm-up; call: host clock around the synchronous scfq_kcount_buffers (summary only); "
                        "index: host clock around the index call inside it; H1 (the last pass, all inputs, without the clear of the table), H2, "
                        "H3 and tier B's counting kernel: HIP events",
              "workloads": {}}
    can = scfq.SCFQ_KCOUNT_CANONICAL
    for name, n in (("illumina_10GB", plan.bytes), ("illumina_1GB_prefix", small.bytes)):
        ptr = buf.data_ptr()
        w = {"input_bytes": n, "tier_b": measure_tier_b(scfq, ptr, n, args.reps), "k": {}}
        print(name, "tier B", json.dumps(w["tier_b"]), flush=True)
        for k in (13, 21, 31):
            for mode, flags in (("plain", 0), ("canonical", can)):
                r = measure_kcount(scfq, ptr, n, k, flags, 0, args.reps, hist=(k == 21 and flags == 0))
                if r["rc"] == 0:
                    r["h1_over_tier_b"] = r["h1_count_ms"]["best"] / w["tier_b"]["count_ms"]["best"]
                w["k"].setdefault(str(k), {})[mode] = r
                print(name, k, mode, json.dumps(r), flush=True)
        auto = w["k"]["21"]["plain"]
        if auto["rc"] == 0:
            bits = auto["slots"].bit_length() - 1
            for label, b in (("one_step_below", bits - 1), ("one_step_above", bits + 1)):
                r = measure_kcount(scfq, ptr, n, 21, 0, b, args.reps) if 10 <= b <= 32 else {"rc": None, "error": "outside 10 .. 32"}
                w["k"]["21"]["table_bits_" + label] = dict(r, table_bits=b)
                print(name, 21, label, json.dumps(r), flush=True)
        result["workloads"][name] = w
    result["reads_10GB"], result["bases_10GB"] = info.records, info.bases
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)
    scfq.lib().scfq_shutdown()


if __name__ == "__main__":
    main()

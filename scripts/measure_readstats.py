#!/usr/bin/env python3
"""fq-readstats on the device-resident 10 GB synthetic workloads (Illumina 150 bp, Nanopore 500 bp .. 50 kb), in ONE process:
the stages of scfq_read_stats_buffer (line index, R1, R2), the whole call, and on the same buffer scfq_count_buffer with
SCFQ_QUAL_HIST and the sizing call of scfq_dedup_buffer.  Writes profiles/readstats/measure.json (--out).

Run it under a time limit of its own:  timeout -k 10 600 python scripts/measure_readstats.py
"""
import argparse
import json
import os
import sys
import time

os.environ["SCFQ_READSTATS_TIMING"] = "1"      # the library brackets R1 / R2 with HIP events (read before its first call)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "seq-collection_amd", "pyhost"))

HBM_PEAK_GBPS = 8000.0


def best(fn, reps):
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t) * 1e3)
    return min(out), sorted(out)[len(out) // 2], r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=10_000_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "readstats", "measure.json"))
    args = ap.parse_args()
    import torch
    import scfq

    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    result = {"device": torch.cuda.get_device_name(0), "bytes_asked": args.bytes, "reps": args.reps, "hbm_peak_GBps": HBM_PEAK_GBPS,
              "timing": "ms; whole calls: host clock around the synchronous call, best and median of reps after one warm-up; "
                        "index: host clock around the synchronous index call inside the read-stats call; r1 / r2: HIP events",
              "workloads": {}}
    for name, kind, seed in (("illumina", 0, 20260101), ("nanopore", 1, 20260103)):
        plan = scfq.synth_plan(kind, seed, args.bytes)
        buf = torch.empty(plan.bytes + 4096, dtype=torch.uint8, device="cuda:0")
        info = scfq.synth_device(kind, seed, plan.records, buf.data_ptr(), plan.bytes)
        torch.cuda.synchronize()
        ptr, n = buf.data_ptr(), plan.bytes
        stages = []

        def read_stats():
            s = scfq.read_stats_device(ptr, n)
            stages.append(scfq.read_stats_stages())
            return s

        read_stats()                                          # warm-up: pool growth, first launches
        stages.clear()
        rs_best, rs_med, s = best(read_stats, args.reps)
        scfq.count_device(ptr, n, flags=scfq.SCFQ_QUAL_HIST)
        c_best, c_med, c = best(lambda: scfq.count_device(ptr, n, flags=scfq.SCFQ_QUAL_HIST), args.reps)
        scfq.dedup_device(ptr, n)
        d_best, d_med, d = best(lambda: scfq.dedup_device(ptr, n), args.reps)
        assert (s.reads, s.bases, s.gc_bases, s.n_bases) == (c.reads, c.bases, c.gc_bases, c.n_bases) == \
               (info.records, info.bases, info.gc_bases, info.n_bases)
        assert s.qual_bytes == sum(c.qual_hist) and s.qual_sum == sum(b * k for b, k in enumerate(c.qual_hist))
        st = [min(x[k] for x in stages) for k in range(4)]
        r1_gbps = n / (st[1] * 1e-3) / 1e9 if st[1] > 0 else 0.0
        result["workloads"][name] = {
            "input_bytes": n, "reads": s.reads, "lines": s.lines, "min_len": s.min_len, "max_len": s.max_len, "n50": s.n50, "l50": s.l50,
            "n90": s.n90, "l90": s.l90, "row": scfq.format_read_stats_tsv(s),
            "index_ms": st[0], "r1_ms": st[1], "r2_sums_hist_ms": st[2], "r2_nx_ms": st[3],
            "r1_scanned_GBps": r1_gbps, "r1_fraction_of_hbm_peak": r1_gbps / HBM_PEAK_GBPS,
            "r1_traffic_bytes_model": n + 8 * s.lines + 40 * s.reads,
            "read_stats_call_ms": {"best": rs_best, "median": rs_med},
            "count_qual_hist_call_ms": {"best": c_best, "median": c_med},
            "dedup_sizing_call_ms": {"best": d_best, "median": d_med},
            "read_stats_over_dedup": rs_best / d_best,
        }
        print(name, json.dumps(result["workloads"][name]), flush=True)
        del buf
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)
    scfq.lib().scfq_shutdown()


if __name__ == "__main__":
    main()

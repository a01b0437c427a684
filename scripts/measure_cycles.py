#!/usr/bin/env python3
"""fq-cycles on the device-resident 10 GB synthetic workloads (Illumina 150 bp, Nanopore 500 bp .. 50 kb), in ONE process:
the stages of scfq_cycles_buffer (line index, line pass, counting kernel C1, finish), the whole call, and on the same buffer
scfq_read_stats_buffer (the yardstick) and scfq_count_buffer with SCFQ_QUAL_HIST.  Writes profiles/cycles/measure.json (--out).

Run it under a time limit of its own:  timeout -k 10 600 python scripts/measure_cycles.py
"""
import argparse
import json
import os
import sys
import time

os.environ["SCFQ_CYCLES_TIMING"] = "1"      # the library brackets its stages with HIP events (read before its first call)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cycles", "measure.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import scfq

    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    result = {"device": torch.cuda.get_device_name(0), "bytes_asked": args.bytes, "reps": args.reps, "hbm_peak_GBps": HBM_PEAK_GBPS,
              "timing": "ms; whole calls: host clock around the synchronous call, best and median of reps after one warm-up; "
                        "index: host clock around the synchronous index call inside the cycles call; line pass / c1 / finish: HIP events",
              "workloads": {}}
    for name, kind, seed in (("illumina", 0, 20260101), ("nanopore", 1, 20260103)):
        plan = scfq.synth_plan(kind, seed, args.bytes)
        buf = torch.empty(plan.bytes + 4096, dtype=torch.uint8, device="cuda:0")
        info = scfq.synth_device(kind, seed, plan.records, buf.data_ptr(), plan.bytes)
        torch.cuda.synchronize()
        ptr, n = buf.data_ptr(), plan.bytes
        sizing, _ = scfq.cycles_device(ptr, n, 0)                # warm-up and the sizing call: pool growth, first launches
        cap = max(sizing.max_seq_len, sizing.max_qual_len)
        rows = np.zeros((cap, 8), dtype=np.int64)
        stages = []

        def cycles():
            s, _ = scfq.cycles_device(ptr, n, rows)
            stages.append(scfq.cycles_stages())
            return s

        cycles()
        stages.clear()
        cy_best, cy_med, s = best(cycles, args.reps)
        z_best, z_med, _ = best(lambda: scfq.cycles_device(ptr, n, 0), args.reps)
        scfq.read_stats_device(ptr, n)
        rs_best, rs_med, rs = best(lambda: scfq.read_stats_device(ptr, n), args.reps)
        scfq.count_device(ptr, n, flags=scfq.SCFQ_QUAL_HIST)
        c_best, c_med, c = best(lambda: scfq.count_device(ptr, n, flags=scfq.SCFQ_QUAL_HIST), args.reps)
        t = s.total
        assert (s.reads, t.bases, t.g + t.c, t.n) == (c.reads, c.bases, c.gc_bases, c.n_bases) == (info.records, info.bases, info.gc_bases, info.n_bases)
        assert (t.quals, t.qual_sum) == (rs.qual_bytes, rs.qual_sum) and s.cycles == cap and rows.sum(axis=0).tolist() == [getattr(t, f) for f in scfq.CYCLE_FIELDS]
        st = [min(x[k] for x in stages) for k in range(4)]
        c1_gbps = n / (st[2] * 1e-3) / 1e9 if st[2] > 0 else 0.0
        result["workloads"][name] = {
            "input_bytes": n, "reads": s.reads, "lines": s.lines, "max_seq_len": s.max_seq_len, "max_qual_len": s.max_qual_len, "cycles": s.cycles,
            "row_1": scfq.format_cycle_row_tsv(rows[0]), "total": scfq.format_cycle_row_tsv(t),
            "index_ms": st[0], "line_pass_ms": st[1], "c1_ms": st[2], "finish_ms": st[3],
            "c1_scanned_GBps": c1_gbps, "c1_fraction_of_hbm_peak": c1_gbps / HBM_PEAK_GBPS,
            "c1_traffic_bytes_model": n + 8 * s.lines,
            "cycles_call_ms": {"best": cy_best, "median": cy_med},
            "cycles_sizing_call_ms": {"best": z_best, "median": z_med},
            "read_stats_call_ms": {"best": rs_best, "median": rs_med},
            "count_qual_hist_call_ms": {"best": c_best, "median": c_med},
            "cycles_over_read_stats": cy_best / rs_best,
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

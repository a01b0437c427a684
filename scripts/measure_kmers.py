#!/usr/bin/env python3
"""fq-kmers on the device-resident 10 GB synthetic workloads (Illumina 150 bp, Nanopore 500 bp .. 50 kb), in ONE process:
for k in 1 4 7 8 10 12, plain and canonical, the whole scfq_kmers_buffer call (the sizing call: the summary without the copy of
the table) and its stages (line index, counting kernel M1, finish), k-mers per second and scanned GB/s, and on the same buffer
scfq_cycles_buffer (the yardstick).  Then the poly-G input (one line of G with an N every 1000 bytes) at k = 8 and 12 with and
without the merge of adjacent lanes (SCFQ_KMERS_MERGE=0, read once per process: a child process).
Writes profiles/kmers/measure.json (--out).

Run it under a time limit of its own:  timeout -k 10 900 python scripts/measure_kmers.py
"""
import argparse
import json
import os
import subprocess
import sys
import time

os.environ["SCFQ_KMERS_TIMING"] = "1"      # the library brackets its stages with HIP events (read before its first call)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "seq-collection_amd", "pyhost"))

KS = (1, 4, 7, 8, 10, 12)


def best(fn, reps):
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t) * 1e3)
    return min(out), sorted(out)[len(out) // 2], r


def measure_call(scfq, ptr, n, k, flags, reps):
    stages = []

    def call():
        s, _ = scfq.kmers_device(ptr, n, k, flags)
        stages.append(scfq.kmers_stages())
        return s

    call()                                  # warm-up: pool growth, first launches
    stages.clear()
    b, m, s = best(call, reps)
    st = [min(x[j] for x in stages) for j in range(4)]
    assert s.windows == s.kmers + s.skipped
    return {"call_ms": {"best": b, "median": m}, "index_ms": st[0], "count_ms": st[1], "finish_ms": st[2],
            "windows": s.windows, "kmers": s.kmers, "skipped": s.skipped, "short_lines": s.short_lines, "distinct": s.distinct,
            "max_count": s.max_count, "table_bytes": 8 * s.table_entries,
            "count_kmers_per_s": s.kmers / (st[1] * 1e-3) if st[1] > 0 else 0.0,
            "count_scanned_GBps": n / (st[1] * 1e-3) / 1e9 if st[1] > 0 else 0.0}


def poly_g(torch, bytes_):
    line = torch.full((bytes_,), ord("G"), dtype=torch.uint8, device="cuda:0")
    line[999::1000] = ord("N")
    return torch.cat([torch.frombuffer(bytearray(b"@g\n"), dtype=torch.uint8).to("cuda:0"), line,
                      torch.frombuffer(bytearray(b"\n+\n\n"), dtype=torch.uint8).to("cuda:0")])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=10_000_000_000)
    ap.add_argument("--poly-bytes", type=int, default=1 << 30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmers", "measure.json"))
    ap.add_argument("--poly-only", action="store_true", help="(the child process of the merge comparison) print the poly-G numbers as JSON")
    args = ap.parse_args()
    import numpy as np
    import torch
    import scfq

    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    if args.poly_only:
        buf = poly_g(torch, args.poly_bytes)
        torch.cuda.synchronize()
        out = {"k%d" % k: measure_call(scfq, buf.data_ptr(), buf.numel(), k, 0, args.reps) for k in (7, 8, 12)}
        print(json.dumps(out))
        scfq.lib().scfq_shutdown()
        return
    result = {"device": torch.cuda.get_device_name(0), "bytes_asked": args.bytes, "reps": args.reps,
              "timing": "ms; whole calls: host clock around the synchronous sizing call (cap = 0: everything but the copy of the table), best "
                        "and median of reps after one warm-up; index: host clock around the synchronous index call inside the call; "
                        "count / finish: HIP events",
              "workloads": {}}
    for name, kind, seed in (("illumina", 0, 20260101), ("nanopore", 1, 20260103)):
        plan = scfq.synth_plan(kind, seed, args.bytes)
        buf = torch.empty(plan.bytes + 4096, dtype=torch.uint8, device="cuda:0")
        info = scfq.synth_device(kind, seed, plan.records, buf.data_ptr(), plan.bytes)
        torch.cuda.synchronize()
        ptr, n = buf.data_ptr(), plan.bytes
        sizing, _ = scfq.cycles_device(ptr, n, 0)
        rows = np.zeros((max(sizing.max_seq_len, sizing.max_qual_len), 8), dtype=np.int64)
        scfq.cycles_device(ptr, n, rows)
        cy_best, cy_med, (cy, _) = best(lambda: scfq.cycles_device(ptr, n, rows), args.reps)
        w = {"input_bytes": n, "reads": info.records, "bases": info.bases, "cycles_call_ms": {"best": cy_best, "median": cy_med}, "k": {}}
        for k in KS:
            for mode, flags in (("plain", 0), ("canonical", scfq.SCFQ_KMERS_CANONICAL)):
                r = measure_call(scfq, ptr, n, k, flags, args.reps)
                r["call_over_cycles_call"] = r["call_ms"]["best"] / cy_best
                w["k"].setdefault(str(k), {})[mode] = r
                print(name, k, mode, json.dumps(r), flush=True)
            if k == 1:
                p = w["k"]["1"]["plain"]
                assert p["windows"] == info.bases == cy.total.bases and p["skipped"] == info.n_bases
        b, m, (s, table) = best(lambda: scfq.kmers_device(ptr, n, 12, 0, True), 3)
        w["k12_full_call_with_128MiB_table_to_host_ms"] = {"best": b, "median": m}
        assert int(table.sum()) == s.kmers
        result["workloads"][name] = w
        del buf
        torch.cuda.empty_cache()
    # what the merge of adjacent lanes buys where every window of a wave is the same k-mer
    poly = {}
    for merge in ("1", "0"):
        env = dict(os.environ, SCFQ_KMERS_MERGE=merge)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--poly-only", "--poly-bytes", str(args.poly_bytes), "--reps", str(args.reps)],
                             env=env, capture_output=True, text=True, timeout=300, check=True).stdout
        poly["merge_" + merge] = json.loads(out.strip().splitlines()[-1])
        print("poly-G merge", merge, json.dumps(poly["merge_" + merge]), flush=True)
    result["poly_g"] = {"bytes": args.poly_bytes, **poly}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)
    scfq.lib().scfq_shutdown()


if __name__ == "__main__":
    main()

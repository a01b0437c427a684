#!/usr/bin/env python3
"""fq-adapters on the device-resident 10 GB synthetic workloads (Illumina 150 bp, Nanopore 500 bp .. 50 kb), in ONE process:
with the built-in set (seven 12-mers), a single 12-mer and a single 32-mer (the 64-bit compares), the sizing call (cap = 0) and a
full call (1000 rows) of scfq_adapters_buffer and its stages (line index, matching kernel A1, rows A2, finish A3), and in the same
process and on the same buffer scfq_kmers_buffer at k = 12 plain: its counting kernel M1 is the yardstick of A1 (the same
partition and the same loads).  Then one poly-A line of 1 GiB with the built-in set: every chunk holds the probe and all of them
belong to one word of the first-occurrence table.
Writes profiles/adapters/measure.json (--out).

Run it under a time limit of its own:  timeout -k 10 900 python scripts/measure_adapters.py
"""
import argparse
import json
import os
import sys
import time

os.environ["SCFQ_ADAPTERS_TIMING"] = "1"    # the library brackets its stages with HIP events (read before its first call)
os.environ["SCFQ_KMERS_TIMING"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "seq-collection_amd", "pyhost"))

LONG = "AGATCGGAAGAGCACACGTCTGAACTCCAGTC"      # 32 letters


def best(fn, reps):
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t) * 1e3)
    return min(out), sorted(out)[len(out) // 2], r


def measure_call(scfq, ptr, n, probes, cap, reps):
    stages = []

    def call():
        s, _ = scfq.adapters_device(ptr, n, probes, cap)
        stages.append(scfq.adapters_stages())
        return s

    call()                                  # warm-up: pool growth, first launches
    stages.clear()
    b, m, s = best(call, reps)
    st = [min(x[j] for x in stages) for j in range(4)]
    return {"call_ms": {"best": b, "median": m}, "index_ms": st[0], "match_ms": st[1], "rows_ms": st[2], "finish_ms": st[3],
            "n_probes": s.n_probes, "hits": list(s.hits)[:s.n_probes], "reads_with": list(s.total.first)[:s.n_probes], "reads_with_any": s.total.any,
            "max_seq_len": s.max_seq_len, "positions": s.positions,
            "match_scanned_GBps": n / (st[1] * 1e-3) / 1e9 if st[1] > 0 else 0.0}


def kmers12(scfq, ptr, n, reps):
    stages = []

    def call():
        s, _ = scfq.kmers_device(ptr, n, 12, 0)
        stages.append(scfq.kmers_stages())
        return s

    call()
    stages.clear()
    b, m, s = best(call, reps)
    st = [min(x[j] for x in stages) for j in range(4)]
    return {"call_ms": {"best": b, "median": m}, "index_ms": st[0], "count_ms": st[1], "finish_ms": st[2], "kmers": s.kmers,
            "count_scanned_GBps": n / (st[1] * 1e-3) / 1e9 if st[1] > 0 else 0.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=10_000_000_000)
    ap.add_argument("--poly-bytes", type=int, default=1 << 30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adapters", "measure.json"))
    args = ap.parse_args()
    import torch
    import scfq

    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    builtin = scfq.adapters_default()
    result = {"device": torch.cuda.get_device_name(0), "bytes_asked": args.bytes, "reps": args.reps,
              "builtin": [list(x) for x in builtin],
              "timing": "ms; whole calls: host clock around the synchronous call, best and median of reps after one warm-up; index: host "
                        "clock around the synchronous index call inside the call; match / rows / finish and the k-mer count: HIP events",
              "workloads": {}}
    sets = (("builtin", None), ("single_12", [builtin[0][1]]), ("single_32", [LONG]))
    for name, kind, seed in (("illumina", 0, 20260101), ("nanopore", 1, 20260103)):
        plan = scfq.synth_plan(kind, seed, args.bytes)
        buf = torch.empty(plan.bytes + 4096, dtype=torch.uint8, device="cuda:0")
        info = scfq.synth_device(kind, seed, plan.records, buf.data_ptr(), plan.bytes)
        torch.cuda.synchronize()
        ptr, n = buf.data_ptr(), plan.bytes
        w = {"input_bytes": n, "reads": info.records, "bases": info.bases, "kmers_k12_plain": kmers12(scfq, ptr, n, args.reps), "probes": {}}
        print(name, "kmers k=12", json.dumps(w["kmers_k12_plain"]), flush=True)
        for label, probes in sets:
            for mode, cap in (("sizing", 0), ("full_1000", 1000)):
                r = measure_call(scfq, ptr, n, probes, cap, args.reps)
                r["match_over_kmers_count"] = r["match_ms"] / w["kmers_k12_plain"]["count_ms"] if w["kmers_k12_plain"]["count_ms"] > 0 else 0.0
                w["probes"].setdefault(label, {})[mode] = r
                print(name, label, mode, json.dumps(r), flush=True)
        result["workloads"][name] = w
        del buf
        torch.cuda.empty_cache()
    # one line of A: the load in front of the atomic and the hand-over between the lanes of a wave keep the atomics few
    L = args.poly_bytes
    buf = torch.cat([torch.frombuffer(bytearray(b"@a\n"), dtype=torch.uint8).to("cuda:0"), torch.full((L,), ord("A"), dtype=torch.uint8, device="cuda:0"),
                     torch.frombuffer(bytearray(b"\n+\n\n"), dtype=torch.uint8).to("cuda:0")])
    torch.cuda.synchronize()
    r = measure_call(scfq, buf.data_ptr(), buf.numel(), None, 1000, args.reps)
    assert r["hits"][4] == L - 11 and r["reads_with_any"] == 1, r
    r["kmers_k12_plain"] = kmers12(scfq, buf.data_ptr(), buf.numel(), args.reps)
    result["poly_a"] = {"bytes": L, **r}
    print("poly-A", json.dumps(result["poly_a"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)
    scfq.lib().scfq_shutdown()


if __name__ == "__main__":
    main()

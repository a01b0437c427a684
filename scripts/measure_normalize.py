#!/usr/bin/env python3
"""fq-normalize on reads with real coverage, resident in HBM, in ONE process: about 2 M reads of 150 bp drawn from either strand of a
synthetic genome of 4 Mb with 1 % substitution errors (about 75 x; random-letter reads would have depth 1 everywhere and say nothing),
k = 21 canonical, target 40, min_depth 3.  Measured: N1 (the depth kernel), N2 with its scans and N3 (the write kernel) against a table
that is given, the whole call of that form, and the whole two-pass call (table = NULL).  Yardsticks on the same input in the same
process: fq-kcount's H1, the pass normalization cannot avoid, and fq-screen's S2 with the genome as the reference, the nearest existing
lookup kernel, with S4 beside N3.  A child process with SCFQ_NORM_LDS_WINDOWS=64 (read once per process) measures N1 on the same input
when every read keeps its counts in device memory.
Writes profiles/normalize/measure.json (--out).

Run it under a time limit of its own:  timeout -k 10 600 python scripts/measure_normalize.py
"""
import argparse
import json
import os
import subprocess
import sys
import time

for name in ("SCFQ_NORM_TIMING", "SCFQ_KCOUNT_TIMING", "SCFQ_SCREEN_TIMING"):      # the library brackets its stages with HIP events
    os.environ[name] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "seq-collection_amd", "pyhost"))

K, TARGET, MIN_DEPTH, READ_LEN = 21, 40, 3, 150


def stats(ms):
    return {"best": min(ms), "median": sorted(ms)[len(ms) // 2]}


def make_input(torch, genome_bases, reads, seed):
    """(genome as a FASTA on the host, the FASTQ on the device): fixed-width names, so that a record has 314 bytes"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    genome = torch.randint(0, 4, (genome_bases,), generator=g, device="cuda", dtype=torch.int64)
    rec = 1 + 8 + 1 + READ_LEN + 3 + READ_LEN + 1
    out = torch.empty((reads, rec), dtype=torch.uint8, device="cuda")
    step = 1 << 18
    for r0 in range(0, reads, step):
        n = min(step, reads - r0)
        start = torch.randint(0, genome_bases - READ_LEN + 1, (n, 1), generator=g, device="cuda")
        codes = genome[start + torch.arange(READ_LEN, device="cuda")]
        flip = torch.randint(0, 2, (n, 1), generator=g, device="cuda") == 1
        codes = torch.where(flip, 3 - codes.flip(1), codes)
        err = torch.randint(0, 100, (n, READ_LEN), generator=g, device="cuda") == 0
        codes = torch.where(err, (codes + torch.randint(1, 4, (n, READ_LEN), generator=g, device="cuda")) & 3, codes)
        block = out[r0:r0 + n]
        block[:, 0] = ord("@")
        idx = torch.arange(r0, r0 + n, device="cuda")
        for d in range(8):
            block[:, 1 + d] = (48 + (idx // 10 ** (7 - d)) % 10).to(torch.uint8)
        block[:, 9] = 10
        block[:, 10:10 + READ_LEN] = letters[codes]
        block[:, 10 + READ_LEN] = 10
        block[:, 11 + READ_LEN] = ord("+")
        block[:, 12 + READ_LEN] = 10
        block[:, 13 + READ_LEN:13 + 2 * READ_LEN] = ord("I")
        block[:, 13 + 2 * READ_LEN] = 10
    fasta = b">genome\n" + letters[genome].cpu().numpy().tobytes() + b"\n"
    torch.cuda.synchronize()
    return fasta, out.reshape(-1)


def measure_norm(scfq, torch, table, opts, buf, out, reps):
    calls, stages = [], []
    s = None
    for rep in range(reps + 1):            # (the first one is the warm-up: pool growth, first launches)
        t0 = time.perf_counter()
        s, _ = scfq.norm_device(table, buf.data_ptr(), buf.numel(), opts=opts, out1=(out.data_ptr(), out.numel()) if out is not None else None)
        ms = (time.perf_counter() - t0) * 1e3
        if rep:
            calls.append(ms)
            stages.append(scfq.norm_stages() + scfq.kcount_stages()[1:2])
    r = {"call_ms": stats(calls), "index_ms": stats([x[0] for x in stages]), "n1_depth_ms": stats([x[1] for x in stages]),
         "n2_decide_scans_ms": stats([x[2] for x in stages]), "n3_write_ms": stats([x[3] for x in stages]),
         "units_in": s.units_in, "units_out": s.units_out, "dropped_low": s.dropped_low, "dropped_high": s.dropped_high, "kmers": s.kmers,
         "weak_kmers": s.weak_kmers, "out1_bytes": s.out1_bytes, "slots": s.slots, "distinct": s.distinct, "passes": s.passes}
    n1 = r["n1_depth_ms"]["best"]
    r["n1_kmers_per_s"] = s.kmers / (n1 * 1e-3) if n1 > 0 else 0.0
    if out is not None and r["n3_write_ms"]["best"] > 0:
        r["n3_written_GBps"] = s.out1_bytes / (r["n3_write_ms"]["best"] * 1e-3) / 1e9
    if table is None:
        r["h1_count_ms_inside"] = stats([x[4] for x in stages])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=4_000_000)
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only-n1", action="store_true", help="the child: N1 against a given table, one JSON line on stdout")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normalize", "measure.json"))
    args = ap.parse_args()
    import torch
    import scfq

    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    scfq.set_wait_stream(torch.cuda.current_stream().cuda_stream)
    fasta, buf = make_input(torch, args.genome, args.reads, 20261027)
    n = buf.numel()
    opts = scfq.norm_opts(target=TARGET, min_depth=MIN_DEPTH)
    can = scfq.SCFQ_KCOUNT_CANONICAL
    if args.only_n1:
        s, table = scfq.kcount_device(buf.data_ptr(), n, k=K, flags=can)
        with table:
            r = measure_norm(scfq, torch, table, opts, buf, None, args.reps)
        print(json.dumps({"lds_windows_env": os.environ.get("SCFQ_NORM_LDS_WINDOWS"), "n1_depth_ms": r["n1_depth_ms"], "call_ms": r["call_ms"],
                          "units_out": r["units_out"], "kmers": r["kmers"]}))
        scfq.lib().scfq_shutdown()
        return
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "input_bytes": n, "reads": args.reads, "read_length": READ_LEN,
              "genome_bases": args.genome, "k": K, "canonical": True, "target": TARGET, "min_depth": MIN_DEPTH,
              "timing": "ms; best and median of reps after one warm-up; call: host clock around the synchronous call; index: host clock around the "
                        "index call inside it; N1, N2 with its scans, N3, H1, S2 and S4: HIP events"}
    out = torch.empty(n + 4096, dtype=torch.uint8, device="cuda")
    # H1: the counting pass, and the table for the rest
    h1, calls = [], []
    for rep in range(args.reps + 1):
        t0 = time.perf_counter()
        s, table = scfq.kcount_device(buf.data_ptr(), n, k=K, flags=can, table=(rep == args.reps))
        if rep:
            calls.append((time.perf_counter() - t0) * 1e3)
            h1.append(scfq.kcount_stages()[1])
    result["kcount"] = {"call_ms": stats(calls), "h1_count_ms": stats(h1), "kmers": s.kmers, "distinct": s.distinct, "slots": s.slots, "passes": s.passes,
                        "max_count": s.max_count, "h1_kmers_per_s": s.kmers / (min(h1) * 1e-3) if min(h1) > 0 else 0.0}
    print("kcount", json.dumps(result["kcount"]), flush=True)
    with table:
        result["given_table"] = measure_norm(scfq, torch, table, opts, buf, out, args.reps)
        print("given table", json.dumps(result["given_table"]), flush=True)
        result["given_table_sizing_call"] = measure_norm(scfq, torch, table, opts, buf, None, args.reps)
    result["two_pass"] = measure_norm(scfq, torch, None, scfq.norm_opts(k=K, canonical=True, target=TARGET, min_depth=MIN_DEPTH), buf, out, args.reps)
    print("two pass", json.dumps(result["two_pass"]), flush=True)
    # S2 / S4: fq-screen with the genome as its reference; every read matches, so keep_matched writes every record
    with scfq.screen_index_host([("genome", fasta)], K) as index:
        sopts = scfq.screen_opts(keep_matched=True)
        s2, s4, calls = [], [], []
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            ss = scfq.screen_device(index, buf.data_ptr(), n, opts=sopts, out1=(out.data_ptr(), out.numel()))
            if rep:
                calls.append((time.perf_counter() - t0) * 1e3)
                st = scfq.screen_stages()
                s2.append(st[1]), s4.append(st[3])
        result["screen"] = {"call_ms": stats(calls), "s2_lookup_ms": stats(s2), "s4_write_ms": stats(s4), "kmers": ss.kmers, "hit_kmers": ss.hit_kmers,
                            "out1_bytes": ss.out1_bytes, "index_slots": index.summary.slots, "index_distinct": index.summary.distinct,
                            "s4_written_GBps": ss.out1_bytes / (min(s4) * 1e-3) / 1e9 if min(s4) > 0 else 0.0}
    print("screen", json.dumps(result["screen"]), flush=True)
    n1 = result["given_table"]["n1_depth_ms"]["best"]
    result["n1_over_h1"] = n1 / min(h1) if min(h1) > 0 else None
    result["n1_over_s2"] = n1 / min(s2) if min(s2) > 0 else None
    # the child: the same input (the same seed on the same device), every read on the path through device memory
    del out
    torch.cuda.empty_cache()
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--only-n1", "--genome", str(args.genome), "--reads", str(args.reads), "--reps",
                            str(args.reps)], env=dict(os.environ, SCFQ_NORM_LDS_WINDOWS="64"), capture_output=True, text=True, timeout=300)
    if child.returncode == 0:
        result["lds_windows_64"] = json.loads(child.stdout.strip().splitlines()[-1])
        result["lds_windows_64"]["same_result"] = (result["lds_windows_64"]["units_out"] == result["given_table"]["units_out"])
        result["n1_lds64_over_n1"] = result["lds_windows_64"]["n1_depth_ms"]["best"] / n1 if n1 > 0 else None
    else:
        result["lds_windows_64"] = {"returncode": child.returncode, "error": (child.stdout + child.stderr)[-2000:]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)
    scfq.lib().scfq_shutdown()


if __name__ == "__main__":
    main()

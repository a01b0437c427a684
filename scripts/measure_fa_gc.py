#!/usr/bin/env python3
"""fa-gc on a device-resident synthetic FASTA (3 GB, 60 columns, 25 contigs), in ONE process: the stages of the index call (F1 tile
scan, F2 record scan, F3 contig table: HIP events), the whole index call, on the same bytes scfq_count_buffer (the yardstick: the
scan kernel of fq-count), and scfq_fa_count_intervals for 10^4, 10^6 and 10^7 cells at windows 50, 3 200 and 500 000.  Next to
it one host core doing what the reference does per cell (a recount of the 2 w + 1 bases with numpy, 10^3 cells, scaled linearly
and labelled so).  Writes profiles/fa_gc/measure.json (--out).

Run it under a time limit of its own:  timeout -k 10 600 python scripts/measure_fa_gc.py
"""
import argparse
import json
import os
import sys
import time

os.environ["SCFQ_FA_TIMING"] = "1"          # the library brackets its stages with HIP events (read before its first call)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "seq-collection_amd", "pyhost"))

HBM_PEAK_GBPS = 8000.0
WIDTH = 60


def best(fn, reps):
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t) * 1e3)
    return min(out), sorted(out)[len(out) // 2], r


def synth(torch, total, contigs):
    """`contigs` contigs of equal length, WIDTH columns, A C G T uniform; returns (buffer, bytes, [(name, length)])"""
    lines = total // contigs // (WIDTH + 1)
    headers = [b">chr%d synthetic\n" % (k + 1) for k in range(contigs)]
    n = sum(map(len, headers)) + contigs * lines * (WIDTH + 1)
    buf = torch.empty(n + 4096, dtype=torch.uint8, device="cuda:0")
    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda:0")
    at = 0
    for h in headers:
        buf[at:at + len(h)] = torch.tensor(list(h), dtype=torch.uint8, device="cuda:0")
        at += len(h)
        body = buf[at:at + lines * (WIDTH + 1)].view(lines, WIDTH + 1)
        body[:, :WIDTH] = letters[torch.randint(0, 4, (lines, WIDTH), device="cuda:0")]
        body[:, WIDTH] = 10
        at += lines * (WIDTH + 1)
    torch.cuda.synchronize()
    return buf, n, [("chr%d" % (k + 1), lines * WIDTH) for k in range(contigs)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=3_000_000_000)
    ap.add_argument("--contigs", type=int, default=25)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fa_gc", "measure.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import scfq

    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    buf, n, table = synth(torch, args.bytes, args.contigs)
    ptr = buf.data_ptr()
    scfq.set_wait_stream(torch.cuda.current_stream().cuda_stream)
    result = {"device": torch.cuda.get_device_name(0), "input_bytes": n, "contigs": args.contigs, "columns": WIDTH, "reps": args.reps,
              "hbm_peak_GBps": HBM_PEAK_GBPS,
              "timing": "ms; whole calls: host clock around the synchronous call, best and median of reps after one warm-up; "
                        "f1 / f2 / f3: HIP events inside the index call, best of reps"}
    stages = []

    def index():
        ix = scfq.fa_index_device(ptr, n)
        stages.append(scfq.fa_stages())
        return ix

    index().close()                                     # warm-up: pool growth, first launches
    stages.clear()
    keep = []
    ix_best, ix_med, ix = best(lambda: keep.append(index()) or keep[-1], args.reps)
    for other in keep[:-1]:
        other.close()
    assert [(c[0], c[2]) for c in ix.contigs] == table and ix.summary.bases == sum(t[1] for t in table) == ix.summary.acgt_bases
    st = [min(x[k] for x in stages) for k in range(3)]
    scfq.count_device(ptr, n)
    c_best, c_med, c = best(lambda: scfq.count_device(ptr, n), args.reps)
    scfq.count_device(ptr, n, flags=scfq.SCFQ_TIMING)
    yard_ms = scfq.last_timing().scan_kernel_ms
    gbps = lambda ms: n / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
    result["index"] = {"f1_tile_scan_ms": st[0], "f2_resolve_ms": st[1], "f3_contigs_ms": st[2], "f1_GBps": gbps(st[0]),
                       "f2_GBps_of_input": gbps(st[1]), "f3_GBps_of_input": gbps(st[2]), "f1_fraction_of_hbm_peak": gbps(st[0]) / HBM_PEAK_GBPS,
                       "index_call_ms": {"best": ix_best, "median": ix_med}, "index_call_GBps": gbps(ix_best), "tiles": ix.summary.tiles}
    result["yardstick_count_buffer"] = {"call_ms": {"best": c_best, "median": c_med}, "call_GBps": gbps(c_best),
                                        "scan_kernel_ms_last_call": yard_ms, "scan_kernel_GBps": gbps(yard_ms)}
    result["f1_over_yardstick_kernel"] = gbps(st[0]) / gbps(yard_ms) if yard_ms > 0 and st[0] > 0 else None
    result["f1_over_yardstick_call"] = gbps(st[0]) / gbps(c_best) if c_best > 0 and st[0] > 0 else None
    print("index", json.dumps(result["index"]), flush=True)
    print("yardstick", json.dumps(result["yardstick_count_buffer"]), flush=True)

    rng = np.random.default_rng(1)
    length = table[0][1]
    result["queries"] = {}
    for w in (50, 3200, 500000):
        for cells in (10 ** 4, 10 ** 6, 10 ** 7):
            contig = rng.integers(0, args.contigs, cells)
            pos0 = rng.integers(0, length, cells)
            q = np.column_stack([contig, np.maximum(0, pos0 - w), np.minimum(length, pos0 + w + 1)]).astype(np.uint64)
            scfq.fa_count_intervals(ix, q[:1000])
            q_best, q_med, out = best(lambda: scfq.fa_count_intervals(ix, q), 3 if cells >= 10 ** 7 else args.reps)
            assert (out[:, 2] == q[:, 2] - q[:, 1]).all() and (out[:, 1] == out[:, 2]).all()
            result["queries"]["w%d_cells%d" % (w, cells)] = {"call_ms": {"best": q_best, "median": q_med}, "ns_per_cell": q_best * 1e6 / cells}
            print(w, cells, json.dumps(result["queries"]["w%d_cells%d" % (w, cells)]), flush=True)

    # one host core, the reference's way: the bases of a chromosome in memory, 2 w + 1 of them recounted per cell
    first = buf[len(b">chr1 synthetic\n"):len(b">chr1 synthetic\n") + length // WIDTH * (WIDTH + 1)].cpu().numpy()
    chrom = first[first != 10]
    gc_table = np.zeros(256, dtype=bool)
    gc_table[list(b"GCgc")] = True
    acgt_table = np.zeros(256, dtype=bool)
    acgt_table[list(b"ACGTacgt")] = True
    result["host_recount_one_core"] = {"what": "numpy recount of the 2 w + 1 bases of every cell on one host core, 1000 cells measured, "
                                               "scaled linearly to the cell counts above (not the reference binary)"}
    for w in (50, 3200, 500000):
        pos0 = rng.integers(0, length, 1000)
        t = time.perf_counter()
        for p in pos0:
            s = chrom[max(0, p - w):p + w + 1]
            _ = int(gc_table[s].sum()) / max(1, int(acgt_table[s].sum()))
        ms = (time.perf_counter() - t) * 1e3
        result["host_recount_one_core"]["w%d" % w] = {"ms_per_1000_cells": ms, "scaled_ms_1e4": ms * 10, "scaled_ms_1e6": ms * 1e3, "scaled_ms_1e7": ms * 1e4}
    print("host", json.dumps(result["host_recount_one_core"]), flush=True)
    ix.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)
    scfq.lib().scfq_shutdown()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""How a launch of the scan kernel ends: residency (waves alive) against time, from the stamps build of the library (`make stamps`:
every wave of fq_scan_tiles and of fq_stream_null writes wall_clock64() at its start and before its partial's stores).

ONE launch of each kernel over the benchmark's device-resident Illumina buffer (10 GB by default), after a small warm-up launch.  For
each: the residency curve, the time from "residency first below 75 % / 50 % of its plateau" to the end of the launch, the bytes completed
per microsecond in that window against the plateau's rate, what the launch would have saved had the window run at the plateau's rate (as a
share of the launch), and the spread of wave lifetimes per segment of the geometry.  The stamps cost time: quote shares, never this
build's run time.

    make -C seq-collection_amd stamps
    SCFQ_TAPER_WAVES=0 python scripts/measure_scan_drain.py --label uniform
    python scripts/measure_scan_drain.py --label tapered

Results are merged into profiles/scan_taper/drain.json under the label."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--label", required=True)
ap.add_argument("--bytes", type=float, default=10e9)
ap.add_argument("--lib", default=os.path.join(ROOT, "seq-collection_amd", "ablate", "libsc_fqcount_hip_stamps.so"))
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_taper", "drain.json"))
args = ap.parse_args()
os.environ["SCFQ_LIB_OVERRIDE"] = args.lib
sys.path.insert(0, os.path.join(ROOT, "seq-collection_amd", "pyhost"))

import numpy as np
import torch
import scfq

TILE = 4096
L = scfq.lib()
if not hasattr(L, "scfq_debug_scan_stamps"):
    sys.exit("%s is not a stamps build (make -C seq-collection_amd stamps)" % args.lib)
L.scfq_debug_scan_stamps.restype = ctypes.c_int64
L.scfq_debug_scan_stamps.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
L.scfq_debug_wall_clock_khz.restype = ctypes.c_int64


def stamps():
    n = L.scfq_debug_scan_stamps(None, 0)
    assert n > 0, n
    a = np.zeros((n, 2), dtype=np.uint64)
    assert L.scfq_debug_scan_stamps(a.ctypes.data, n) == n
    return a


def range_tiles(g):
    """tiles of every range of the geometry, and the segment each belongs to"""
    segs = g.segments()
    tiles, seg_of = [], []
    for s, (first_range, first_tile, tpr) in enumerate(segs):
        end = segs[s + 1][1] if s + 1 < len(segs) else g.n_tiles
        k = -(-(end - first_tile) // tpr)
        t = np.full(k, tpr, dtype=np.int64)
        t[-1] = end - first_tile - (k - 1) * tpr
        tiles.append(t)
        seg_of.append(np.full(k, s))
    return np.concatenate(tiles), np.concatenate(seg_of)


def analyse(st, g, ticks_per_us):
    tiles, seg_of = range_tiles(g)
    assert st.shape[0] == tiles.size == g.n_ranges, (st.shape, tiles.size, g.n_ranges)
    t0 = st[:, 0].min()
    s = (st[:, 0] - t0).astype(np.float64) / ticks_per_us
    e = (st[:, 1] - t0).astype(np.float64) / ticks_per_us
    assert (e >= s).all()
    dur = float(e.max())
    ss, es = np.sort(s), np.sort(e)
    alive_at = lambda t: np.searchsorted(ss, t, side="right") - np.searchsorted(es, t, side="right")
    grid = np.arange(0.0, dur, 0.5)
    alive = alive_at(grid)
    mid = (grid >= 0.25 * dur) & (grid <= 0.75 * dur)
    plateau = float(np.median(alive[mid]))
    nbytes = tiles.astype(np.float64) * TILE
    life = np.maximum(e - s, 1e-3)

    def rate(a, b):      # bytes per microsecond completed in [a, b), a range's bytes spread evenly over its lifetime
        ov = np.clip(np.minimum(e, b) - np.maximum(s, a), 0.0, None)
        return float((nbytes * ov / life).sum() / (b - a))

    plateau_rate = rate(0.25 * dur, 0.75 * dur)
    out = {"ranges": int(g.n_ranges), "tiles_per_range": "/".join(str(x[2]) for x in g.segments()), "plateau_waves": plateau,
           "launch_us_in_this_build": round(dur, 1), "plateau_bytes_per_us": round(plateau_rate, 1), "below": {}}
    late = grid >= 0.5 * dur
    for pct in (75, 50, 25):
        idx = np.nonzero(late & (alive < plateau * pct / 100.0))[0]
        if idx.size == 0:
            continue
        t = float(grid[idx[0]])
        r = rate(t, dur)
        out["below"]["%d%%" % pct] = {
            "us_to_end": round(dur - t, 1), "share_of_launch": round((dur - t) / dur, 5),
            "bytes_per_us": round(r, 1), "rate_over_plateau": round(r / plateau_rate, 4),
            "loss_share_of_launch": round((dur - t) * (1.0 - r / plateau_rate) / dur, 5)}
    # the ramp at the other end, for comparison: time until the residency first reaches 75 % of the plateau
    idx = np.nonzero(alive >= 0.75 * plateau)[0]
    out["ramp_us_to_75%"] = round(float(grid[idx[0]]), 1) if idx.size else None
    out["whole_launch_rate_over_plateau"] = round(float(nbytes.sum() / dur / plateau_rate), 4)
    out["lifetimes_us"] = {}
    for k, seg in enumerate(g.segments()):
        m = (seg_of == k) & (tiles == seg[2])
        if m.any():
            q = np.percentile(e[m] - s[m], [0, 5, 50, 95, 100])
            out["lifetimes_us"]["tpr %d" % seg[2]] = {"ranges": int(m.sum()), "min": round(q[0], 1), "p5": round(q[1], 1), "median": round(q[2], 1),
                                                     "p95": round(q[3], 1), "max": round(q[4], 1)}
    step = max(1, grid.size // 300)
    tail = grid >= dur - 400.0
    out["residency"] = {"us": [round(float(x), 1) for x in grid[::step]], "waves": [int(x) for x in alive[::step]]}
    out["residency_last_400us"] = {"us_before_end": [round(dur - float(x), 1) for x in grid[tail][::10]], "waves": [int(x) for x in alive[tail][::10]]}
    return out


torch.cuda.set_device(0)
ticks_per_us = L.scfq_debug_wall_clock_khz() / 1000.0
assert ticks_per_us > 0
plan = scfq.synth_plan(0, 20260101, int(args.bytes))
buf = torch.empty(plan.bytes + 8192, dtype=torch.uint8, device="cuda:0")
ptr = (buf.data_ptr() + 4095) // 4096 * 4096
info = scfq.synth_device(0, 20260101, plan.records, ptr, plan.bytes)
torch.cuda.synchronize()
scfq.count_device(ptr, 64 << 20)      # warm-up: code objects, buffers
res = {"bytes": int(plan.bytes), "wall_clock_ticks_per_us": ticks_per_us,
       "note": "stamps build: shares and ratios are the result, run times are not those of the product"}
c = scfq.count_device(ptr, plan.bytes)
assert (c.reads, c.gc_bases, c.n_bases, c.bases) == (info.records, info.gc_bases, info.n_bases, info.bases)
g = scfq.debug_scan_geometry(plan.bytes, 0, 0, torch.cuda.get_device_properties(0).multi_processor_count)
res["kernel"] = scfq.debug_last_scan_kernel()
res["fq_scan_tiles"] = analyse(stamps(), g, ticks_per_us)
whole = plan.bytes // TILE * TILE
assert scfq.debug_stream_ms(ptr, whole, 1) > 0
g = scfq.debug_scan_geometry(whole, 0, 0, torch.cuda.get_device_properties(0).multi_processor_count)
res["fq_stream_null"] = analyse(stamps(), g, ticks_per_us)

os.makedirs(os.path.dirname(args.out), exist_ok=True)
doc = {}
if os.path.exists(args.out):
    with open(args.out) as f:
        doc = json.load(f)
doc[args.label] = res
with open(args.out, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
for k in ("fq_scan_tiles", "fq_stream_null"):
    print(args.label, k, res[k]["tiles_per_range"], "plateau", res[k]["plateau_waves"], json.dumps(res[k]["below"]))

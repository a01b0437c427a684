// fq_scan_geometry.hpp — which tiles belong to which range of a K1 launch.  One small value type, built on the host (pure C++, no HIP
// in it), passed to the kernels by value, read there with a handful of scalar compares.
//
// A launch is cut into at most kMaxScanSegments SEGMENTS of equal-sized ranges: range r of segment s covers the tiles
//     first_tile[s] + (r - first_range[s]) * tpr[s]   up to   + tpr[s],   clipped to first_tile[s + 1].
// Ranges are dispatched in index order, one wave each.  A uniform launch (one segment) ends with its waves' finish times spread over a
// good part of one wave lifetime, and while the residency falls through that spread the read stream runs below its rate.  The TAPERED
// geometry keeps the head of the input in ranges of the base size and halves the range size from segment to segment over the last
// quarter of a slot-fill, so the waves that are dispatched last are the short ones and the launch drains within one SHORT wave lifetime —
// without paying the per-range costs (an unhidden first load, the wave reductions and the partial's stores, a longer fold) over the
// whole input.  The histogram forms (4 KiB of partial per range, or 8 ranges tied to one workgroup) stay uniform: one segment through
// the same code path.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SCFQ_GEO_HD __host__ __device__ __forceinline__
#else
#define SCFQ_GEO_HD inline
#endif

namespace scfq {

constexpr int kMaxScanSegments = 6;

// Where the taper starts, in per cent of one slot-fill (resident_waves x base_tpr tiles) left to scan, and the smallest range size it
// goes down to.  Chosen from the A/B runs in profiles/scan_taper/ab.json (start 25 / 31 / 50 / 62 / 75 / 100 / 125 / 188 / 250 % of a
// fill of 4 096 waves, floor 6 / 12 / 25 tiles, at 640 MiB, 10 GB and 25 GB): the gain is flat from 25 to 60 % and gone at 250 %, where
// the fold of the extra ranges has eaten it; a floor of 25 tiles gives a third of it away, one of 6 adds ranges for nothing.
// Constants, not knobs.
constexpr uint32_t kTaperStartPercent = 25;
constexpr uint32_t kTaperFloorTiles = 12;

struct ScanGeometry {
  uint32_t n_segments;
  uint32_t first_range[kMaxScanSegments + 1];   // [n_segments] = n_ranges; so are the entries of unused segments
  uint32_t first_tile[kMaxScanSegments + 1];    // [n_segments] = n_tiles; so are the entries of unused segments
  uint32_t tpr[kMaxScanSegments];               // unused segments: 1
  SCFQ_GEO_HD uint32_t n_ranges() const { return first_range[kMaxScanSegments]; }
  SCFQ_GEO_HD uint32_t n_tiles() const { return first_tile[kMaxScanSegments]; }
};

// The tiles [t_begin, t_end) of `range` (< n_ranges).  Everything here is wave-uniform when `range` is: scalar compares and selects.
SCFQ_GEO_HD void scan_range_tiles(const ScanGeometry& g, uint32_t range, uint32_t& t_begin, uint32_t& t_end) {
  uint32_t fr = 0, ft = 0, tp = g.tpr[0], end = g.first_tile[1];
#pragma unroll
  for (int s = 1; s < kMaxScanSegments; ++s) {
    const bool in = range >= g.first_range[s];
    fr = in ? g.first_range[s] : fr;
    ft = in ? g.first_tile[s] : ft;
    tp = in ? g.tpr[s] : tp;
    end = in ? g.first_tile[s + 1] : end;
  }
  t_begin = ft + (range - fr) * tp;
  t_end = (end - t_begin > tp) ? t_begin + tp : end;
}

// resident_waves: waves the device holds at once (one slot-fill); 0 = no taper.  n_tiles < 2^32, 1 <= base_tpr.
inline ScanGeometry make_scan_geometry(uint64_t n_tiles, uint32_t base_tpr, uint32_t resident_waves) {
  ScanGeometry g{};
  uint32_t n = 0;
  uint64_t tile = 0, range = 0;
  auto push = [&](uint64_t tiles, uint32_t tpr) {   // one segment of `tiles` tiles in ranges of `tpr`
    g.first_range[n] = (uint32_t)range;
    g.first_tile[n] = (uint32_t)tile;
    g.tpr[n] = tpr;
    tile += tiles;
    range += (tiles + tpr - 1) / tpr;
    ++n;
  };
  // the taper always has room for two halvings below the base size
  const uint32_t floor_tpr = base_tpr / 4 < kTaperFloorTiles ? base_tpr / 4 : kTaperFloorTiles;
  const uint64_t fill = (uint64_t)resident_waves * base_tpr;
  const uint64_t tail = fill * kTaperStartPercent / 100;
  // (an input that is resident all at once has no drain to shorten: its largest range decides)
  if (resident_waves == 0 || floor_tpr == 0 || n_tiles <= fill || tail < base_tpr) {
    push(n_tiles, base_tpr);
  } else {
    uint64_t left = n_tiles;
    uint64_t head = (left > tail ? left - tail : left / 2) / base_tpr * base_tpr;   // whole ranges only, at least one (n_tiles > fill)
    if (head == 0) head = base_tpr;
    push(head, base_tpr);
    left -= head;
    uint32_t tpr = base_tpr;
    while (left) {
      tpr = tpr / 2 > floor_tpr ? tpr / 2 : floor_tpr;
      const uint64_t half = left / 2 / tpr * tpr;
      if (tpr == floor_tpr || n == kMaxScanSegments - 1 || half == 0) { push(left, tpr); break; }
      push(half, tpr);
      left -= half;
    }
  }
  g.n_segments = n;
  for (uint32_t s = n; s <= (uint32_t)kMaxScanSegments; ++s) {
    g.first_range[s] = (uint32_t)range;
    g.first_tile[s] = (uint32_t)tile;
    if (s < (uint32_t)kMaxScanSegments) g.tpr[s] = 1;
  }
  return g;
}

}  // namespace scfq

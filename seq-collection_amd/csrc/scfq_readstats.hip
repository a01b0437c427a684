// scfq_readstats.hip — `sc fq-readstats` on the MI355X (gfx950): per-read length, G+C, N and quality, and their summary
// (min / max / N50 / N90, length, GC and mean-quality histograms).  Not in the reference; definitions in include/sc_fqcount.h.
//
// The whole (inflated) input sits in HBM, as for fq-dedup:
//   K5  line index            (scfq_scratch::build_line_index: line_off[0 .. lines], and whether the input holds "\r\n" at all)
//   R0  rs_borders            a thread per tile: first[t] = the first line that starts at or after the tile's first byte, and the one
//                             table entry that tile shares with the tile before it is zeroed
//   R1  rs_reduce             the segmented reduction, partitioned by BYTES: a block per 32 KiB tile.  Its stretch of line_off goes to
//                             LDS, every lane takes 16 bytes at a time (one coalesced 16-byte load), finds its line by binary search in
//                             LDS and reduces the chunk line segment by line segment: G|C and N by SWAR compares, the quality bytes by
//                             v_sad_u8, under a byte mask — no per-byte branch.  A lane keeps the sums of its current line in registers and
//                             adds them to the record's LDS slot when the line changes; a wave whose lanes all end in one line (inside a
//                             long read) adds once.  A record that lies inside the tile is STORED (five words); a record that crosses a
//                             tile border gets atomicAdds from every tile it touches, into the entry R0 zeroed, and its two lengths from
//                             the tile its first byte lies in.
//                             A tile with more than kRsLineCap lines (lines shorter than 16 bytes on average) has no LDS stretch: it searches
//                             line_off in global memory and adds to the table directly; R0 zeroed every entry such a tile touches.
//   R2  rs_summarise          one pass over the table: sums, min / max and the three histograms per block in LDS, flushed with global atomics;
//       N50 / N90             exact: the lengths sorted in descending order over the bits max_len needs (rocprim), scanned, searched —
//                             or in closed form when every read has the same length
// Everything is integer / byte work; there is no CPU fallback.
#include "../../include/sc_fqcount.h"
#include "../../include/sc_fqcount_debug.h"

#include <cstring>        // (rocprim's texture iterator calls memset from host code)
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "scfq_record_device.hpp"
#include "scfq_scratch.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>

namespace {

thread_local char g_rerr[scfq_scratch::kErrBytes] = "";
thread_local double g_stage_ms[4] = {0, 0, 0, 0};

using scfq_scratch::DevBuf;

constexpr uint32_t kRsTile = 32768;        // bytes of input a block of R1 owns
constexpr uint32_t kRsThreads = 256;
constexpr uint32_t kRsSteps = kRsTile / (16 * kRsThreads);
constexpr uint32_t kRsLineCap = 2048;      // lines of a tile whose offsets go to LDS
constexpr uint32_t kRsSlots = kRsLineCap / 4 + 2;
constexpr uint32_t kRelFar = 0x7ffffff0u;  // an offset beyond the tile, as stored in LDS

// first j in [0, lines] with line_off[j] >= x.  line_off[lines] >= n, so every x <= n has one.
__device__ __forceinline__ uint64_t first_line_at_or_after(const uint64_t* line_off, uint64_t lines, uint64_t x) {
  uint64_t a = 0, b = lines;                 // answer in [a, b]
  while (a < b) {
    const uint64_t m = a + (b - a) / 2;
    if (line_off[m] >= x) b = m; else a = m + 1;
  }
  return a;
}

// tile t is the input's bytes [tile_lo(t), tile_lo(t + 1)): cut where the ADDRESS is a multiple of the tile, so that every 16-byte chunk is aligned
__device__ __forceinline__ uint64_t tile_lo(uint64_t t, uint32_t shift, uint64_t n) {
  const uint64_t a = t * kRsTile;
  return a <= shift ? 0 : std::min<uint64_t>(a - shift, n);
}

// text length of line k (0 for a line the input does not have)
__device__ __forceinline__ uint64_t line_text_len(const uint8_t* base, uint64_t n, const uint64_t* line_off, uint64_t lines, uint64_t k, bool has_cr) {
  if (k >= lines) return 0;
  uint64_t s, e;
  line_span(base, n, line_off, k, s, e, has_cr);
  return e - s;
}

struct TileLines {
  uint64_t ja, jb;            // the lines that START in the tile: [ja, jb)
  uint64_t j_first, j_last;   // the lines that have a byte (text or newline) in it
  bool dense;
};

__device__ __forceinline__ TileLines tile_lines(const uint64_t* line_off, uint64_t ja, uint64_t jb, uint64_t lo) {
  TileLines tl;
  tl.ja = ja;
  tl.jb = jb;
  tl.j_first = (line_off[ja] == lo) ? ja : ja - 1;      // (line_off[0] = 0 = tile 0's lo: ja - 1 only where ja >= 1)
  tl.j_last = (jb >= 1 && jb - 1 > tl.j_first) ? jb - 1 : tl.j_first;
  tl.dense = tl.j_last - tl.j_first + 1 > kRsLineCap;
  return tl;
}

__device__ __forceinline__ void zero_rec(scfq_read_rec* r) { r->seq_len = 0; r->gc_bases = 0; r->n_bases = 0; r->qual_len = 0; r->qual_sum = 0; }

// R0: a thread per tile (and one for the end of the input)
__global__ __launch_bounds__(256) void rs_borders(const uint64_t* line_off, uint64_t lines, uint64_t n, uint32_t shift, uint64_t n_tiles,
                                                 uint64_t* first, scfq_read_rec* rec) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (t > n_tiles) return;
  const uint64_t lo = t == n_tiles ? n : tile_lo(t, shift, n);
  const uint64_t ja = first_line_at_or_after(line_off, lines, lo);
  first[t] = ja;
  if (t == n_tiles) return;
  const uint64_t hi = t + 1 == n_tiles ? n : tile_lo(t + 1, shift, n);
  const uint64_t jb = first_line_at_or_after(line_off, lines, hi);
  const TileLines tl = tile_lines(line_off, ja, jb, lo);
  const uint64_t r_first = tl.j_first >> 2, r_last = tl.j_last >> 2;
  if (tl.dense) {
    for (uint64_t r = r_first; r <= r_last; ++r) zero_rec(&rec[r]);
  } else if (line_off[4 * r_first] < lo) {
    zero_rec(&rec[r_first]);           // the record this tile shares with the one before it
  }
}

__device__ __forceinline__ uint32_t byte_mask_below(int k) { return k <= 0 ? 0u : (k >= 4 ? 0xffffffffu : (1u << (8 * k)) - 1u); }
// 0x80 in every byte of x that is zero (exact: no carry crosses a byte)
__device__ __forceinline__ uint32_t zero_bytes(uint32_t x) { return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u; }

// R1
__global__ __launch_bounds__(kRsThreads) void rs_reduce(const uint8_t* base, uint64_t n, const uint64_t* line_off, uint64_t lines, uint32_t shift,
                                                       uint64_t n_tiles, const uint64_t* first, bool has_cr, scfq_read_rec* rec) {
  __shared__ uint32_t rel[kRsLineCap + 2];
  __shared__ uint32_t acc[3][kRsSlots];
  const uint64_t t = blockIdx.x;
  const int64_t t0 = (int64_t)(t * kRsTile) - (int64_t)shift;      // (negative for tile 0 of an unaligned input)
  const int64_t lo = (int64_t)tile_lo(t, shift, n), hi = t + 1 == n_tiles ? (int64_t)n : (int64_t)tile_lo(t + 1, shift, n);
  const TileLines tl = tile_lines(line_off, first[t], first[t + 1], (uint64_t)lo);
  const uint64_t j_first = tl.j_first, j_last = tl.j_last;
  const bool dense = tl.dense;
  const uint64_t r_first = j_first >> 2;
  const uint32_t n_slots = dense ? 0u : (uint32_t)((j_last >> 2) - r_first + 1);
  if (!dense) {
    const uint32_t entries = (uint32_t)(j_last - j_first + 2);       // line_off[j_first .. j_last + 1]; j_last + 1 <= lines
    for (uint32_t k = threadIdx.x; k < entries; k += kRsThreads) {
      const int64_t d = (int64_t)line_off[j_first + k] - lo;
      rel[k] = d < 0 ? 0u : (d > (int64_t)kRelFar ? kRelFar : (uint32_t)d);
    }
    for (uint32_t s = threadIdx.x; s < n_slots; s += kRsThreads) { acc[0][s] = 0; acc[1][s] = 0; acc[2][s] = 0; }
  }
  __syncthreads();
  auto off = [&](uint64_t k) -> int64_t { return dense ? (int64_t)line_off[k] : lo + (int64_t)rel[k - j_first]; };

  // the sums of the line this lane is in
  uint64_t cur_j = ~0ull;
  uint32_t a_gc = 0, a_n = 0, a_qs = 0;
  auto flush = [&]() {
    if (cur_j != ~0ull && (a_gc | a_n | a_qs)) {
      const uint64_t r = cur_j >> 2;
      if (dense) {
        if (a_gc) atomicAdd(reinterpret_cast<unsigned long long*>(&rec[r].gc_bases), (unsigned long long)a_gc);
        if (a_n) atomicAdd(reinterpret_cast<unsigned long long*>(&rec[r].n_bases), (unsigned long long)a_n);
        if (a_qs) atomicAdd(reinterpret_cast<unsigned long long*>(&rec[r].qual_sum), (unsigned long long)a_qs);
      } else {
        const uint32_t s = (uint32_t)(r - r_first);
        if (a_gc) atomicAdd(&acc[0][s], a_gc);
        if (a_n) atomicAdd(&acc[1][s], a_n);
        if (a_qs) atomicAdd(&acc[2][s], a_qs);
      }
    }
    a_gc = a_n = a_qs = 0;
  };

#pragma unroll 2
  for (uint32_t step = 0; step < kRsSteps; ++step) {
    const int64_t c0 = t0 + 16 * (int64_t)(step * kRsThreads + threadIdx.x);
    const int64_t v0 = c0 > lo ? c0 : lo, v1 = c0 + 16 < hi ? c0 + 16 : hi;
    if (v0 >= v1) continue;
    uint32_t w[4] = {0, 0, 0, 0};
    if (c0 >= 0 && c0 + 16 <= (int64_t)n) {
      const uint4 q = *reinterpret_cast<const uint4*>(base + c0);      // (base + c0 is 16-byte aligned: t0 = -shift mod 16)
      w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
    } else {
      // the input's first or last chunk: only its own bytes are read
      uint32_t x0 = 0, x1 = 0, x2 = 0, x3 = 0;
      for (int64_t p = v0; p < v1; ++p) {
        const uint32_t k = (uint32_t)(p - c0), b = (uint32_t)base[p] << (8 * (k & 3));
        if (k < 4) x0 |= b; else if (k < 8) x1 |= b; else if (k < 12) x2 |= b; else x3 |= b;
      }
      w[0] = x0; w[1] = x1; w[2] = x2; w[3] = x3;
    }
    // the line byte v0 lies in: the last k in [j_first, j_last] with off(k) <= v0
    uint64_t a = j_first, b = j_last + 1;
    while (b - a > 1) {
      const uint64_t m = a + (b - a) / 2;
      if (off(m) <= v0) a = m; else b = m;
    }
    uint64_t j = a;
    int64_t p = v0;
    for (;;) {
      const int64_t nl = off(j + 1) - 1;          // the line's (real or implied) '\n'
      int64_t te = nl < v1 ? nl : v1;             // end of its text inside this chunk
      if (has_cr && nl < (int64_t)n && nl - 1 >= p && nl - 1 < v1) {      // the byte before a real '\n' is in this chunk
        const uint32_t k = (uint32_t)(nl - 1 - c0);
        const uint32_t word = k < 4 ? w[0] : (k < 8 ? w[1] : (k < 12 ? w[2] : w[3]));
        if (((word >> (8 * (k & 3))) & 0xffu) == '\r') te = nl - 1;
      }
      if (te > p && (j & 1)) {                    // text of a sequence (4i + 1) or quality (4i + 3) line
        if (j != cur_j) { flush(); cur_j = j; }
        const int s = (int)(p - c0), e = (int)(te - c0);
        const bool seq = (j & 3) == 1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const uint32_t m = byte_mask_below(e - 4 * i) & ~byte_mask_below(s - 4 * i);
          if (seq) {
            // 'G' 0x47 and 'C' 0x43 differ in bit 2 only
            a_gc += (uint32_t)__builtin_popcount(zero_bytes((w[i] & ~0x04040404u) ^ 0x43434343u) & m);
            a_n += (uint32_t)__builtin_popcount(zero_bytes(w[i] ^ 0x4e4e4e4eu) & m);
          } else {
            a_qs = __builtin_amdgcn_sad_u8(w[i] & m, 0u, a_qs);
          }
        }
      }
      if (nl >= v1) break;
      p = nl + 1;
      ++j;
      if (p >= v1) break;
    }
  }
  // what the lanes still hold: one add per wave when they all sit in the same line (a tile inside a long read)
  {
    const uint64_t j0 = __builtin_amdgcn_readfirstlane((uint32_t)cur_j) | ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(cur_j >> 32)) << 32);
    const bool uniform = __builtin_amdgcn_ballot_w64(cur_j != j0) == 0 && j0 != ~0ull;
    if (uniform) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        a_gc += (uint32_t)__shfl_xor((int)a_gc, o, 64);
        a_n += (uint32_t)__shfl_xor((int)a_n, o, 64);
        a_qs += (uint32_t)__shfl_xor((int)a_qs, o, 64);
      }
      if ((threadIdx.x & 63) != 0) { a_gc = a_n = a_qs = 0; }
    }
    flush();
  }
  __syncthreads();
  if (dense) {
    // the lengths of the records whose first byte lies in this tile
    for (uint64_t r = (tl.ja + 3) / 4 + threadIdx.x; 4 * r < tl.jb; r += kRsThreads) {
      const uint64_t sl = line_text_len(base, n, line_off, lines, 4 * r + 1, has_cr), ql = line_text_len(base, n, line_off, lines, 4 * r + 3, has_cr);
      if (sl) atomicAdd(reinterpret_cast<unsigned long long*>(&rec[r].seq_len), (unsigned long long)sl);
      if (ql) atomicAdd(reinterpret_cast<unsigned long long*>(&rec[r].qual_len), (unsigned long long)ql);
    }
    return;
  }
  for (uint32_t s = threadIdx.x; s < n_slots; s += kRsThreads) {
    const uint64_t r = r_first + s;
    const uint32_t gc = acc[0][s], nb = acc[1][s], qs = acc[2][s];
    const uint64_t end_line = 4 * r + 4 < lines ? 4 * r + 4 : lines;
    const bool owner = (int64_t)line_off[4 * r] >= lo;                       // the record's first byte lies in this tile
    const bool inside = owner && ((int64_t)line_off[end_line] <= hi || t + 1 == n_tiles);
    uint64_t sl = 0, ql = 0;
    if (owner) { sl = line_text_len(base, n, line_off, lines, 4 * r + 1, has_cr); ql = line_text_len(base, n, line_off, lines, 4 * r + 3, has_cr); }
    if (inside) {
      rec[r].seq_len = sl; rec[r].gc_bases = gc; rec[r].n_bases = nb; rec[r].qual_len = ql; rec[r].qual_sum = qs;
    } else {
      if (sl) atomicAdd(reinterpret_cast<unsigned long long*>(&rec[r].seq_len), (unsigned long long)sl);
      if (gc) atomicAdd(reinterpret_cast<unsigned long long*>(&rec[r].gc_bases), (unsigned long long)gc);
      if (nb) atomicAdd(reinterpret_cast<unsigned long long*>(&rec[r].n_bases), (unsigned long long)nb);
      if (ql) atomicAdd(reinterpret_cast<unsigned long long*>(&rec[r].qual_len), (unsigned long long)ql);
      if (qs) atomicAdd(reinterpret_cast<unsigned long long*>(&rec[r].qual_sum), (unsigned long long)qs);
    }
  }
}

// ---- R2 ---------------------------------------------------------------------------------------------------------------------
// device image of the summary: [0] bases [1] gc [2] n [3] qual_bytes [4] qual_sum [5] min_len [6] max_len [7] no_qual, then the histograms
constexpr uint32_t kSumHead = 8;
constexpr uint32_t kHistWords = SCFQ_LEN_HIST_BINS + SCFQ_GC_HIST_BINS + SCFQ_MEANQ_HIST_BINS;
constexpr uint32_t kSumWords = kSumHead + kHistWords;

__device__ __forceinline__ uint64_t div_floor(uint64_t a, uint64_t b) {      // (b > 0) 64-bit division is a long routine on this device
  return ((a | b) >> 32) == 0 ? (uint64_t)((uint32_t)a / (uint32_t)b) : a / b;
}

__global__ __launch_bounds__(256) void rs_summarise(const scfq_read_rec* rec, uint64_t reads, unsigned long long* sum) {
  __shared__ uint32_t hist[kHistWords];
  for (uint32_t k = threadIdx.x; k < kHistWords; k += 256) hist[k] = 0;
  __syncthreads();
  uint64_t s_len = 0, s_gc = 0, s_n = 0, s_ql = 0, s_qs = 0, mn = ~0ull, mx = 0, noq = 0;
  const uint64_t rounds = (reads + (uint64_t)gridDim.x * 256 - 1) / ((uint64_t)gridDim.x * 256);      // (every lane makes every round: the ballot below)
  for (uint64_t it = 0; it < rounds; ++it) {
    const uint64_t i = (it * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
    const bool have = i < reads;
    uint64_t sl = 0, gc = 0, nb = 0, ql = 0, qs = 0;
    if (have) { const scfq_read_rec r = rec[i]; sl = r.seq_len; gc = r.gc_bases; nb = r.n_bases; ql = r.qual_len; qs = r.qual_sum; }
    const uint32_t lb = sl ? 64u - (uint32_t)__builtin_clzll(sl) : 0u;
    // reads of one length class, the usual case: one LDS add per wave instead of 64 on one address
    const uint32_t lb0 = __builtin_amdgcn_readfirstlane(lb);
    const uint64_t live = __builtin_amdgcn_ballot_w64(have);
    if (__builtin_amdgcn_ballot_w64(have && lb != lb0) == 0) {
      if ((threadIdx.x & 63) == 0 && live) atomicAdd(&hist[lb0], (uint32_t)__popcll(live));
    } else if (have) {
      atomicAdd(&hist[lb], 1u);
    }
    if (have) {
      s_len += sl; s_gc += gc; s_n += nb; s_ql += ql; s_qs += qs;
      mn = sl < mn ? sl : mn;
      mx = sl > mx ? sl : mx;
      const uint64_t den = sl - nb;
      atomicAdd(&hist[SCFQ_LEN_HIST_BINS + (den ? (uint32_t)div_floor(100 * gc, den) : 101u)], 1u);
      if (ql) atomicAdd(&hist[SCFQ_LEN_HIST_BINS + SCFQ_GC_HIST_BINS + (uint32_t)div_floor(qs, ql)], 1u); else ++noq;
    }
  }
  s_len = wave_sum(s_len); s_gc = wave_sum(s_gc); s_n = wave_sum(s_n); s_ql = wave_sum(s_ql); s_qs = wave_sum(s_qs); noq = wave_sum(noq);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t a = __shfl_xor((unsigned long long)mn, o, 64), b = __shfl_xor((unsigned long long)mx, o, 64);
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
  }
  if ((threadIdx.x & 63) == 0) {
    if (s_len) atomicAdd(&sum[0], (unsigned long long)s_len);
    if (s_gc) atomicAdd(&sum[1], (unsigned long long)s_gc);
    if (s_n) atomicAdd(&sum[2], (unsigned long long)s_n);
    if (s_ql) atomicAdd(&sum[3], (unsigned long long)s_ql);
    if (s_qs) atomicAdd(&sum[4], (unsigned long long)s_qs);
    atomicMin(&sum[5], (unsigned long long)mn);
    atomicMax(&sum[6], (unsigned long long)mx);
    if (noq) atomicAdd(&sum[7], (unsigned long long)noq);
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < kHistWords; k += 256)
    if (hist[k]) atomicAdd(&sum[kSumHead + k], (unsigned long long)hist[k]);
}

__global__ __launch_bounds__(256) void rs_lengths(const scfq_read_rec* rec, uint64_t reads, uint64_t* keys) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < reads) keys[i] = rec[i].seq_len;
}

// acc[i]: the sum of the i + 1 longest reads.  out: n50 l50 n90 l90 — the one position where acc * 100 >= bases * x first holds
__global__ __launch_bounds__(256) void rs_find_nx(const uint64_t* sorted, const uint64_t* acc, uint64_t reads, uint64_t bases, uint64_t* out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= reads) return;
  const uint64_t a = acc[i] * 100, before = i ? acc[i - 1] * 100 : 0;
  if (a >= bases * 50 && before < bases * 50) { out[0] = sorted[i]; out[1] = i + 1; }
  if (a >= bases * 90 && before < bases * 90) { out[2] = sorted[i]; out[3] = i + 1; }
}

// d_in: the whole input, resident; user_rec / cap: the caller's table or nullptr
int readstats_device(const uint8_t* d_in, uint64_t n, scfq_read_rec* user_rec, uint64_t cap, scfq_read_summary* out, hipStream_t stream) {
  for (double& m : g_stage_ms) m = 0;
  out->input_bytes = n;
  uint64_t lines = 0;
  DevBuf line_off, table, first, sum, keys, keys2, acc, tmp, nx;
  int rc = SCFQ_OK;
  bool has_cr = true;
  {
    const auto t_a = std::chrono::steady_clock::now();
    if ((rc = scfq_scratch::build_line_index(d_in, n, stream, g_rerr, line_off, &lines, &has_cr))) return rc;
    g_stage_ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_a).count();
  }
  const uint64_t reads = (lines + 3) / 4;
  out->lines = lines;
  out->reads = reads;
  if (reads >= (1ull << 31)) { std::snprintf(g_rerr, sizeof g_rerr, "more than 2^31 records in one input"); return SCFQ_EARG; }
  if (user_rec && cap < reads) { std::snprintf(g_rerr, sizeof g_rerr, "the record table holds %llu records, the input has %llu", (unsigned long long)cap, (unsigned long long)reads); return SCFQ_EARG; }
  if (reads == 0) return SCFQ_OK;
  scfq_read_rec* rec = user_rec;
  if (!rec) {
    if ((rc = table.alloc(reads * sizeof(scfq_read_rec), stream, g_rerr))) return rc;
    rec = table.as<scfq_read_rec>();
  }
  const uint32_t shift = (uint32_t)((uintptr_t)d_in & 15u);
  const uint64_t n_tiles = (n + shift + kRsTile - 1) / kRsTile;
  if (n_tiles >= (1ull << 31)) { std::snprintf(g_rerr, sizeof g_rerr, "input too large for one launch"); return SCFQ_EARG; }
  if ((rc = first.alloc((n_tiles + 1) * 8, stream, g_rerr)) || (rc = sum.alloc(kSumWords * 8, stream, g_rerr))) return rc;
  static const bool timing = scfq_scratch::env_switch("SCFQ_READSTATS_TIMING");
  scfq_scratch::StageClock clk(stream, timing);
  clk.mark(0);
  hipLaunchKernelGGL(rs_borders, dim3((unsigned)((n_tiles + 1 + 255) / 256)), dim3(256), 0, stream, line_off.as<uint64_t>(), lines, n, shift, n_tiles,
                     first.as<uint64_t>(), rec);
  SCFQ_SCRATCH_CHK(g_rerr, hipGetLastError());
  hipLaunchKernelGGL(rs_reduce, dim3((unsigned)n_tiles), dim3(kRsThreads), 0, stream, d_in, n, line_off.as<uint64_t>(), lines, shift, n_tiles,
                     first.as<uint64_t>(), has_cr, rec);
  SCFQ_SCRATCH_CHK(g_rerr, hipGetLastError());
  clk.mark(1);
  SCFQ_SCRATCH_CHK(g_rerr, hipMemsetAsync(sum.p, 0, kSumWords * 8, stream));
  SCFQ_SCRATCH_CHK(g_rerr, hipMemsetAsync(sum.as<uint64_t>() + 5, 0xff, 8, stream));      // min_len starts at all ones
  hipLaunchKernelGGL(rs_summarise, dim3((unsigned)std::min<uint64_t>((reads + 255) / 256, 2048)), dim3(256), 0, stream, rec, reads,
                     sum.as<unsigned long long>());
  SCFQ_SCRATCH_CHK(g_rerr, hipGetLastError());
  clk.mark(2);
  static thread_local uint64_t h[kSumWords];
  SCFQ_SCRATCH_CHK(g_rerr, hipMemcpyAsync(h, sum.p, kSumWords * 8, hipMemcpyDeviceToHost, stream));
  SCFQ_SCRATCH_CHK(g_rerr, hipStreamSynchronize(stream));
  out->bases = h[0]; out->gc_bases = h[1]; out->n_bases = h[2]; out->qual_bytes = h[3]; out->qual_sum = h[4];
  out->min_len = h[5]; out->max_len = h[6]; out->no_qual = h[7];
  std::memcpy(out->len_hist, h + kSumHead, SCFQ_LEN_HIST_BINS * 8);
  std::memcpy(out->gc_hist, h + kSumHead + SCFQ_LEN_HIST_BINS, SCFQ_GC_HIST_BINS * 8);
  std::memcpy(out->meanq_hist, h + kSumHead + SCFQ_LEN_HIST_BINS + SCFQ_GC_HIST_BINS, SCFQ_MEANQ_HIST_BINS * 8);
  if (out->bases != 0 && out->min_len == out->max_len) {
    // every read has the same length: the k longest hold k / reads of the bases, Lx = ceil(reads * x / 100)
    out->n50 = out->n90 = out->max_len;
    out->l50 = (reads * 50 + 99) / 100;
    out->l90 = (reads * 90 + 99) / 100;
  } else if (out->bases != 0) {
    if (out->bases >= (1ull << 57)) { std::snprintf(g_rerr, sizeof g_rerr, "more than 2^57 bases in one input"); return SCFQ_EARG; }
    const unsigned bits = 64u - (unsigned)__builtin_clzll(out->max_len);
    if ((rc = keys.alloc(reads * 8, stream, g_rerr)) || (rc = keys2.alloc(reads * 8, stream, g_rerr)) || (rc = acc.alloc(reads * 8, stream, g_rerr)) || (rc = nx.alloc(32, stream, g_rerr))) return rc;
    const unsigned blocks = (unsigned)((reads + 255) / 256);
    hipLaunchKernelGGL(rs_lengths, dim3(blocks), dim3(256), 0, stream, rec, reads, keys.as<uint64_t>());
    SCFQ_SCRATCH_CHK(g_rerr, hipGetLastError());
    size_t sort_bytes = 0, scan_bytes = 0;
    SCFQ_SCRATCH_CHK(g_rerr, rocprim::radix_sort_keys_desc(nullptr, sort_bytes, keys.as<uint64_t>(), keys2.as<uint64_t>(), (size_t)reads, 0u, bits, stream));
    SCFQ_SCRATCH_CHK(g_rerr, rocprim::inclusive_scan(nullptr, scan_bytes, keys2.as<uint64_t>(), acc.as<uint64_t>(), (size_t)reads, rocprim::plus<uint64_t>(), stream));
    if ((rc = tmp.alloc(std::max(sort_bytes, scan_bytes), stream, g_rerr))) return rc;
    SCFQ_SCRATCH_CHK(g_rerr, rocprim::radix_sort_keys_desc(tmp.p, sort_bytes, keys.as<uint64_t>(), keys2.as<uint64_t>(), (size_t)reads, 0u, bits, stream));
    SCFQ_SCRATCH_CHK(g_rerr, rocprim::inclusive_scan(tmp.p, scan_bytes, keys2.as<uint64_t>(), acc.as<uint64_t>(), (size_t)reads, rocprim::plus<uint64_t>(), stream));
    SCFQ_SCRATCH_CHK(g_rerr, hipMemsetAsync(nx.p, 0, 32, stream));
    hipLaunchKernelGGL(rs_find_nx, dim3(blocks), dim3(256), 0, stream, keys2.as<uint64_t>(), acc.as<uint64_t>(), reads, out->bases, nx.as<uint64_t>());
    SCFQ_SCRATCH_CHK(g_rerr, hipGetLastError());
    clk.mark(3);
    uint64_t r4[4] = {0, 0, 0, 0};
    SCFQ_SCRATCH_CHK(g_rerr, hipMemcpyAsync(r4, nx.p, 32, hipMemcpyDeviceToHost, stream));
    SCFQ_SCRATCH_CHK(g_rerr, hipStreamSynchronize(stream));
    out->n50 = r4[0]; out->l50 = r4[1]; out->n90 = r4[2]; out->l90 = r4[3];
  }
  g_stage_ms[1] = clk.between(0, 1);
  g_stage_ms[2] = clk.between(1, 2);
  g_stage_ms[3] = clk.between(2, 3);
  return SCFQ_OK;
}

}  // namespace

extern "C" {

const char* scfq_read_stats_error_detail(void) { return g_rerr; }

int scfq_debug_read_stats_stages(double* ms, uint32_t cap) { return scfq_scratch::copy_stage_ms(g_stage_ms, ms, cap); }

int scfq_read_stats_buffer(const void* ptr, uint64_t n, int is_device, scfq_read_rec* records_device, uint64_t cap, scfq_read_summary* out) {
  if (!out || out->struct_size != sizeof(scfq_read_summary) || (!ptr && n)) return SCFQ_EARG;
  scfq_scratch::clear_keep_size(out);
  g_rerr[0] = '\0';
  scfq_scratch::ResidentInput in;
  int rc = in.from_buffer(ptr, n, is_device != 0, is_device || records_device, g_rerr);
  if (rc) return rc;
  rc = readstats_device(in.d_in, n, records_device, cap, out, in.stream);
  if (rc == SCFQ_OK) in.mark_clean();      // (its last act was to wait for the stream)
  return rc;
}

int scfq_read_stats_file(const char* path, const scfq_opts* opts, scfq_read_summary* out) {
  if (!path || !out || out->struct_size != sizeof(scfq_read_summary)) return SCFQ_EARG;
  scfq_scratch::clear_keep_size(out);
  g_rerr[0] = '\0';
  scfq_scratch::ResidentInput in;
  int rc = in.from_file(path, opts, g_rerr);
  if (rc) return rc;
  rc = readstats_device(in.d_in, in.n, nullptr, 0, out, in.stream);
  if (rc == SCFQ_OK) in.mark_clean();      // (its last act was to wait for the stream)
  return rc;
}

}  // extern "C"

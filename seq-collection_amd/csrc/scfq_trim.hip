// scfq_trim.hip — `sc fq-trim` on the MI355X (gfx950): adapters, poly-G tails, bad quality and read-through cut off the 3' ends.
// Not in the reference; definitions in include/sc_fqcount.h.
//
// The input sits in HBM whole (one FASTQ, two, or one interleaved):
//   K5  line index            (scfq_scratch::build_line_index) of each input
//   P1  is_overlap            paired input only: d* of every pair into a table in pool memory (scfq_overlap.hpp: fq-insert-size's own
//                             code, compiled once, in scfq_insert.hip)
//   T1  tr_cut                the hot path: a wave per read, kTrWaves waves per block, the blocks stride over the reads.  The lanes load
//                             S[0, e) a byte each and turn it into P1's three bit planes (two code bits, and "is exactly the letter of
//                             its code"): three ballots per 64 bases, so a plane is at most 8 wave-uniform words.  Lane l owns the
//                             positions l, l + 64, ...: the 32-letter window at p is a funnel shift of each plane, a probe's mismatches
//                             are one population count under the mask of t = min(m, e - p) letters, and 100 mm <= pct t needs no
//                             division.  The probes (planes, lengths) are a kernel argument: scalar registers, a compile-time loop over
//                             the 8 slots.  The round (64 positions) in which a lane has a match ends the search: one wave_min of
//                             (p << 8 | j).  Poly-G is a count of leading ones of plane(G) below e, on wave-uniform words.  The window
//                             step is a wave prefix sum of q(i) with a carry between rounds: sum(p) = E[p + W] - E[p], the first bad
//                             p by a ballot.  Lane 0 stores 8 bytes per read: e after each of the four steps and the probe.
//   T2  tr_lengths            a thread per read (single-end) or pair: the bytes it adds to each output, summed per group of kTrGroup,
//                             and the statistics, one atomic per block and counter
//       exclusive scans       one per output over the groups (rocprim), each with a last entry that is the output's size
//   T3  tr_write              a wave per group.  Lanes 0 .. 31 look their read or pair up once, a prefix over the lengths inside the
//                             wave gives every record its place, then the records are written one after another by the whole wave: a
//                             record that is its own input bytes is one wave_copy, any other one its four pieces, each a wave_copy.
// T3 compares the two totals with the capacities before it stores anything: a result that does not fit leaves both outputs alone.
// T2 and T3 get a record's lengths from the same function (read_of).  Everything is integer / byte work; there is no CPU fallback.
#include "../../include/sc_fqcount.h"
#include "../../include/sc_fqcount_debug.h"

#include <cstring>        // (rocprim's texture iterator calls memset from host code)
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "scfq_reads_host.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

namespace {

thread_local char g_terr[scfq_scratch::kErrBytes] = "";
thread_local double g_stage_ms[4] = {0, 0, 0, 0};

using scfq_reads::Dest;
using scfq_reads::DevBuf;
using scfq_reads::finish;
using scfq_reads::Mode;

constexpr uint32_t kTrWaves = 4;                         // reads a block of T1 works on at a time; groups of a block of T3
constexpr uint32_t kTrMaxBlocks = 4096;                  // of T1
constexpr uint32_t kTrWords = SCFQ_TRIM_MAX_LEN / 64;    // words of a plane
constexpr uint32_t kTrGroup = kRecGroup;                 // reads or pairs of a group: one wave of T3, one entry of the scans
static_assert(SCFQ_TRIM_MAX_LEN == 512 && SCFQ_TRIM_MAX_PROBES == 8 && SCFQ_ADAPTERS_MAX_LEN == 32, "a cut point is 10 bits, a window one 32-bit word");

// T1's word per read: e after the overlap, adapter, poly-G and quality step, 10 bits each (the last one is the cut point), the probe
constexpr uint64_t kCutTooLong = 1ull << 44;
__host__ __device__ __forceinline__ uint32_t cut_e(uint64_t c, uint32_t step) { return (uint32_t)(c >> (10 * step)) & 1023u; }
__host__ __device__ __forceinline__ uint32_t cut_probe(uint64_t c) { return (uint32_t)(c >> 40) & 15u; }

// the counters of T2
enum { kTooLong = 0, kShort, kDropped, kBasesIn, kBasesOut, kCutOverlap, kCutAdapter, kCutPolyG, kCutQuality, kBasesOverlap, kBasesAdapter, kBasesPolyG,
       kBasesQuality, kAdapterReads, kBasesDropped = kAdapterReads + SCFQ_TRIM_MAX_PROBES, kOverlapped, kCounters };

struct TrProbes {         // bit k of a plane: letter k of the probe (P1's code: bits 1 and 2 of the letter)
  uint32_t c0[SCFQ_TRIM_MAX_PROBES], c1[SCFQ_TRIM_MAX_PROBES], len[SCFQ_TRIM_MAX_PROBES];
  uint32_t n;
};

struct TrSteps { uint32_t min_adapter_overlap, adapter_pct, poly_g, window, window_quality, q0, min_length; };

// code (bit 0, bit 1) and valid bit of a byte: bits 1 and 2 of 'A' 'C' 'T' 'G' are 0 1 2 3 (is_overlap's classify)
__device__ __forceinline__ void classify(uint32_t b, bool& c0, bool& c1, bool& v) {
  const uint32_t h = (b >> 1) & 3u;
  v = ((0x47544341u >> (8 * h)) & 0xffu) == b;
  c0 = (h & 1u) != 0;
  c1 = (h & 2u) != 0;
}

__device__ __forceinline__ int wave_prefix(int v, uint32_t lane) {      // inclusive
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(v, d, 64);
    if (lane >= (uint32_t)d) v += up;
  }
  return v;
}

// the word lane w keeps, wave-uniform
__device__ __forceinline__ uint64_t word_of(uint64_t v, uint32_t w) {
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(v >> 32), (int)w) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)w);
}
// bits [64 w + lane, 64 w + lane + 32) of a plane whose word w lane w keeps: a funnel shift of words w and w + 1
__device__ __forceinline__ uint32_t window_at(uint64_t plane, uint32_t w, uint32_t lane) {
  const uint64_t lo = word_of(plane, w), hi = word_of(plane, w + 1);
  return (uint32_t)(lane ? (lo >> lane) | (hi << (64 - lane)) : lo);
}

// T1.  Read r is record r of `a` (single-end: paired = 0) or mate r & 1 of pair r >> 1: record p * stride of a, record p * stride + second
// of b.  recs: P1's table, or nullptr (no overlap step).  (Held to 64 VGPRs and 8 waves per SIMD with amdgpu_waves_per_eu the
// kernel took the same time as with the 118 VGPRs and 4 waves the compiler chooses, within 6 % either way: it is bound by instruction
// issue, not by waves in flight — profiles/trim/measure.json, t1_waves_per_eu_8.)
__global__ __launch_bounds__(64 * kTrWaves) void tr_cut(RecInput a, RecInput b, uint64_t stride, uint64_t second, uint32_t paired, uint64_t reads,
                                                       const scfq_overlap_rec* recs, TrProbes pr, TrSteps st, uint64_t* cuts) {
  const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // (no barrier and no LDS: the waves of a block go their own ways)
  for (uint64_t r0 = (uint64_t)blockIdx.x * kTrWaves; r0 < reads; r0 += (uint64_t)gridDim.x * kTrWaves) {
    const uint64_t r = r0 + wave;
    if (r >= reads) continue;
    const uint64_t p = paired ? r >> 1 : r;
    const bool mate2 = paired && (r & 1);
    const RecInput& in = mate2 ? b : a;
    const uint64_t i = paired ? p * stride + (mate2 ? second : 0) : r;
    uint64_t ss, se, qs, qe;
    text_span(in, 4 * i + 1, ss, se);
    if (se - ss > SCFQ_TRIM_MAX_LEN) {
      if (lane == 0) cuts[r] = kCutTooLong;
      continue;
    }
    text_span(in, 4 * i + 3, qs, qe);
    const int len = (int)(se - ss), lq = (int)std::min(qe - qs, se - ss);
    int e = len;
    // 1: the insert of a pair with an accepted offset ends both mates (such a pair has no too-long mate)
    if (recs) {
      const scfq_overlap_rec rec = recs[p];
      if (rec.overlap) {
        int lb = len;
        if (!mate2) {
          uint64_t s2, e2;
          text_span(b, 4 * (p * stride + second) + 1, s2, e2);
          lb = (int)(e2 - s2);
        }
        e = std::min(len, rec.offset + lb);               // (d* + Lb >= 1)
      }
    }
    const int e0 = e;
    // the planes of S[0, e0) and q(i): position 64 w + lane is this lane's, word w of a plane is kept by lane w (lane 8 and up: 0)
    uint64_t x0 = 0, x1 = 0, xv = 0;
    int qv[kTrWords];
#pragma unroll
    for (uint32_t w = 0; w < kTrWords; ++w) {
      qv[w] = 0;
      if (64 * (int)w < e0) {
        const int y = (int)(64 * w + lane);
        bool c0, c1, v;
        classify(y < e0 ? in.base[ss + (uint64_t)y] : 0u, c0, c1, v);
        const uint64_t b0 = __builtin_amdgcn_ballot_w64(c0), b1 = __builtin_amdgcn_ballot_w64(c1), bv = __builtin_amdgcn_ballot_w64(v);
        if (lane == w) { x0 = b0; x1 = b1; xv = bv; }
        if (st.window_quality && y < lq) qv[w] = (int)in.base[qs + (uint64_t)y] - (int)st.q0;
      }
    }
    // 2: the smallest p at which a probe matches, the lowest probe there
    uint32_t probe = 0;
    if (pr.n) {
#pragma unroll
      for (uint32_t w = 0; w < kTrWords; ++w) {
        if (64 * (int)w < e) {
          const int pos = (int)(64 * w + lane), left = e - pos;
          const uint32_t w0 = window_at(x0, w, lane), w1 = window_at(x1, w, lane), wv = window_at(xv, w, lane);
          uint32_t best = ~0u;
#pragma unroll
          for (uint32_t j = 0; j < SCFQ_TRIM_MAX_PROBES; ++j) {
            if (j < pr.n) {                                  // (kernel-uniform)
              const int t = std::min((int)pr.len[j], left);
              const uint32_t tc = (uint32_t)std::max(t, 0), mask = tc >= 32 ? ~0u : (1u << tc) - 1u;
              const uint32_t mm = (uint32_t)__builtin_popcount(((w0 ^ pr.c0[j]) | (w1 ^ pr.c1[j]) | ~wv) & mask);
              const bool hit = t >= (int)st.min_adapter_overlap && 100u * mm <= st.adapter_pct * tc;
              if (hit && best == ~0u) best = ((uint32_t)pos << 8) | j;
            }
          }
          if (__builtin_amdgcn_ballot_w64(best != ~0u)) {    // (wave-uniform) later rounds hold larger p only
            const uint32_t key = (uint32_t)wave_min((uint64_t)best);
            e = (int)(key >> 8);
            probe = key & 0xffu;
            break;
          }
        }
      }
    }
    const int e1 = e;
    // 3: the all-G suffix of S[0, e), from the top word down, on wave-uniform values
    if (st.poly_g && e > 0) {
      const uint64_t xg = x0 & x1 & xv;                      // 'G' is code 3
      int pos = e, g = 0;
      bool go = true;
#pragma unroll
      for (int w = (int)kTrWords - 1; w >= 0; --w) {
        if (go && pos > 64 * w) {
          const int nb = pos - 64 * w;                       // 1 .. 64 positions of this word lie below pos
          const uint64_t other = ~word_of(xg, (uint32_t)w) << (64 - nb);      // the highest position on top
          const int run = other ? __builtin_clzll(other) : nb;
          g += run;
          pos -= run;
          go = run == nb;
        }
      }
      if (g >= (int)st.poly_g) e -= g;
    }
    const int e2 = e;
    // 4: the first window below e whose sum is under the threshold.  E: the exclusive prefix sums of q, a round at a time
    const int win = (int)st.window;
    if (st.window_quality && e >= win) {
      const int limit = (int)(st.window_quality * st.window);
      int incl = wave_prefix(qv[0], lane);
      int e_cur = incl - qv[0], carry = __shfl(incl, 63, 64);
#pragma unroll
      for (uint32_t w = 0; w < kTrWords; ++w) {
        if (64 * (int)w + win <= e) {                        // (wave-uniform) the round's first window lies below e
          const int qn = w + 1 < kTrWords ? qv[w + 1] : 0;
          incl = wave_prefix(qn, lane);
          const int e_next = carry + incl - qn;
          carry += __shfl(incl, 63, 64);
          const int src = (int)((lane + (uint32_t)win) & 63u);
          const int same = __shfl(e_cur, src, 64), next = __shfl(e_next, src, 64);
          const int sum = ((int)lane + win < 64 ? same : next) - e_cur;
          const uint64_t bad = __builtin_amdgcn_ballot_w64((int)(64 * w + lane) + win <= e && sum < limit);
          if (bad) {
            e = (int)(64 * w) + __builtin_ctzll(bad);
            break;
          }
          e_cur = e_next;
        }
      }
    }
    if (lane == 0) cuts[r] = (uint64_t)e0 | ((uint64_t)e1 << 10) | ((uint64_t)e2 << 20) | ((uint64_t)e << 30) | ((uint64_t)probe << 40);
  }
}

// what a read adds to its output if it is kept and where its pieces lie.  T2 and T3 both get it from here, so the lengths the scans saw
// are the lengths T3 writes
enum : uint32_t { kPieces = 0, kCopy, kEcho };
struct TrRead {
  uint64_t len;                        // bytes of the output record
  uint64_t hs, ss, ps, qs;             // starts of the header, sequence, separator and quality texts
  uint32_t hl, e, pl, ql;              // their lengths in the output
  uint32_t kind;                       // kPieces: the four pieces; kCopy: len bytes from hs on; kEcho: a too-long read
};

__device__ __forceinline__ TrRead read_of(const RecInput& in, uint64_t i, uint64_t cut, uint64_t& seq_len) {
  TrRead r = {};
  uint64_t e;
  text_span(in, 4 * i + 1, r.ss, e);
  seq_len = e - r.ss;
  if (cut & kCutTooLong) {
    r.kind = kEcho;
    r.len = echo_len(in, i);
    return r;
  }
  r.e = cut_e(cut, 3);
  text_span(in, 4 * i, r.hs, e);
  r.hl = (uint32_t)(e - r.hs);                          // (a header of 4 GiB or more is not supported: the lengths are 32-bit)
  text_span(in, 4 * i + 2, r.ps, e);
  r.pl = (uint32_t)(e - r.ps);
  text_span(in, 4 * i + 3, r.qs, e);
  r.ql = (uint32_t)std::min<uint64_t>(e - r.qs, r.e);
  r.len = (uint64_t)r.hl + r.e + r.pl + r.ql + 4;
  // all four lines there, the last one with its newline, and nothing left out of any: the record's own bytes
  if (4 * i + 4 <= in.lines) {
    const uint64_t r1 = in.line_off[4 * i + 4];
    if (r1 <= in.n && r1 - in.line_off[4 * i] == r.len) r.kind = kCopy;
  }
  return r;
}

// a kept read's record, by the whole wave
__device__ __forceinline__ void write_read(const RecInput& in, uint64_t i, const TrRead& r, uint8_t* dst, uint32_t lane) {
  if (r.kind == kEcho) { echo_record(in, i, dst, r.len, lane); return; }
  if (r.kind == kCopy) { wave_copy(dst, in.base + r.hs, r.len, lane); return; }
  uint8_t* const s = dst + r.hl + 1;
  uint8_t* const p = s + r.e + 1;
  uint8_t* const q = p + r.pl + 1;
  wave_copy(dst, in.base + r.hs, r.hl, lane);
  wave_copy(s, in.base + r.ss, r.e, lane);
  wave_copy(p, in.base + r.ps, r.pl, lane);
  wave_copy(q, in.base + r.qs, r.ql, lane);
  if (lane == 0) dst[r.hl] = '\n';
  if (lane == 1) s[r.e] = '\n';
  if (lane == 2) p[r.pl] = '\n';
  if (lane == 3) q[r.ql] = '\n';
}

// a unit: a single-end read, or a pair.  What its reads add to the two outputs, and whether it is kept
struct TrUnit {
  TrRead m[2];
  uint64_t len1, len2;                 // bytes for out1 and out2 (0 for a dropped unit)
  uint64_t first;                      // of len1, mate 1's record (interleaved input: mate 2's follows it)
  uint64_t seq_len[2], cut[2];
  uint32_t mates;
  bool dropped;
};

__device__ __forceinline__ TrUnit look_up(const RecInput& a, const RecInput& b, uint64_t stride, uint64_t second, uint32_t paired, uint64_t u,
                                          const uint64_t* cuts, uint32_t min_length) {
  TrUnit t = {};
  t.mates = paired ? 2u : 1u;
  bool is_short = false;
#pragma unroll
  for (uint32_t k = 0; k < 2; ++k) {
    if (k < t.mates) {
      t.cut[k] = cuts[paired ? 2 * u + k : u];
      t.m[k] = read_of(k ? b : a, paired ? u * stride + (k ? second : 0) : u, t.cut[k], t.seq_len[k]);
      is_short = is_short || (!(t.cut[k] & kCutTooLong) && t.m[k].e < min_length);
    }
  }
  t.dropped = is_short;
  if (is_short) return t;
  t.first = t.m[0].len;
  t.len1 = t.first + (paired && second ? t.m[1].len : 0);
  t.len2 = paired && !second ? t.m[1].len : 0;
  return t;
}

// T2.  group_len: two arrays of n_groups + 1 entries, one after the other (the last entry of each stays 0: the scan's total)
__global__ __launch_bounds__(256) void tr_lengths(RecInput a, RecInput b, uint64_t stride, uint64_t second, uint32_t paired, uint64_t units, const uint64_t* cuts,
                                                 const scfq_overlap_rec* recs, uint32_t min_length, uint64_t n_groups, uint64_t* group_len,
                                                 unsigned long long* counters) {
  __shared__ uint64_t sum_sh[kCounters][4];
  const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint64_t len[2] = {0, 0}, c[kCounters];
#pragma unroll
  for (int k = 0; k < kCounters; ++k) c[k] = 0;
  if (u < units) {
    const TrUnit t = look_up(a, b, stride, second, paired, u, cuts, min_length);
    len[0] = t.len1; len[1] = t.len2;
    if (recs) c[kOverlapped] = recs[u].overlap != 0;
#pragma unroll
    for (uint32_t k = 0; k < 2; ++k) {
      if (k >= t.mates) continue;
      const uint64_t cut = t.cut[k], sl = t.seq_len[k];
      const bool too_long = (cut & kCutTooLong) != 0;
      const uint64_t e0 = too_long ? sl : cut_e(cut, 0), e1 = too_long ? sl : cut_e(cut, 1), e2 = too_long ? sl : cut_e(cut, 2),
                     e3 = too_long ? sl : cut_e(cut, 3);
      c[kTooLong] += too_long;
      c[kShort] += !too_long && e3 < min_length;
      c[kDropped] += t.dropped;
      c[kBasesIn] += sl;
      c[kBasesOut] += t.dropped ? 0 : e3;
      c[kBasesDropped] += t.dropped ? e3 : 0;
      c[kCutOverlap] += e0 < sl; c[kBasesOverlap] += sl - e0;
      c[kCutAdapter] += e1 < e0; c[kBasesAdapter] += e0 - e1;
      c[kCutPolyG] += e2 < e1;   c[kBasesPolyG] += e1 - e2;
      c[kCutQuality] += e3 < e2; c[kBasesQuality] += e2 - e3;
#pragma unroll
      for (uint32_t j = 0; j < SCFQ_TRIM_MAX_PROBES; ++j) c[kAdapterReads + j] += e1 < e0 && cut_probe(cut) == j;
    }
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) store_group_len(len[k], k, u, units, n_groups, group_len);
  // the statistics: ONE atomic per block and counter (dd_count_marks: an atomic per wave on one address costs more than the kernel)
#pragma unroll
  for (int k = 0; k < kCounters; ++k) {
    const uint64_t s = wave_sum(c[k]);
    if ((threadIdx.x & 63) == 0) sum_sh[k][threadIdx.x >> 6] = s;
  }
  __syncthreads();
  if (threadIdx.x < kCounters) {
    const uint64_t t = sum_sh[threadIdx.x][0] + sum_sh[threadIdx.x][1] + sum_sh[threadIdx.x][2] + sum_sh[threadIdx.x][3];
    if (t) atomicAdd(&counters[threadIdx.x], (unsigned long long)t);
  }
}

using ::bcast;      // (the overload below hides the shared ones otherwise)
__device__ __forceinline__ TrRead bcast(const TrRead& m, uint32_t from) {
  TrRead r;
  r.len = bcast(m.len, from);
  r.hs = bcast(m.hs, from); r.ss = bcast(m.ss, from); r.ps = bcast(m.ps, from); r.qs = bcast(m.qs, from);
  r.hl = bcast(m.hl, from); r.e = bcast(m.e, from); r.pl = bcast(m.pl, from); r.ql = bcast(m.ql, from);
  r.kind = bcast(m.kind, from);
  return r;
}

// T3.  group_off: the two scanned arrays of T2's layout
__global__ __launch_bounds__(64 * kTrWaves) void tr_write(RecInput a, RecInput b, uint64_t stride, uint64_t second, uint32_t paired, uint64_t units,
                                                         const uint64_t* cuts, uint32_t min_length, uint64_t n_groups, const uint64_t* group_off, RecOut o1,
                                                         RecOut o2) {
  const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // (when one result is more than its output holds, nothing is written to either)
  if (!(output_fits(o1, 0, n_groups, group_off) && output_fits(o2, 1, n_groups, group_off))) return;
  const uint64_t g = (uint64_t)blockIdx.x * kTrWaves + wave;
  if (g >= n_groups) return;
  const uint64_t u0 = g * kTrGroup;
  const uint32_t count = (uint32_t)std::min<uint64_t>(kTrGroup, units - u0);
  TrUnit mine = {};
  if (lane < count) mine = look_up(a, b, stride, second, paired, u0 + lane, cuts, min_length);
  const uint64_t len[2] = {mine.len1, mine.len2};
  uint64_t at[2];
  place_units(len, g, n_groups, group_off, lane, at);
  for (uint32_t q = 0; q < count; ++q) {
    const uint64_t l1 = bcast(mine.len1, q), l2 = bcast(mine.len2, q), first = bcast(mine.first, q), w1 = bcast(at[0], q), w2 = bcast(at[1], q);
    if (l1 + l2 == 0) continue;                            // (a dropped unit; a kept record has its four '\n' at the least, or is an echo of nothing)
    const uint64_t u = u0 + q;
    const uint64_t i1 = paired ? u * stride : u, i2 = u * stride + second;
    const TrRead m1 = bcast(mine.m[0], q);                 // (every lane takes part in the shuffles)
    if (o1.p && first) write_read(a, i1, m1, o1.p + w1, lane);
    if (paired) {
      const TrRead m2 = bcast(mine.m[1], q);
      if (second) { if (o1.p && m2.len) write_read(b, i2, m2, o1.p + w1 + first, lane); }
      else if (o2.p && m2.len) write_read(b, i2, m2, o2.p + w2, lane);
    }
  }
}

struct Params {
  scfq_overlap::Params ov;
  uint32_t flags;
  TrProbes probes;
  TrSteps steps;
};

bool args_ok(const scfq_trim_opts* opts, const scfq_trim_stats* st, Params& p) {
  if (!st || st->struct_size != sizeof(scfq_trim_stats)) return false;
  std::memset(&p, 0, sizeof p);
  p.ov.min_overlap = 30; p.ov.max_mm = 5; p.ov.max_pct = 20;
  p.steps = TrSteps{5, 10, 0, 4, 0, 33, 15};
  const char* seqs[SCFQ_TRIM_MAX_PROBES];
  uint32_t n = 0;
  if (opts) {
    if (opts->struct_size != sizeof(scfq_trim_opts)) return false;
    p.flags = opts->flags;
    p.ov.min_overlap = opts->min_overlap; p.ov.max_mm = opts->max_mismatches; p.ov.max_pct = opts->max_mismatch_pct;
    p.steps = TrSteps{opts->min_adapter_overlap, opts->adapter_mismatch_pct, opts->poly_g, opts->window, opts->window_quality, opts->phred_offset, opts->min_length};
    const uint32_t known = SCFQ_TRIM_INTERLEAVED | SCFQ_TRIM_NO_OVERLAP | SCFQ_TRIM_NO_ADAPTERS;
    if (p.flags & ~known) { std::snprintf(g_terr, sizeof g_terr, "unknown flag bits 0x%x", p.flags & ~known); return false; }
    if (!scfq_overlap::params_in_range(p.ov, g_terr)) return false;
    const TrSteps& s = p.steps;
    if (s.min_adapter_overlap < 1 || s.min_adapter_overlap > 32) { std::snprintf(g_terr, sizeof g_terr, "min_adapter_overlap %u is not in 1 .. 32", s.min_adapter_overlap); return false; }
    if (s.adapter_pct > 100) { std::snprintf(g_terr, sizeof g_terr, "adapter_mismatch_pct %u is not in 0 .. 100", s.adapter_pct); return false; }
    if (s.poly_g > SCFQ_TRIM_MAX_LEN) { std::snprintf(g_terr, sizeof g_terr, "poly_g %u is not in 0 .. %d", s.poly_g, SCFQ_TRIM_MAX_LEN); return false; }
    if (s.window < 1 || s.window > 32) { std::snprintf(g_terr, sizeof g_terr, "window %u is not in 1 .. 32", s.window); return false; }
    if (s.window_quality > 93) { std::snprintf(g_terr, sizeof g_terr, "window_quality %u is not in 0 .. 93", s.window_quality); return false; }
    if (s.min_length > SCFQ_TRIM_MAX_LEN) { std::snprintf(g_terr, sizeof g_terr, "min_length %u is not in 0 .. %d", s.min_length, SCFQ_TRIM_MAX_LEN); return false; }
    if (s.q0 != 33 && s.q0 != 64) { std::snprintf(g_terr, sizeof g_terr, "phred_offset %u is not 33 or 64", s.q0); return false; }
    if (opts->reserved[0] || opts->reserved[1]) { std::snprintf(g_terr, sizeof g_terr, "the reserved words are %u and %u, not 0", opts->reserved[0], opts->reserved[1]); return false; }
    if (opts->n_probes > SCFQ_TRIM_MAX_PROBES) { std::snprintf(g_terr, sizeof g_terr, "%u probes: 0 .. %u are allowed", opts->n_probes, (unsigned)SCFQ_TRIM_MAX_PROBES); return false; }
    if (opts->n_probes && (p.flags & SCFQ_TRIM_NO_ADAPTERS)) { std::snprintf(g_terr, sizeof g_terr, "%u probes together with SCFQ_TRIM_NO_ADAPTERS", opts->n_probes); return false; }
    for (; n < opts->n_probes; ++n) seqs[n] = opts->probes[n];
  }
  if (n == 0 && !(p.flags & SCFQ_TRIM_NO_ADAPTERS)) {      // the built-in set without its poly-A and poly-G entries
    const char *name = nullptr, *seq = nullptr;
    for (uint32_t i = 0; scfq_adapters_default(i, &name, &seq) > 0 && n < SCFQ_TRIM_MAX_PROBES; ++i)
      if (std::strncmp(name, "poly", 4) != 0) seqs[n++] = seq;
  }
  p.probes.n = n;
  for (uint32_t j = 0; j < n; ++j) {
    const char* s = seqs[j];
    if (!s || !*s) { std::snprintf(g_terr, sizeof g_terr, "probe %u is %s", j, s ? "empty" : "NULL"); return false; }
    uint32_t len = 0;
    for (; s[len]; ++len) {
      if (len >= SCFQ_ADAPTERS_MAX_LEN) { std::snprintf(g_terr, sizeof g_terr, "probe %u is longer than %u letters", j, (unsigned)SCFQ_ADAPTERS_MAX_LEN); return false; }
      const unsigned char b = (unsigned char)s[len];
      if (b != 'A' && b != 'C' && b != 'G' && b != 'T') {
        std::snprintf(g_terr, sizeof g_terr, "probe %u holds the byte 0x%02x at %u: only A C G T are allowed", j, (unsigned)b, len);
        return false;
      }
      p.probes.c0[j] |= ((b >> 1) & 1u) << len;
      p.probes.c1[j] |= ((b >> 2) & 1u) << len;
    }
    p.probes.len[j] = len;
  }
  return true;
}

int trim_device(const uint8_t* d1, uint64_t n1, const uint8_t* d2, uint64_t n2, Mode mode, const Params& prm, bool own_outputs, Dest dst[2], DevBuf own[2],
                bool check_caps, scfq_trim_stats* st, hipStream_t stream) {
  for (double& m : g_stage_ms) m = 0;
  const bool paired = mode != Mode::single, interleaved = mode == Mode::interleaved;
  const bool overlap = paired && !(prm.flags & SCFQ_TRIM_NO_OVERLAP);
  st->input_bytes1 = n1;
  st->input_bytes2 = n2;
  st->flags = prm.flags;
  st->min_overlap = prm.ov.min_overlap; st->max_mismatches = prm.ov.max_mm; st->max_mismatch_pct = prm.ov.max_pct;
  st->min_adapter_overlap = prm.steps.min_adapter_overlap; st->adapter_mismatch_pct = prm.steps.adapter_pct;
  st->poly_g = prm.steps.poly_g; st->window = prm.steps.window; st->window_quality = prm.steps.window_quality;
  st->min_length = prm.steps.min_length; st->phred_offset = prm.steps.q0; st->n_probes = prm.probes.n;
  scfq_overlap::Indexed ix;
  int rc = SCFQ_OK;
  double index_ms = 0;
  uint64_t units = 0, reads = 0;
  if ((rc = scfq_reads::index_units(d1, n1, d2, n2, mode, stream, g_terr, ix, &index_ms, st, &units, &reads))) return rc;
  st->reads_in = reads;
  if (units == 0) return SCFQ_OK;           // (two empty outputs: they fit into anything)
  const uint64_t n_groups = (units + kTrGroup - 1) / kTrGroup;
  DevBuf recs, acc, cuts, group_len, group_off, counters, tmp;
  scfq_reads::GroupScan gs(2, n_groups, group_len, group_off, stream, g_terr);
  if ((overlap && ((rc = recs.alloc(units * sizeof(scfq_overlap_rec), stream, g_terr)) || (rc = acc.alloc(scfq_overlap::kAccWords * 8, stream, g_terr)))) ||
      (rc = cuts.alloc(reads * 8, stream, g_terr)) || (rc = gs.alloc()) || (rc = counters.alloc(kCounters * 8, stream, g_terr)))
    return rc;
  size_t scan_bytes = 0;
  if ((rc = gs.scratch_bytes(&scan_bytes)) || (rc = tmp.alloc(scan_bytes, stream, g_terr))) return rc;
  static const bool timing = scfq_scratch::env_switch("SCFQ_TRIM_TIMING");
  scfq_scratch::StageClock clk(stream, timing);
  if (overlap) SCFQ_SCRATCH_CHK(g_terr, hipMemsetAsync(acc.p, 0, scfq_overlap::kAccWords * 8, stream));
  SCFQ_SCRATCH_CHK(g_terr, hipMemsetAsync(counters.p, 0, kCounters * 8, stream));
  if ((rc = gs.zero())) return rc;
  clk.mark(0);
  if (overlap && (rc = scfq_overlap::queue_overlap(d1, n1, d2, n2, interleaved, ix, prm.ov, recs.as<scfq_overlap_rec>(), acc.as<unsigned long long>(), stream, g_terr)))
    return rc;
  clk.mark(1);
  const RecInput a = {d1, n1, ix.off1.as<uint64_t>(), ix.lines1, ix.cr1};
  const RecInput b = mode == Mode::two ? RecInput{d2, n2, ix.off2.as<uint64_t>(), ix.lines2, ix.cr2} : a;
  const uint64_t stride = interleaved ? 2 : 1, second = interleaved ? 1 : 0;
  const scfq_overlap_rec* table = overlap ? recs.as<scfq_overlap_rec>() : nullptr;
  hipLaunchKernelGGL(tr_cut, dim3((unsigned)std::min<uint64_t>((reads + kTrWaves - 1) / kTrWaves, kTrMaxBlocks)), dim3(64 * kTrWaves), 0, stream, a, b, stride,
                     second, paired ? 1u : 0u, reads, table, prm.probes, prm.steps, cuts.as<uint64_t>());
  SCFQ_SCRATCH_CHK(g_terr, hipGetLastError());
  clk.mark(2);
  hipLaunchKernelGGL(tr_lengths, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, stream, a, b, stride, second, paired ? 1u : 0u, units, cuts.as<uint64_t>(),
                     table, prm.steps.min_length, n_groups, gs.len(), counters.as<unsigned long long>());
  SCFQ_SCRATCH_CHK(g_terr, hipGetLastError());
  if ((rc = gs.scan(tmp.p, scan_bytes))) return rc;
  clk.mark(3);
  // the sizes and the statistics come back first: pool memory for the outputs is taken to fit, and a caller's buffer that is too small
  // is known here
  uint64_t h[kCounters];
  if ((rc = gs.read_totals())) return rc;
  SCFQ_SCRATCH_CHK(g_terr, hipMemcpyAsync(h, counters.p, kCounters * 8, hipMemcpyDeviceToHost, stream));
  SCFQ_SCRATCH_CHK(g_terr, hipStreamSynchronize(stream));
  st->out1_bytes = gs.total[0]; st->out2_bytes = gs.total[1];
  st->too_long = h[kTooLong]; st->short_reads = h[kShort]; st->dropped_reads = h[kDropped]; st->reads_out = reads - h[kDropped];
  st->bases_in = h[kBasesIn]; st->bases_out = h[kBasesOut]; st->bases_dropped = h[kBasesDropped];
  st->cut_overlap = h[kCutOverlap]; st->cut_adapter = h[kCutAdapter]; st->cut_polyg = h[kCutPolyG]; st->cut_quality = h[kCutQuality];
  st->bases_overlap = h[kBasesOverlap]; st->bases_adapter = h[kBasesAdapter]; st->bases_polyg = h[kBasesPolyG]; st->bases_quality = h[kBasesQuality];
  for (uint32_t j = 0; j < SCFQ_TRIM_MAX_PROBES; ++j) st->adapter_reads[j] = h[kAdapterReads + j];
  st->overlapped_pairs = h[kOverlapped];
  const scfq_reads::Placement put = scfq_reads::place_outputs(gs, scfq_reads::kOutNames, dst, own_outputs, check_caps, false, own, stream, g_terr);
  if (put.rc) return put.rc;
  if (put.out[0].p || put.out[1].p) {
    hipLaunchKernelGGL(tr_write, dim3((unsigned)((n_groups + kTrWaves - 1) / kTrWaves)), dim3(64 * kTrWaves), 0, stream, a, b, stride, second, paired ? 1u : 0u,
                       units, cuts.as<uint64_t>(), prm.steps.min_length, n_groups, gs.off(), put.out[0], put.out[1]);
    SCFQ_SCRATCH_CHK(g_terr, hipGetLastError());
  }
  clk.mark(4);
  SCFQ_SCRATCH_CHK(g_terr, hipStreamSynchronize(stream));
  g_stage_ms[0] = clk.between(0, 1);
  g_stage_ms[1] = clk.between(1, 2);
  g_stage_ms[2] = clk.between(2, 3);
  g_stage_ms[3] = clk.between(3, 4);
  return put.verdict;      // (SCFQ_EARG for an output that is too small: place_outputs has left the text)
}

}  // namespace

extern "C" {

const char* scfq_trim_error_detail(void) { return g_terr; }

int scfq_debug_trim_stages(double* ms, uint32_t cap) { return scfq_scratch::copy_stage_ms(g_stage_ms, ms, cap); }

int scfq_trim_buffers(const void* r1, uint64_t n1, const void* r2, uint64_t n2, int is_device, const scfq_trim_opts* opts, void* out1, uint64_t cap1, void* out2,
                      uint64_t cap2, int out_is_device, scfq_trim_stats* stats) {
  g_terr[0] = '\0';
  Params prm;
  if (!args_ok(opts, stats, prm) || (!r1 && n1) || (!r2 && n2) || (!out1 && cap1) || (!out2 && cap2)) return SCFQ_EARG;
  const bool interleaved = (prm.flags & SCFQ_TRIM_INTERLEAVED) != 0;
  if (interleaved && (r2 || n2)) { std::snprintf(g_terr, sizeof g_terr, "interleaved input takes no second buffer"); return SCFQ_EARG; }
  const Mode mode = interleaved ? Mode::interleaved : (r2 ? Mode::two : Mode::single);
  if (mode != Mode::two && out2) { std::snprintf(g_terr, sizeof g_terr, "one input has no second output (out2)"); return SCFQ_EARG; }
  scfq_scratch::clear_keep_size(stats);
  Dest dst[2] = {{static_cast<uint8_t*>(out1), cap1, out1 != nullptr}, {static_cast<uint8_t*>(out2), cap2, out2 != nullptr}};
  const bool any_out = out1 || out2, direct = any_out && out_is_device;
  scfq_scratch::ResidentInput in1, in2;
  int rc = in1.from_buffer(r1, n1, is_device != 0, is_device || direct, g_terr);
  if (rc) return rc;
  // (a host buffer's copy is waited for inside; device memory of the caller is ordered before in1's stream above)
  if (mode == Mode::two && (rc = in2.from_buffer(r2, n2, is_device != 0, false, g_terr))) return rc;
  DevBuf own[2];
  rc = trim_device(in1.d_in, in1.n, in2.d_in, in2.n, mode, prm, /*own_outputs=*/!direct, dst, own, /*check_caps=*/true, stats, in1.stream);
  if (rc) return finish(in1, rc);
  if (!direct) {
    const uint64_t bytes[2] = {stats->out1_bytes, stats->out2_bytes};
    if ((rc = scfq_reads::outputs_to_host(2, dst, own, bytes, in1.stream, g_terr))) return rc;
    SCFQ_SCRATCH_CHK(g_terr, hipStreamSynchronize(in1.stream));
  }
  for (DevBuf& o : own) o.drop();
  in1.mark_clean();      // (the last act was to wait for the stream; behind it lie returns of pool memory only)
  return SCFQ_OK;
}

int scfq_trim_files(const char* path1, const char* path2, const scfq_opts* opts, const scfq_trim_opts* topts, int out1_fd, int out2_fd, scfq_trim_stats* stats) {
  g_terr[0] = '\0';
  Params prm;
  if (!path1 || !args_ok(topts, stats, prm)) return SCFQ_EARG;
  const bool interleaved = (prm.flags & SCFQ_TRIM_INTERLEAVED) != 0;
  if (interleaved && path2) { std::snprintf(g_terr, sizeof g_terr, "interleaved input takes no second file"); return SCFQ_EARG; }
  const Mode mode = interleaved ? Mode::interleaved : (path2 ? Mode::two : Mode::single);
  if (mode != Mode::two && out2_fd >= 0) { std::snprintf(g_terr, sizeof g_terr, "one input has no second output (out2)"); return SCFQ_EARG; }
  scfq_scratch::clear_keep_size(stats);
  scfq_scratch::ResidentInput in1, in2;
  int rc = in1.from_file(path1, opts, g_terr);
  if (rc) return rc;
  if (mode == Mode::two && (rc = in2.from_file(path2, opts, g_terr))) return rc;      // (staged when this returns)
  const int fd[2] = {out1_fd, out2_fd};
  Dest dst[2] = {{nullptr, 0, out1_fd >= 0}, {nullptr, 0, out2_fd >= 0}};
  DevBuf own[2];
  rc = trim_device(in1.d_in, in1.n, in2.d_in, in2.n, mode, prm, /*own_outputs=*/true, dst, own, /*check_caps=*/false, stats, in1.stream);
  if (rc) return finish(in1, rc);
  const uint64_t bytes[2] = {stats->out1_bytes, stats->out2_bytes};
  return scfq_reads::outputs_to_fds(2, own, bytes, fd, in1, g_terr);
}

}  // extern "C"

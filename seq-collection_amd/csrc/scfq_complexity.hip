// scfq_complexity.hip — `sc fq-complexity` on the MI355X (gfx950): symmetric DUST masking and filtering of low-complexity reads.
// Not in the reference; definitions in include/sc_fqcount.h.
//
// The input sits in HBM whole (one FASTQ, two, or one interleaved):
//   K5  line index            (scfq_scratch::build_line_index) of each input
//   D1  cx_score              the hot path: a wave per read, kCxWaves waves per block, the blocks stride over the reads.  Position
//                             64 w + lane is a lane's: it loads its three bases and stores the 6-bit triplet code, or 0xFF for a triplet
//                             that is not valid, into LDS, one byte each.  Then every position j gets its 64-bit word near(j) in LDS:
//                             bit d - 1 says t(j - d) == t(j), both valid, d = 1 .. window - 3 (byte reads, lane-consecutive).
//                             Starts are handled 64 at a time (a round), rounds from the LAST to the first; lane i owns start
//                             s = 64 w + i.  In step l = 2 .. window - 2 every lane adds triplet j = s + l - 1 to its interval:
//                             c += popcount(near(j) & (2^(l-1) - 1)) (one 8-byte LDS read, lane-consecutive), forms
//                             best(s, j) = max(c / (l-1), best(s, j-1), best(s+1, j)) — the last term is the neighbour lane's value of
//                             the step before, one __shfl_down; lane 63 takes it from the row that lane 0 of the round above left
//                             in LDS (two rows, by the round's parity) —, tests high && c / (l-1) >= both older terms, and keeps the
//                             furthest perfect end and the number of perfect intervals.  A fraction is one word, c << 6 | (l-1);
//                             two fractions are compared by two 24-bit multiplies; there is no division in the loop (one per lane
//                             and read behind it, for the score) and no floating point.  The furthest ends go to LDS; the mask
//                             plane is the union of [s, end + 2]: a prefix maximum over the wave with a carry between the words,
//                             one ballot per word.  Lane 0 stores the 8-byte record, lanes 0 .. 7 the eight mask words (64 bytes a
//                             read in pool memory, not compacted).
//   D2  cx_lengths            a thread per read (single-end) or pair: low or not, the bytes it adds to each output, summed per group of
//                             kCxGroup, the statistics — one atomic per block and counter — and the score histogram (LDS, then one
//                             atomic per block and bin that is not 0)
//       exclusive scans       one per output over the groups (rocprim), each with a last entry that is the output's size
//   D3  cx_write              a wave per group, as fq-trim's T3: a record that is its own input bytes and has no byte to change is one
//                             wave_copy; any other one its header, separator and quality pieces by wave_copy and the sequence piece
//                             by the lanes, a byte each under the read's mask words.
// D3 compares the two totals with the capacities before it stores anything: a result that does not fit leaves both outputs alone.
// D2 and D3 get a record's lengths from the same function (read_of).  Everything is integer / byte work; there is no CPU fallback.
#include "../../include/sc_fqcount.h"
#include "../../include/sc_fqcount_debug.h"

#include <cstring>        // (rocprim's texture iterator calls memset from host code)
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "scfq_reads_host.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

static_assert(sizeof(scfq_cplx_rec) == 8 && sizeof(scfq_cplx_stats) == 29 * 8 && sizeof(scfq_cplx_opts) == 40, "the ABI's sizes");

namespace {

thread_local char g_cerr[scfq_scratch::kErrBytes] = "";
thread_local double g_stage_ms[4] = {0, 0, 0, 0};

using scfq_reads::Dest;
using scfq_reads::DevBuf;
using scfq_reads::finish;
using scfq_reads::Mode;

constexpr uint32_t kCxWaves = 4;                         // reads a block of D1 works on at a time; groups of a block of D3
constexpr uint32_t kCxMaxBlocks = 4096;                  // of D1
constexpr uint32_t kCxWords = SCFQ_CPLX_MAX_LEN / 64;    // mask words of a read
constexpr uint32_t kCxGroup = kRecGroup;                 // reads or pairs of a group: one wave of D3, one entry of the scans
constexpr uint32_t kCxPad = 64;                          // invalid codes in front of position 0: j - d never leaves the array
constexpr uint16_t kNoFirst = 0xFFFF, kScoreTooLong = 0xFFFF;
static_assert(SCFQ_CPLX_MAX_LEN == 512 && kCxWords == 8, "a position is 9 bits, the mask words of a read are kept by lanes 0 .. 7");

// the counters of D2; the histogram follows them
enum { kTooLong = 0, kLow, kDropped, kMaskedReads, kIntervals, kBasesIn, kBasesOut, kMaskedBases, kMaskedBasesOut, kMaxScore, kCounters };

struct CxSteps { uint32_t window, threshold, mask, max_masked_pct; };

// what a wave of D1 keeps in LDS
struct CxWave {
  uint64_t near[SCFQ_CPLX_MAX_LEN];            // bit d - 1 of near[j]: t(j - d) == t(j), both valid
  uint32_t row[2][64];                         // row[w & 1][l]: best(64 w, 64 w + l - 1) of round w, as c << 6 | (l - 1)
  uint16_t reach[SCFQ_CPLX_MAX_LEN];           // per start: its furthest perfect end + 3, or 0
  uint8_t code[kCxPad + SCFQ_CPLX_MAX_LEN];    // t(i) at kCxPad + i, 0xFF for a triplet that is not valid
};

// the 2-bit code of a base in bits 0 and 1; bit 7 for a byte that is not exactly A C G T (bits 1 and 2 of 'A' 'C' 'T' 'G' are 0 1 2 3)
__device__ __forceinline__ uint32_t base_code(uint32_t b) {
  const uint32_t h = (b >> 1) & 3u;
  return (((0x47544341u >> (8 * h)) & 0xffu) == b) ? h : 0x80u;
}

__device__ __forceinline__ void wave_sync() {      // LDS written by one lane is read by another lane of the same wave
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// fractions as c << 6 | d, d = 1 .. 61, c <= 1891: the products below stay under 2^24
__device__ __forceinline__ uint32_t fr_num(uint32_t f) { return f >> 6; }
__device__ __forceinline__ uint32_t fr_den(uint32_t f) { return f & 63u; }
__device__ __forceinline__ bool fr_less(uint32_t a, uint32_t b) { return __umul24(fr_num(a), fr_den(b)) < __umul24(fr_num(b), fr_den(a)); }
constexpr uint32_t kFrZero = 1u;      // 0 / 1

// D1.  Read r is record r of `a` (single-end: paired = 0) or mate r & 1 of pair r >> 1: record p * stride of a, record p * stride + second
// of b.  maskw: kCxWords words per read.
__global__ __launch_bounds__(64 * kCxWaves) void cx_score(RecInput a, RecInput b, uint64_t stride, uint64_t second, uint32_t paired, uint64_t reads,
                                                         CxSteps st, scfq_cplx_rec* recs, uint64_t* maskw) {
  __shared__ CxWave lds[kCxWaves];
  const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  CxWave& my = lds[wave];
  my.code[lane] = 0xFF;                                      // (kCxPad == 64; written once, no round touches it)
  my.row[0][lane] = kFrZero;
  my.row[1][lane] = kFrZero;
  // (no block barrier: the waves of a block go their own ways)
  for (uint64_t r0 = (uint64_t)blockIdx.x * kCxWaves; r0 < reads; r0 += (uint64_t)gridDim.x * kCxWaves) {
    const uint64_t r = r0 + wave;
    if (r >= reads) continue;
    const uint64_t p = paired ? r >> 1 : r;
    const bool mate2 = paired && (r & 1);
    const RecInput& in = mate2 ? b : a;
    const uint64_t i = paired ? p * stride + (mate2 ? second : 0) : r;
    uint64_t ss, se;
    text_span(in, 4 * i + 1, ss, se);
    if (se - ss > SCFQ_CPLX_MAX_LEN) {
      if (lane == 0) recs[r] = scfq_cplx_rec{kScoreTooLong, 0, kNoFirst, 0};
      if (lane < kCxWords) maskw[r * kCxWords + lane] = 0;
      continue;
    }
    const int len = (int)(se - ss);
    const int nt = len >= 3 ? len - 2 : 0;                   // triplets
    const int rounds = (nt + 63) / 64;                       // 0 .. 8
    const int steps = std::min((int)st.window - 2, nt);      // the longest interval, in triplets
    uint32_t score = 0, count = 0;
    uint64_t my_word = 0;
    uint32_t masked = 0, first = kNoFirst;
    if (nt >= 2) {
      wave_sync();                                           // (the read before this one is done with the arrays)
      // the triplet codes of the rounds' positions
      for (int w = 0; w < rounds; ++w) {
        const int y = 64 * w + (int)lane;                    // < 512
        uint32_t t = 0xFFu;
        if (y < nt) {
          const uint32_t c0 = base_code(in.base[ss + (uint64_t)y]), c1 = base_code(in.base[ss + (uint64_t)y + 1]), c2 = base_code(in.base[ss + (uint64_t)y + 2]);
          t = ((c0 | c1 | c2) & 0x80u) ? 0xFFu : (c0 << 4) | (c1 << 2) | c2;
        }
        my.code[kCxPad + y] = (uint8_t)t;
      }
      wave_sync();
      // near(j): the equal triplets among the steps - 1 in front of j (kCxPad >= 61: the reads stay inside the array)
      for (int w = 0; w < rounds; ++w) {
        const int y = 64 * w + (int)lane;
        const uint32_t mine = my.code[kCxPad + y];
        uint64_t e = 0;
        for (int d = 1; d < steps; ++d) e |= (uint64_t)(my.code[kCxPad + y - d] == mine) << (d - 1);
        my.near[y] = mine == 0xFFu ? 0 : e;
      }
      wave_sync();
      uint32_t top = kFrZero;                                // the largest fraction this lane has seen
      for (int w = rounds - 1; w >= 0; --w) {
        const int s = 64 * w + (int)lane;
        const int last = std::min(steps, nt - 64 * w);       // lane 0's last step: the round's
        const uint32_t par = (uint32_t)w & 1u;
        uint32_t c = 0, best = kFrZero, reach = 0;
        for (int l = 2; l <= last; ++l) {
          const int j = s + l - 1;
          const bool active = j < nt;                        // (j < 512 then)
          const uint64_t e = active ? my.near[j] : 0;
          c += (uint32_t)__builtin_popcountll(e & ((1ull << (l - 1)) - 1ull));
          uint32_t nb = (uint32_t)__shfl_down((int)best, 1, 64);
          if (lane == 63) nb = my.row[par ^ 1u][l - 1];      // (entry 1 of a row is 0 / 1 for good)
          const uint32_t cur = (c << 6) | (uint32_t)(l - 1);
          const bool high = 10u * c > st.threshold * (uint32_t)(l - 1);
          const bool perfect = active && high && !fr_less(cur, best) && !fr_less(cur, nb);
          if (perfect) { reach = (uint32_t)j + 3u; ++count; }
          const uint32_t older = fr_less(best, nb) ? nb : best;
          if (active) best = fr_less(cur, older) ? older : cur;
          if (lane == 0) my.row[par][l] = best;              // (l <= 62)
        }
        if (fr_less(top, best)) top = best;
        my.reach[s] = (uint16_t)reach;
        wave_sync();                                         // the row of this round is the next one's
      }
      score = (uint32_t)wave_max((uint64_t)(10u * fr_num(top) / fr_den(top)));
      count = (uint32_t)wave_sum((uint64_t)count);
      // the mask plane: position y is masked iff a start at or in front of it reaches behind it
      uint32_t carry = 0;
      for (int w = 0; w < (len + 63) / 64; ++w) {
        const int y = 64 * w + (int)lane;
        uint32_t v = w < rounds ? my.reach[y] : 0u;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const uint32_t up = (uint32_t)__shfl_up((int)v, d, 64);
          if (lane >= (uint32_t)d) v = std::max(v, up);
        }
        v = std::max(v, carry);
        const uint64_t m = __builtin_amdgcn_ballot_w64((uint32_t)y < v);
        carry = (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
        if (m && first == kNoFirst) first = (uint32_t)(64 * w) + (uint32_t)__builtin_ctzll(m);
        masked += (uint32_t)__builtin_popcountll(m);
        if (lane == (uint32_t)w) my_word = m;
      }
    }
    if (lane == 0) recs[r] = scfq_cplx_rec{(uint16_t)score, (uint16_t)masked, (uint16_t)first, (uint16_t)count};
    if (lane < kCxWords) maskw[r * kCxWords + lane] = my_word;
  }
}

// what a read adds to its output if it is kept and where its pieces lie.  D2 and D3 both get it from here, so the lengths the scans saw
// are the lengths D3 writes
enum : uint32_t { kPieces = 0, kCopy, kEcho };
struct CxRead {
  uint64_t len;                        // bytes of the output record
  uint64_t hs, ss, ps, qs;             // starts of the header, sequence, separator and quality texts
  uint64_t idx;                        // the read's entry of the per-read table and of the mask words
  uint32_t hl, sl, pl, ql;             // their lengths
  uint32_t kind;                       // kPieces: the four pieces; kCopy: len bytes from hs on; kEcho: a too-long read
};

__device__ __forceinline__ CxRead read_of(const RecInput& in, uint64_t i, uint64_t idx, const scfq_cplx_rec& rec, uint32_t mask_mode, uint64_t& seq_len) {
  CxRead r = {};
  uint64_t e;
  r.idx = idx;
  text_span(in, 4 * i + 1, r.ss, e);
  seq_len = e - r.ss;
  if (rec.score == kScoreTooLong) {
    r.kind = kEcho;
    r.len = echo_len(in, i);
    return r;
  }
  r.sl = (uint32_t)seq_len;
  text_span(in, 4 * i, r.hs, e);
  r.hl = (uint32_t)(e - r.hs);                          // (a header or quality line of 4 GiB or more is not supported: the lengths are 32-bit)
  text_span(in, 4 * i + 2, r.ps, e);
  r.pl = (uint32_t)(e - r.ps);
  text_span(in, 4 * i + 3, r.qs, e);
  r.ql = (uint32_t)(e - r.qs);
  r.len = (uint64_t)r.hl + r.sl + r.pl + r.ql + 4;
  // all four lines there, the last one with its newline, nothing left out of any and no byte to change: the record's own bytes
  if ((rec.masked == 0 || mask_mode == SCFQ_CPLX_MASK_NONE) && 4 * i + 4 <= in.lines) {
    const uint64_t r1 = in.line_off[4 * i + 4];
    if (r1 <= in.n && r1 - in.line_off[4 * i] == r.len) r.kind = kCopy;
  }
  return r;
}

// a kept read's record, by the whole wave
__device__ __forceinline__ void write_read(const RecInput& in, uint64_t i, const CxRead& r, const uint64_t* maskw, uint32_t mask_mode, uint8_t* dst, uint32_t lane) {
  if (r.kind == kEcho) { echo_record(in, i, dst, r.len, lane); return; }
  if (r.kind == kCopy) { wave_copy(dst, in.base + r.hs, r.len, lane); return; }
  uint8_t* const s = dst + r.hl + 1;
  uint8_t* const p = s + r.sl + 1;
  uint8_t* const q = p + r.pl + 1;
  wave_copy(dst, in.base + r.hs, r.hl, lane);
  for (uint32_t w = 0; 64 * w < r.sl; ++w) {                // (sl <= 512: at most kCxWords words)
    const uint32_t y = 64 * w + lane;
    const bool bit = (maskw[r.idx * kCxWords + w] >> lane) & 1ull;
    if (y < r.sl) {
      uint8_t c = in.base[r.ss + y];
      if (bit && mask_mode == SCFQ_CPLX_MASK_N) c = 'N';
      if (bit && mask_mode == SCFQ_CPLX_MASK_LOWER && c >= 'A' && c <= 'Z') c |= 0x20;
      s[y] = c;
    }
  }
  wave_copy(p, in.base + r.ps, r.pl, lane);
  wave_copy(q, in.base + r.qs, r.ql, lane);
  if (lane == 0) dst[r.hl] = '\n';
  if (lane == 1) s[r.sl] = '\n';
  if (lane == 2) p[r.pl] = '\n';
  if (lane == 3) q[r.ql] = '\n';
}

// a unit: a single-end read, or a pair.  What its reads add to the two outputs, and whether it is kept
struct CxUnit {
  CxRead m[2];
  uint64_t len1, len2;                 // bytes for out1 and out2 (0 for a dropped unit)
  uint64_t first;                      // of len1, mate 1's record (interleaved input: mate 2's follows it)
  uint64_t seq_len[2];
  scfq_cplx_rec rec[2];
  uint32_t mates;
  bool low[2], dropped;
};

__device__ __forceinline__ CxUnit look_up(const RecInput& a, const RecInput& b, uint64_t stride, uint64_t second, uint32_t paired, uint64_t u,
                                          const scfq_cplx_rec* recs, const CxSteps& st) {
  CxUnit t = {};
  t.mates = paired ? 2u : 1u;
#pragma unroll
  for (uint32_t k = 0; k < 2; ++k) {
    if (k < t.mates) {
      const uint64_t idx = paired ? 2 * u + k : u;
      t.rec[k] = recs[idx];
      t.m[k] = read_of(k ? b : a, paired ? u * stride + (k ? second : 0) : u, idx, t.rec[k], st.mask, t.seq_len[k]);
      t.low[k] = t.rec[k].score != kScoreTooLong && t.seq_len[k] >= 1 && 100ull * t.rec[k].masked > (uint64_t)st.max_masked_pct * t.seq_len[k];
      t.dropped = t.dropped || t.low[k];
    }
  }
  if (t.dropped) return t;
  t.first = t.m[0].len;
  t.len1 = t.first + (paired && second ? t.m[1].len : 0);
  t.len2 = paired && !second ? t.m[1].len : 0;
  return t;
}

// D2.  group_len: two arrays of n_groups + 1 entries, one after the other (the last entry of each stays 0: the scan's total).  counters:
// kCounters words, then the SCFQ_CPLX_SCORE_BINS of the histogram.  lens: L of every read, for the per-read rows of the file form
__global__ __launch_bounds__(256) void cx_lengths(RecInput a, RecInput b, uint64_t stride, uint64_t second, uint32_t paired, uint64_t units,
                                                 const scfq_cplx_rec* recs, CxSteps st, uint64_t n_groups, uint64_t* group_len, uint32_t* lens,
                                                 unsigned long long* counters) {
  __shared__ uint64_t sum_sh[kCounters][4];
  __shared__ uint32_t hist_sh[SCFQ_CPLX_SCORE_BINS];
  for (uint32_t k = threadIdx.x; k < SCFQ_CPLX_SCORE_BINS; k += 256) hist_sh[k] = 0;
  __syncthreads();
  const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint64_t len[2] = {0, 0}, c[kCounters];
#pragma unroll
  for (int k = 0; k < kCounters; ++k) c[k] = 0;
  if (u < units) {
    const CxUnit t = look_up(a, b, stride, second, paired, u, recs, st);
    len[0] = t.len1; len[1] = t.len2;
#pragma unroll
    for (uint32_t k = 0; k < 2; ++k) {
      if (k >= t.mates) continue;
      const scfq_cplx_rec rec = t.rec[k];
      const bool too_long = rec.score == kScoreTooLong;
      const uint64_t sl = t.seq_len[k];
      lens[t.m[k].idx] = (uint32_t)std::min<uint64_t>(sl, 0xFFFFFFFFull);
      c[kTooLong] += too_long;
      c[kLow] += t.low[k];
      c[kDropped] += t.dropped;
      c[kMaskedReads] += rec.masked != 0;
      c[kIntervals] += rec.intervals;
      c[kBasesIn] += sl;
      c[kBasesOut] += t.dropped ? 0 : sl;
      c[kMaskedBases] += rec.masked;
      c[kMaskedBasesOut] += t.dropped ? 0 : rec.masked;
      if (!too_long) c[kMaxScore] = std::max<uint64_t>(c[kMaxScore], rec.score);
      atomicAdd(&hist_sh[too_long ? SCFQ_CPLX_SCORE_BINS - 1 : std::min<uint32_t>(rec.score, SCFQ_CPLX_SCORE_BINS - 2)], 1u);
    }
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) store_group_len(len[k], k, u, units, n_groups, group_len);
  // the statistics: ONE atomic per block and counter (dd_count_marks: an atomic per wave on one address costs more than the kernel)
#pragma unroll
  for (int k = 0; k < kCounters; ++k) {
    const uint64_t s = k == kMaxScore ? wave_max(c[k]) : wave_sum(c[k]);
    if ((threadIdx.x & 63) == 0) sum_sh[k][threadIdx.x >> 6] = s;
  }
  __syncthreads();
  if (threadIdx.x < kCounters) {
    const uint64_t* v = sum_sh[threadIdx.x];
    if (threadIdx.x == kMaxScore) {
      const uint64_t t = std::max(std::max(v[0], v[1]), std::max(v[2], v[3]));
      if (t) atomicMax(&counters[threadIdx.x], (unsigned long long)t);
    } else {
      const uint64_t t = v[0] + v[1] + v[2] + v[3];
      if (t) atomicAdd(&counters[threadIdx.x], (unsigned long long)t);
    }
  }
  for (uint32_t k = threadIdx.x; k < SCFQ_CPLX_SCORE_BINS; k += 256)
    if (hist_sh[k]) atomicAdd(&counters[kCounters + k], (unsigned long long)hist_sh[k]);
}

using ::bcast;      // (the overload below hides the shared ones otherwise)
__device__ __forceinline__ CxRead bcast(const CxRead& m, uint32_t from) {
  CxRead r;
  r.len = bcast(m.len, from);
  r.hs = bcast(m.hs, from); r.ss = bcast(m.ss, from); r.ps = bcast(m.ps, from); r.qs = bcast(m.qs, from);
  r.idx = bcast(m.idx, from);
  r.hl = bcast(m.hl, from); r.sl = bcast(m.sl, from); r.pl = bcast(m.pl, from); r.ql = bcast(m.ql, from);
  r.kind = bcast(m.kind, from);
  return r;
}

// D3.  group_off: the two scanned arrays of D2's layout
__global__ __launch_bounds__(64 * kCxWaves) void cx_write(RecInput a, RecInput b, uint64_t stride, uint64_t second, uint32_t paired, uint64_t units,
                                                         const scfq_cplx_rec* recs, const uint64_t* maskw, CxSteps st, uint64_t n_groups,
                                                         const uint64_t* group_off, RecOut o1, RecOut o2) {
  const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // (when one result is more than its output holds, nothing is written to either)
  if (!(output_fits(o1, 0, n_groups, group_off) && output_fits(o2, 1, n_groups, group_off))) return;
  const uint64_t g = (uint64_t)blockIdx.x * kCxWaves + wave;
  if (g >= n_groups) return;
  const uint64_t u0 = g * kCxGroup;
  const uint32_t count = (uint32_t)std::min<uint64_t>(kCxGroup, units - u0);
  CxUnit mine = {};
  if (lane < count) mine = look_up(a, b, stride, second, paired, u0 + lane, recs, st);
  const uint64_t len[2] = {mine.len1, mine.len2};
  uint64_t at[2];
  place_units(len, g, n_groups, group_off, lane, at);
  for (uint32_t q = 0; q < count; ++q) {
    const uint64_t l1 = bcast(mine.len1, q), l2 = bcast(mine.len2, q), first = bcast(mine.first, q), w1 = bcast(at[0], q), w2 = bcast(at[1], q);
    if (l1 + l2 == 0) continue;                            // (a dropped unit; a kept record has its four '\n' at the least, or is an echo of nothing)
    const uint64_t u = u0 + q;
    const uint64_t i1 = paired ? u * stride : u, i2 = u * stride + second;
    const CxRead m1 = bcast(mine.m[0], q);                 // (every lane takes part in the shuffles)
    if (o1.p && first) write_read(a, i1, m1, maskw, st.mask, o1.p + w1, lane);
    if (paired) {
      const CxRead m2 = bcast(mine.m[1], q);
      if (second) { if (o1.p && m2.len) write_read(b, i2, m2, maskw, st.mask, o1.p + w1 + first, lane); }
      else if (o2.p && m2.len) write_read(b, i2, m2, maskw, st.mask, o2.p + w2, lane);
    }
  }
}

struct Params {
  uint32_t flags;
  CxSteps steps;
};

bool args_ok(const scfq_cplx_opts* opts, const scfq_cplx_stats* st, Params& p) {
  if (!st || st->struct_size != sizeof(scfq_cplx_stats)) return false;
  p.flags = 0;
  p.steps = CxSteps{64, 20, SCFQ_CPLX_MASK_LOWER, 100};
  if (opts) {
    if (opts->struct_size != sizeof(scfq_cplx_opts)) return false;
    p.flags = opts->flags;
    p.steps = CxSteps{opts->window, opts->threshold, opts->mask, opts->max_masked_pct};
    const uint32_t known = SCFQ_CPLX_INTERLEAVED;
    const CxSteps& s = p.steps;
    if (p.flags & ~known) { std::snprintf(g_cerr, sizeof g_cerr, "unknown flag bits 0x%x", p.flags & ~known); return false; }
    if (s.window < 8 || s.window > 64) { std::snprintf(g_cerr, sizeof g_cerr, "window %u is not in 8 .. 64", s.window); return false; }
    if (s.threshold < 1 || s.threshold > 310) { std::snprintf(g_cerr, sizeof g_cerr, "threshold %u is not in 1 .. 310", s.threshold); return false; }
    if (s.mask > SCFQ_CPLX_MASK_N) { std::snprintf(g_cerr, sizeof g_cerr, "mask %u is not in 0 .. 2", s.mask); return false; }
    if (s.max_masked_pct > 100) { std::snprintf(g_cerr, sizeof g_cerr, "max_masked_pct %u is not in 0 .. 100", s.max_masked_pct); return false; }
    if (opts->reserved[0] || opts->reserved[1] || opts->reserved[2]) {
      std::snprintf(g_cerr, sizeof g_cerr, "the reserved words are %u, %u and %u, not 0", opts->reserved[0], opts->reserved[1], opts->reserved[2]);
      return false;
    }
  }
  return true;
}

// recs_dev / recs_cap: the caller's per-read table in device memory, or nullptr; want_recs with check_recs: a table of recs_cap entries is
// wanted wherever it lives, and one that is too small is an error once the statistics are complete.  recs_keep, lens_keep: where the
// table and the lengths stay for the caller of this function.  hist_host: nullptr, or SCFQ_CPLX_SCORE_BINS words
int cplx_device(const uint8_t* d1, uint64_t n1, const uint8_t* d2, uint64_t n2, Mode mode, const Params& prm, scfq_cplx_rec* recs_dev, bool want_recs,
                uint64_t recs_cap, bool check_recs, DevBuf& recs_keep, DevBuf& lens_keep, uint64_t* hist_host, bool own_outputs, Dest dst[2], DevBuf own[2],
                bool check_caps, scfq_cplx_stats* st, hipStream_t stream) {
  for (double& m : g_stage_ms) m = 0;
  const bool paired = mode != Mode::single, interleaved = mode == Mode::interleaved;
  st->input_bytes1 = n1;
  st->input_bytes2 = n2;
  st->flags = prm.flags; st->window = prm.steps.window; st->threshold = prm.steps.threshold; st->mask = prm.steps.mask;
  st->max_masked_pct = prm.steps.max_masked_pct;
  if (hist_host) std::memset(hist_host, 0, SCFQ_CPLX_SCORE_BINS * 8);
  scfq_overlap::Indexed ix;
  int rc = SCFQ_OK;
  double index_ms = 0;
  uint64_t units = 0, reads = 0;
  if ((rc = scfq_reads::index_units(d1, n1, d2, n2, mode, stream, g_cerr, ix, &index_ms, st, &units, &reads))) return rc;
  st->reads_in = reads;
  const bool recs_small = check_recs && want_recs && recs_cap < reads;
  if (units == 0) return SCFQ_OK;           // (two empty outputs: they fit into anything)
  const uint64_t n_groups = (units + kCxGroup - 1) / kCxGroup;
  const bool to_caller = recs_dev && !recs_small;
  constexpr size_t kWordsOut = kCounters + SCFQ_CPLX_SCORE_BINS;
  DevBuf maskw, group_len, group_off, counters, tmp;
  scfq_reads::GroupScan gs(2, n_groups, group_len, group_off, stream, g_cerr);
  if ((!to_caller && (rc = recs_keep.alloc(reads * sizeof(scfq_cplx_rec), stream, g_cerr))) || (rc = lens_keep.alloc(reads * 4, stream, g_cerr)) ||
      (rc = maskw.alloc(reads * kCxWords * 8, stream, g_cerr)) || (rc = gs.alloc()) || (rc = counters.alloc(kWordsOut * 8, stream, g_cerr)))
    return rc;
  scfq_cplx_rec* const recs = to_caller ? recs_dev : recs_keep.as<scfq_cplx_rec>();
  size_t scan_bytes = 0;
  if ((rc = gs.scratch_bytes(&scan_bytes)) || (rc = tmp.alloc(scan_bytes, stream, g_cerr))) return rc;
  static const bool timing = scfq_scratch::env_switch("SCFQ_CPLX_TIMING");
  scfq_scratch::StageClock clk(stream, timing);
  SCFQ_SCRATCH_CHK(g_cerr, hipMemsetAsync(counters.p, 0, kWordsOut * 8, stream));
  if ((rc = gs.zero())) return rc;
  const RecInput a = {d1, n1, ix.off1.as<uint64_t>(), ix.lines1, ix.cr1};
  const RecInput b = mode == Mode::two ? RecInput{d2, n2, ix.off2.as<uint64_t>(), ix.lines2, ix.cr2} : a;
  const uint64_t stride = interleaved ? 2 : 1, second = interleaved ? 1 : 0;
  clk.mark(0);
  hipLaunchKernelGGL(cx_score, dim3((unsigned)std::min<uint64_t>((reads + kCxWaves - 1) / kCxWaves, kCxMaxBlocks)), dim3(64 * kCxWaves), 0, stream, a, b, stride,
                     second, paired ? 1u : 0u, reads, prm.steps, recs, maskw.as<uint64_t>());
  SCFQ_SCRATCH_CHK(g_cerr, hipGetLastError());
  clk.mark(1);
  hipLaunchKernelGGL(cx_lengths, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, stream, a, b, stride, second, paired ? 1u : 0u, units, recs, prm.steps,
                     n_groups, gs.len(), lens_keep.as<uint32_t>(), counters.as<unsigned long long>());
  SCFQ_SCRATCH_CHK(g_cerr, hipGetLastError());
  if ((rc = gs.scan(tmp.p, scan_bytes))) return rc;
  clk.mark(2);
  // the sizes and the statistics come back first: pool memory for the outputs is taken to fit, and a caller's buffer that is too small
  // is known here
  std::vector<uint64_t> h(kWordsOut);
  if ((rc = gs.read_totals())) return rc;
  SCFQ_SCRATCH_CHK(g_cerr, hipMemcpyAsync(h.data(), counters.p, kWordsOut * 8, hipMemcpyDeviceToHost, stream));
  SCFQ_SCRATCH_CHK(g_cerr, hipStreamSynchronize(stream));
  st->out1_bytes = gs.total[0]; st->out2_bytes = gs.total[1];
  st->too_long = h[kTooLong]; st->low_reads = h[kLow]; st->dropped_reads = h[kDropped]; st->reads_out = reads - h[kDropped];
  st->masked_reads = h[kMaskedReads]; st->perfect_intervals = h[kIntervals];
  st->bases_in = h[kBasesIn]; st->bases_out = h[kBasesOut]; st->masked_bases = h[kMaskedBases]; st->masked_bases_out = h[kMaskedBasesOut];
  st->max_score = h[kMaxScore];
  if (hist_host) std::memcpy(hist_host, h.data() + kCounters, SCFQ_CPLX_SCORE_BINS * 8);
  const scfq_reads::Placement put = scfq_reads::place_outputs(gs, scfq_reads::kOutNames, dst, own_outputs, check_caps, recs_small, own, stream, g_cerr);
  if (put.rc) return put.rc;
  if (put.out[0].p || put.out[1].p) {
    hipLaunchKernelGGL(cx_write, dim3((unsigned)((n_groups + kCxWaves - 1) / kCxWaves)), dim3(64 * kCxWaves), 0, stream, a, b, stride, second, paired ? 1u : 0u,
                       units, recs, maskw.as<uint64_t>(), prm.steps, n_groups, gs.off(), put.out[0], put.out[1]);
    SCFQ_SCRATCH_CHK(g_cerr, hipGetLastError());
  }
  clk.mark(3);
  SCFQ_SCRATCH_CHK(g_cerr, hipStreamSynchronize(stream));
  g_stage_ms[0] = index_ms;
  g_stage_ms[1] = clk.between(0, 1);
  g_stage_ms[2] = clk.between(1, 2);
  g_stage_ms[3] = clk.between(2, 3);
  if (recs_small) {
    std::snprintf(g_cerr, sizeof g_cerr, "the per-read table holds %llu entries, the input has %llu reads", (unsigned long long)recs_cap, (unsigned long long)reads);
    return SCFQ_EARG;
  }
  return put.verdict;      // (SCFQ_EARG for an output that is too small: place_outputs has left the text)
}

}  // namespace

extern "C" {

const char* scfq_cplx_error_detail(void) { return g_cerr; }

int scfq_debug_cplx_stages(double* ms, uint32_t cap) { return scfq_scratch::copy_stage_ms(g_stage_ms, ms, cap); }

int scfq_format_cplx_stats_tsv(const scfq_cplx_stats* s, int header, char* buf, uint64_t cap) {
  static const char kNames[] = "reads_in\treads_out\tdropped_reads\tlow_reads\ttoo_long\tpairs\tunpaired\tmasked_reads\tperfect_intervals\tbases_in\tbases_out\t"
                               "masked_bases\tmasked_bases_out\tmax_score\tout1_bytes\tout2_bytes";
  if (header) return scfq_reads::copy_text(kNames, (int)sizeof kNames - 1, buf, cap);
  if (!s) return SCFQ_EARG;
  const uint64_t v[] = {s->reads_in, s->reads_out, s->dropped_reads, s->low_reads, s->too_long, s->pairs, s->unpaired, s->masked_reads, s->perfect_intervals,
                        s->bases_in, s->bases_out, s->masked_bases, s->masked_bases_out, s->max_score, s->out1_bytes, s->out2_bytes};
  char tmp[512];
  int m = 0;
  for (const uint64_t x : v) m += std::snprintf(tmp + m, sizeof tmp - m, m ? "\t%llu" : "%llu", (unsigned long long)x);
  return scfq_reads::copy_text(tmp, m, buf, cap);
}

int scfq_format_cplx_rec_tsv(uint64_t read, const scfq_cplx_rec* r, uint64_t length, char* buf, uint64_t cap) {
  static const char kNames[] = "read\tlength\tscore\tmasked\tfirst\tintervals";
  if (!r) return scfq_reads::copy_text(kNames, (int)sizeof kNames - 1, buf, cap);
  char tmp[160], score[16] = "-", first[16] = "-";
  if (r->score != kScoreTooLong) std::snprintf(score, sizeof score, "%u", (unsigned)r->score);
  if (r->first != kNoFirst) std::snprintf(first, sizeof first, "%u", (unsigned)r->first);
  const int m = std::snprintf(tmp, sizeof tmp, "%llu\t%llu\t%s\t%u\t%s\t%u", (unsigned long long)read, (unsigned long long)length, score, (unsigned)r->masked, first,
                              (unsigned)r->intervals);
  return scfq_reads::copy_text(tmp, m, buf, cap);
}

int scfq_cplx_buffers(const void* r1, uint64_t n1, const void* r2, uint64_t n2, int is_device, const scfq_cplx_opts* opts, scfq_cplx_rec* recs, uint64_t recs_cap,
                      uint64_t* hist_host, void* out1, uint64_t cap1, void* out2, uint64_t cap2, int out_is_device, scfq_cplx_stats* stats) {
  g_cerr[0] = '\0';
  Params prm;
  if (!args_ok(opts, stats, prm) || (!r1 && n1) || (!r2 && n2) || (!out1 && cap1) || (!out2 && cap2) || (!recs && recs_cap)) return SCFQ_EARG;
  const bool interleaved = (prm.flags & SCFQ_CPLX_INTERLEAVED) != 0;
  if (interleaved && (r2 || n2)) { std::snprintf(g_cerr, sizeof g_cerr, "interleaved input takes no second buffer"); return SCFQ_EARG; }
  const Mode mode = interleaved ? Mode::interleaved : (r2 ? Mode::two : Mode::single);
  if (mode != Mode::two && out2) { std::snprintf(g_cerr, sizeof g_cerr, "one input has no second output (out2)"); return SCFQ_EARG; }
  scfq_scratch::clear_keep_size(stats);
  Dest dst[2] = {{static_cast<uint8_t*>(out1), cap1, out1 != nullptr}, {static_cast<uint8_t*>(out2), cap2, out2 != nullptr}};
  const bool any_out = out1 || out2, direct = any_out && out_is_device, recs_on_device = recs && out_is_device;
  scfq_scratch::ResidentInput in1, in2;
  int rc = in1.from_buffer(r1, n1, is_device != 0, is_device || direct || recs_on_device, g_cerr);
  if (rc) return rc;
  // (a host buffer's copy is waited for inside; device memory of the caller is ordered before in1's stream above)
  if (mode == Mode::two && (rc = in2.from_buffer(r2, n2, is_device != 0, false, g_cerr))) return rc;
  DevBuf own[2], recs_keep, lens_keep;
  rc = cplx_device(in1.d_in, in1.n, in2.d_in, in2.n, mode, prm, recs_on_device ? recs : nullptr, recs != nullptr, recs_cap, true, recs_keep, lens_keep, hist_host,
                   /*own_outputs=*/!direct, dst, own, /*check_caps=*/true, stats, in1.stream);
  if (rc) return finish(in1, rc);
  if (recs && !recs_on_device && stats->reads_in)
    SCFQ_SCRATCH_CHK(g_cerr, hipMemcpyAsync(recs, recs_keep.p, stats->reads_in * sizeof(scfq_cplx_rec), hipMemcpyDeviceToHost, in1.stream));
  if (!direct) {
    const uint64_t bytes[2] = {stats->out1_bytes, stats->out2_bytes};
    if ((rc = scfq_reads::outputs_to_host(2, dst, own, bytes, in1.stream, g_cerr))) return rc;
  }
  SCFQ_SCRATCH_CHK(g_cerr, hipStreamSynchronize(in1.stream));
  for (DevBuf& o : own) o.drop();
  recs_keep.drop();
  lens_keep.drop();
  in1.mark_clean();      // (the last act was to wait for the stream; behind it lie returns of pool memory only)
  return SCFQ_OK;
}

int scfq_cplx_files(const char* path1, const char* path2, const scfq_opts* opts, const scfq_cplx_opts* copts, int out1_fd, int out2_fd, int per_read_fd,
                    uint64_t* hist_host, scfq_cplx_stats* stats) {
  g_cerr[0] = '\0';
  Params prm;
  if (!path1 || !args_ok(copts, stats, prm)) return SCFQ_EARG;
  const bool interleaved = (prm.flags & SCFQ_CPLX_INTERLEAVED) != 0;
  if (interleaved && path2) { std::snprintf(g_cerr, sizeof g_cerr, "interleaved input takes no second file"); return SCFQ_EARG; }
  const Mode mode = interleaved ? Mode::interleaved : (path2 ? Mode::two : Mode::single);
  if (mode != Mode::two && out2_fd >= 0) { std::snprintf(g_cerr, sizeof g_cerr, "one input has no second output (out2)"); return SCFQ_EARG; }
  scfq_scratch::clear_keep_size(stats);
  scfq_scratch::ResidentInput in1, in2;
  int rc = in1.from_file(path1, opts, g_cerr);
  if (rc) return rc;
  if (mode == Mode::two && (rc = in2.from_file(path2, opts, g_cerr))) return rc;      // (staged when this returns)
  const int fd[2] = {out1_fd, out2_fd};
  Dest dst[2] = {{nullptr, 0, out1_fd >= 0}, {nullptr, 0, out2_fd >= 0}};
  DevBuf own[2], recs_keep, lens_keep;
  rc = cplx_device(in1.d_in, in1.n, in2.d_in, in2.n, mode, prm, nullptr, false, 0, false, recs_keep, lens_keep, hist_host, /*own_outputs=*/true, dst, own,
                   /*check_caps=*/false, stats, in1.stream);
  if (rc) return finish(in1, rc);
  if (per_read_fd >= 0 && stats->reads_in) {
    // the table and the lengths come to the host whole; the rows leave in pieces of about 1 MiB
    const uint64_t reads = stats->reads_in;
    std::vector<scfq_cplx_rec> recs(reads);
    std::vector<uint32_t> lens(reads);
    SCFQ_SCRATCH_CHK(g_cerr, hipMemcpyAsync(recs.data(), recs_keep.p, reads * sizeof(scfq_cplx_rec), hipMemcpyDeviceToHost, in1.stream));
    SCFQ_SCRATCH_CHK(g_cerr, hipMemcpyAsync(lens.data(), lens_keep.p, reads * 4, hipMemcpyDeviceToHost, in1.stream));
    SCFQ_SCRATCH_CHK(g_cerr, hipStreamSynchronize(in1.stream));
    std::string text;
    char row[160];
    for (uint64_t i = 0; i < reads; ++i) {
      const int m = scfq_format_cplx_rec_tsv(i, &recs[i], lens[i], row, sizeof row);
      text.append(row, (size_t)m);
      text.push_back('\n');
      if (text.size() >= (1u << 20) || i + 1 == reads) {
        if ((rc = scfq_fdwrite::write_all(per_read_fd, reinterpret_cast<const uint8_t*>(text.data()), text.size(), g_cerr))) return finish(in1, rc);
        text.clear();
      }
    }
  }
  const uint64_t bytes[2] = {stats->out1_bytes, stats->out2_bytes};
  return scfq_reads::outputs_to_fds(2, own, bytes, fd, in1, g_cerr);
}

}  // extern "C"

// scfq_norm.hip — `sc fq-normalize` on the MI355X (gfx950): the k-mer depth of every read against an fq-kcount table, and the reads
// that the depth rule keeps.  Not in the reference; definitions in include/sc_fqcount.h.
//
// A call, the inputs in HBM whole (one FASTQ, two, or one interleaved), the table behind a handle of scfq_kcount.hip (or counted here
// first from the same resident inputs and the same line indexes: scfq_kcount_internal.hpp):
//   K5  line index            (scfq_scratch::build_line_index) of each input
//   N0  nm_long_windows       a thread per read: the windows of the reads that have more than `lds_windows` of them, summed; the host sizes
//                             the device array of their counts by it (4 bytes per window, nothing for ordinary reads)
//   N1  nm_depth              the hot path, S2's shape: a wave per read, kNmWaves waves per block, persistent blocks that stride over the
//                             reads of both inputs.  The read goes through LDS in chunks of 512 window starts: 2 bits per base and a plane
//                             with a bit per base that is not exactly A C G T.  Lane l takes the windows l, l + 64, ...: a funnel shift of
//                             two words is the key (the minimum with its reverse complement in canonical mode), one masked test of the
//                             invalid plane rejects the window, every other one probes the slots as kc_query does: plain 16-byte loads,
//                             at most max_probe slots, ending at the key or at an empty slot.  The count, saturated at 2^32 - 2, or the
//                             marker 2^32 - 1 of an invalid window goes to the wave's array of kNmC words in LDS — for a read with more
//                             windows, to its piece of the device array, taken with one atomic add per read.  kmers, weak, the minimum
//                             and the maximum are wave reductions.  The lower median is a radix select of rank (kmers - 1) / 2 over the
//                             array: one round per bit from the maximum's top bit down, each a ballot and a population count per 64
//                             entries; markers are the largest values there are and the rank never reaches them.  Lane 0 stores 16 bytes.
//   N2  nm_decide             a thread per unit (a read, or a pair): the rule (scfq_norm_host::classify), the bytes it adds to each output
//                             summed per group of kNmGroup, the statistics, the two histogram columns (the first kNmHistLds bins in LDS)
//       exclusive scans       one per output over the groups (rocprim), each with a last entry that is the output's size
//   N3  nm_write              a wave per group echoes the kept records with wave_copy
// Every loop is bounded: probes by max_probe, select rounds by 32, chunk loops by the line's length from the index.  Nothing spins and no
// block waits for another.  There is no CPU fallback.
// (The front of N1 repeats S2's of scfq_screen.hip: the two kernels part ways inside their window loop.)
#include "../../include/sc_fqcount.h"
#include "../../include/sc_fqcount_debug.h"

#include <cstring>        // (rocprim's texture iterator calls memset from host code)
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "scfq_kcount_internal.hpp"
#include "scfq_norm_host.hpp"
#include "scfq_reads_host.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>

static_assert(sizeof(scfq_norm_rec) == 16 && sizeof(scfq_norm_stats) == 37 * 8 && sizeof(scfq_norm_opts) == 48, "the ABI's sizes");

namespace {

using namespace scfq_norm_host;
using scfq_kcount_host::kEmpty;
using scfq_kcount_host::mix64;
using scfq_reads::Dest;
using scfq_reads::DevBuf;
using scfq_reads::finish;
using scfq_reads::Mode;

thread_local char g_nerr[scfq_scratch::kErrBytes] = "";
thread_local double g_stage_ms[4] = {0, 0, 0, 0};

constexpr uint32_t kNmWaves = 4;                         // reads a block of N1 works on at a time; groups of a block of N3
constexpr uint32_t kNmMaxBlocks = 2048;                  // of N1
constexpr uint32_t kNmGroup = kRecGroup;                 // units of a group: one wave of N3, one entry of the scans
constexpr uint32_t kChunk = 512;                         // window starts of a chunk of N1
constexpr uint32_t kCodeWords = 18, kInvWords = 10;      // 64-bit words of a wave's two planes: 9 rounds of 64 bases, and the word behind
constexpr uint32_t kNmC = 2048;                          // counts of a wave in LDS: 8 KiB
constexpr uint32_t kNmMinC = 64;                         // the least SCFQ_NORM_LDS_WINDOWS
constexpr uint32_t kMarker = 0xFFFFFFFFu;                // "no k-mer here"
constexpr uint32_t kNmHistLds = 2048;                    // bins of N2 that live in LDS (two columns of 32-bit counters)
constexpr uint32_t kNmDecideBlocks = 1024;
static_assert(kChunk + SCFQ_KCOUNT_MAX_K - 1 <= 9 * 64, "a chunk's bases are nine rounds of the wave");
static_assert(kMarker == SCFQ_NORM_MAX_DEPTH + 1u, "the marker lies above every count");

struct alignas(16) KcSlot { unsigned long long key, count; };      // (scfq_kcount.hip's slot)

struct NmTable {          // the table as N1 sees it
  const KcSlot* slots;
  uint64_t slot_mask, ones;
  uint32_t max_probe, k, weak_below;
};

struct NmRule { uint32_t target, min_depth, keep_no_kmers; uint64_t seed; };

// the words N0 and N1 add into
enum : uint32_t { kCuLongReads = 0, kCuLongWindows = 1, kCuCursor = 2, kCuAbsent = 3, kCuOverrun = 4, kCuWords = 5 };

// what a wave has written to LDS is read by its other lanes behind this
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the reverse complement of the k-mer index f (2k bits): complement, then the 2-bit groups of the 64-bit word in reverse order
__device__ __forceinline__ uint64_t rev_comp(uint64_t f, uint32_t k) {
  uint64_t r = __builtin_bswap64(~f);
  r = ((r & 0xF0F0F0F0F0F0F0F0ull) >> 4) | ((r & 0x0F0F0F0F0F0F0F0Full) << 4);
  r = ((r & 0xCCCCCCCCCCCCCCCCull) >> 2) | ((r & 0x3333333333333333ull) << 2);
  return r >> (64 - 2 * k);                              // (k >= 13: a shift of 0 .. 38)
}

// Read r is record r of `a` (single-end: paired = 0) or mate r & 1 of pair r >> 1: record p * stride of a, record p * stride + second of b.
__device__ __forceinline__ const RecInput& read_text(const RecInput& a, const RecInput& b, uint64_t stride, uint64_t second, uint32_t paired, uint64_t r,
                                                    uint64_t& ss, uint64_t& se) {
  const uint64_t p = paired ? r >> 1 : r;
  const bool mate2 = paired && (r & 1);
  const RecInput& in = mate2 ? b : a;
  const uint64_t i = paired ? p * stride + (mate2 ? second : 0) : r;
  text_span(in, 4 * i + 1, ss, se);
  return in;
}

// N0.  cu[kCuLongReads], cu[kCuLongWindows]: the reads with more than lds_windows windows and the sum of their windows
__global__ __launch_bounds__(256) void nm_long_windows(RecInput a, RecInput b, uint64_t stride, uint64_t second, uint32_t paired, uint64_t reads, uint32_t k,
                                                      uint32_t lds_windows, unsigned long long* cu) {
  uint64_t n_long = 0, w_long = 0;
  for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < reads; r += (uint64_t)gridDim.x * 256) {
    uint64_t ss, se;
    read_text(a, b, stride, second, paired, r, ss, se);
    const uint64_t len = se - ss, n_win = len >= k ? len - k + 1 : 0;
    if (n_win > lds_windows) { ++n_long; w_long += n_win; }
  }
  n_long = wave_sum(n_long);
  w_long = wave_sum(w_long);
  if ((threadIdx.x & 63) == 0 && n_long) {
    atomicAdd(&cu[kCuLongReads], (unsigned long long)n_long);
    atomicAdd(&cu[kCuLongWindows], (unsigned long long)w_long);
  }
}

// the entry of a read's counts: the wave's LDS array, or the read's piece of the device array (written by this wave, read back through
// the L2: an atomic load at agent scope does not look into the CU's vector cache)
template <bool kLds>
__device__ __forceinline__ uint32_t count_at(const uint32_t* lds, const uint32_t* dev, uint64_t i) {
  if (kLds) return lds[i];
  return __hip_atomic_load(dev + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the value of rank `rank` (0-based) among entries [0, n) of the array; mx: the largest entry that is not the marker, above 0.  One round
// per bit from mx's top bit down: the entries that share the bits found so far and have a 0 here are counted; the rank lies among them or
// behind them.  The marker has a 1 wherever a round looks, so it is never counted and stays behind every rank below `kmers`.
template <bool kLds>
__device__ __forceinline__ uint32_t select_rank(const uint32_t* lds, const uint32_t* dev, uint64_t n, uint32_t rank, uint32_t mx, uint32_t lane) {
  uint64_t prefix = 0;
  for (int bit = 31 - __builtin_clz(mx); bit >= 0; --bit) {                    // (at most 32 rounds)
    uint32_t zeros = 0;
    for (uint64_t i0 = 0; i0 < n; i0 += 64) {                                  // (wave-uniform)
      const uint64_t i = i0 + lane;
      const uint32_t v = i < n ? count_at<kLds>(lds, dev, i) : kMarker;
      const bool here = ((uint64_t)v >> (bit + 1)) == prefix && !((v >> bit) & 1u);
      zeros += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(here));
    }
    if (rank < zeros) prefix <<= 1;
    else { rank -= zeros; prefix = (prefix << 1) | 1u; }
  }
  return (uint32_t)prefix;
}

// N1.  long_counts: long_cap words for the reads with more than lds_windows (<= kNmC) windows, handed out through cu[kCuCursor]
template <bool kCanon>
__global__ __launch_bounds__(64 * kNmWaves) void nm_depth(RecInput a, RecInput b, uint64_t stride, uint64_t second, uint32_t paired, uint64_t reads, NmTable t,
                                                         uint32_t lds_windows, uint32_t* long_counts, uint64_t long_cap, unsigned long long* cu,
                                                         scfq_norm_rec* recs) {
  __shared__ uint64_t planes[kNmWaves][kCodeWords + kInvWords];
  __shared__ uint32_t cnt_sh[kNmWaves][kNmC];
  const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint64_t* const code = planes[wave];
  uint64_t* const inv = code + kCodeWords;
  uint32_t* const cnt = cnt_sh[wave];
  uint8_t* const code_bytes = reinterpret_cast<uint8_t*>(code);
  const uint32_t k = t.k;
  const uint64_t kbits = (1ull << k) - 1;                // (k <= 32)
  uint64_t absent = 0;
  for (uint64_t r0 = (uint64_t)blockIdx.x * kNmWaves; r0 < reads; r0 += (uint64_t)gridDim.x * kNmWaves) {
    const uint64_t r = r0 + wave;
    if (r >= reads) continue;                            // (wave-uniform)
    uint64_t ss, se;
    const RecInput& in = read_text(a, b, stride, second, paired, r, ss, se);
    const uint64_t len = se - ss, n_win = len >= k ? len - k + 1 : 0;
    const bool in_lds = n_win <= lds_windows;            // (wave-uniform; lds_windows <= kNmC)
    uint32_t* dev = nullptr;
    if (!in_lds) {
      unsigned long long at = 0;
      if (lane == 0) at = atomicAdd(&cu[kCuCursor], (unsigned long long)n_win);
      at = __shfl((unsigned long long)at, 0, 64);
      if (at + n_win > long_cap) {                       // (N0 counted the same reads by the same rule: this does not happen)
        if (lane == 0) { atomicAdd(&cu[kCuOverrun], 1ull); recs[r] = scfq_norm_rec{0, 0, 0, 0}; }
        continue;
      }
      dev = long_counts + at;
    }
    uint32_t kmers = 0, weak = 0, mn = kMarker, mx = 0;
    for (uint64_t c0 = 0; c0 + k <= len; c0 += kChunk) {      // the chunk has a window
      const uint32_t lc = (uint32_t)std::min<uint64_t>(len - c0, kChunk + k - 1), n_cw = lc - k + 1, rounds = (lc + 63) / 64;
      wave_lds_sync();                                   // the chunk before has been read
      for (uint32_t rd = 0; rd < rounds; ++rd) {
        const uint32_t pos = 64 * rd + lane;
        const uint32_t byte = pos < lc ? in.base[ss + c0 + pos] : 0u;
        const bool valid = byte == 'A' || byte == 'C' || byte == 'G' || byte == 'T';
        const uint64_t bad = __builtin_amdgcn_ballot_w64(!valid);
        if (lane == 0) inv[rd] = bad;
        // four bases a byte, the first one on top; byte y of the chunk is byte y ^ 7 of the little-endian words
        uint32_t v = valid ? ((((byte >> 1) & 3u) ^ ((byte >> 2) & 1u)) << (6 - 2 * (lane & 3u))) : 0u;
        v |= (uint32_t)__shfl_xor((int)v, 1, 64);
        v |= (uint32_t)__shfl_xor((int)v, 2, 64);
        if ((lane & 3u) == 0) code_bytes[(16 * rd + (lane >> 2)) ^ 7u] = (uint8_t)v;
      }
      wave_lds_sync();
      for (uint32_t q = lane; q < n_cw; q += 64) {
        // (q + k <= lc: every bit looked at below lies in a round that was written; what the funnel shifts pull in from the word
        // behind is cut off by kbits and by the shift down to 2k bits)
        const uint32_t o = q & 63u, w = q >> 6;
        const uint64_t ib = o ? (inv[w] >> o) | (inv[w + 1] << (64 - o)) : inv[w];
        uint32_t c = kMarker;
        if (!(ib & kbits)) {
          const uint32_t off = 2 * (q & 31u), j = q >> 5;
          const uint64_t hi = code[j], lo = code[j + 1];
          const uint64_t x = off ? (hi << off) | (lo >> (64 - off)) : hi;      // (never a shift by 64)
          uint64_t key = x >> (64 - 2 * k);
          if (kCanon) {
            const uint64_t rc = rev_comp(key, k);
            key = rc < key ? rc : key;
          }
          uint64_t found = 0;
          if (key == kEmpty) found = t.ones;             // (k = 32, plain mode: 32 T has no slot)
          else {
            uint64_t slot = mix64(key) & t.slot_mask;
            for (uint32_t p = 0; p < t.max_probe; ++p) {
              const ulonglong2 s = *reinterpret_cast<const ulonglong2*>(t.slots + slot);
              if (s.x == key) { found = s.y; break; }
              if (s.x == kEmpty) break;
              slot = (slot + 1) & t.slot_mask;
            }
          }
          c = found < SCFQ_NORM_MAX_DEPTH ? (uint32_t)found : SCFQ_NORM_MAX_DEPTH;
          ++kmers;
          weak += c < t.weak_below;
          absent += c == 0;
          mn = c < mn ? c : mn;
          mx = c > mx ? c : mx;
        }
        if (in_lds) cnt[c0 + q] = c;                     // (c0 + q < n_win <= lds_windows <= kNmC)
        else dev[c0 + q] = c;                            // (c0 + q < n_win: inside the read's piece)
      }
    }
    if (in_lds) wave_lds_sync();
    else { __threadfence(); __builtin_amdgcn_wave_barrier(); }
    const uint32_t n_kmers = (uint32_t)wave_sum(kmers), n_weak = (uint32_t)wave_sum(weak);
    const uint32_t lo_c = (uint32_t)wave_min(mn), hi_c = (uint32_t)wave_max(mx);
    uint32_t depth = 0;
    if (n_kmers && hi_c)
      depth = in_lds ? select_rank<true>(cnt, nullptr, n_win, (n_kmers - 1) / 2, hi_c, lane)
                     : select_rank<false>(nullptr, dev, n_win, (n_kmers - 1) / 2, hi_c, lane);
    if (lane == 0) recs[r] = scfq_norm_rec{n_kmers, depth, n_kmers ? lo_c : 0u, n_weak};
  }
  absent = wave_sum(absent);
  if (lane == 0 && absent) atomicAdd(&cu[kCuAbsent], (unsigned long long)absent);
}

// a unit: a single-end read, or a pair.  N2 and N3 both get it from here, so the lengths the scans saw are the lengths N3 writes
struct NmUnit {
  uint64_t len1, len2;                 // bytes for out1 and out2 (0 for a unit that is not written)
  uint64_t first;                      // of len1, mate 1's record (interleaved input: mate 2's follows it)
  uint32_t cls, depth;                 // the class (scfq_norm_host) and D
  bool kept;
};

__device__ __forceinline__ NmUnit look_up(const RecInput& a, const RecInput& b, uint64_t stride, uint64_t second, uint32_t paired, uint64_t u,
                                          const scfq_norm_rec* recs, const NmRule& rule) {
  NmUnit t = {};
  const scfq_norm_rec r1 = recs[paired ? 2 * u : u];
  const scfq_norm_rec r2 = paired ? recs[2 * u + 1] : scfq_norm_rec{0, 0, 0, 0};
  t.cls = classify(r1.kmers, r1.depth, r2.kmers, r2.depth, u, rule.target, rule.min_depth, rule.seed, &t.depth);
  t.kept = t.cls == kKept || (t.cls == kNoKmers && rule.keep_no_kmers);
  if (!t.kept) return t;
  t.first = echo_len(a, paired ? u * stride : u);
  const uint64_t m2 = paired ? echo_len(b, u * stride + second) : 0;
  t.len1 = t.first + (second ? m2 : 0);
  t.len2 = second ? 0 : m2;
  return t;
}

// the counters of N2
enum { kOut = 0, kDropNoKmers, kDropLow, kDropHigh, kShort, kBasesIn, kBasesOut, kWindows, kKmers, kWeak, kCounters };

// N2.  group_len: two arrays of n_groups + 1 entries, one after the other (the last entry of each stays 0: the scan's total).
// hist: nullptr, or 2 * bins words: [2d] units with D = d, [2d + 1] the kept ones among them; the last bin gathers D >= bins - 1
__global__ __launch_bounds__(256) void nm_decide(RecInput a, RecInput b, uint64_t stride, uint64_t second, uint32_t paired, uint64_t units,
                                                const scfq_norm_rec* recs, NmRule rule, uint32_t k, uint64_t n_groups, uint64_t* group_len,
                                                unsigned long long* hist, uint64_t bins, unsigned long long* counters) {
  __shared__ unsigned long long sum_sh[kCounters];
  __shared__ uint32_t hist_sh[2 * kNmHistLds];           // (a block sees fewer than 2^32 units)
  const uint32_t in_lds = hist ? (uint32_t)(bins < kNmHistLds ? bins : kNmHistLds) : 0u;
  if (threadIdx.x < kCounters) sum_sh[threadIdx.x] = 0;
  for (uint32_t x = threadIdx.x; x < 2 * in_lds; x += 256) hist_sh[x] = 0;
  __syncthreads();
  uint64_t c[kCounters];
#pragma unroll
  for (int x = 0; x < kCounters; ++x) c[x] = 0;
  const uint32_t mates = paired ? 2u : 1u;
  for (uint64_t u0 = (uint64_t)blockIdx.x * 256; u0 < units; u0 += (uint64_t)gridDim.x * 256) {      // (block-uniform)
    const uint64_t u = u0 + threadIdx.x;
    const bool live = u < units;
    uint64_t len[2] = {0, 0};
    if (live) {
      const NmUnit t = look_up(a, b, stride, second, paired, u, recs, rule);
      len[0] = t.len1; len[1] = t.len2;
      c[kOut] += t.kept;
      c[kDropNoKmers] += !t.kept && t.cls == kNoKmers;
      c[kDropLow] += t.cls == kLow;
      c[kDropHigh] += t.cls == kHigh;
#pragma unroll
      for (uint32_t m = 0; m < 2; ++m) {
        if (m >= mates) continue;
        const scfq_norm_rec rec = recs[paired ? 2 * u + m : u];
        uint64_t s, e;
        text_span(m ? b : a, 4 * (paired ? u * stride + (m ? second : 0) : u) + 1, s, e);
        const uint64_t L = e - s;
        c[kShort] += L < k;
        c[kBasesIn] += L;
        c[kBasesOut] += t.kept ? L : 0;
        c[kWindows] += L >= k ? L - k + 1 : 0;
        c[kKmers] += rec.kmers;
        c[kWeak] += rec.weak;
      }
      if (hist && t.cls != kNoKmers) {
        const uint64_t bin = t.depth < bins - 1 ? t.depth : bins - 1;
        if (bin < in_lds) {
          atomicAdd(&hist_sh[2 * bin], 1u);
          if (t.kept) atomicAdd(&hist_sh[2 * bin + 1], 1u);
        } else {
          atomicAdd(&hist[2 * bin], 1ull);
          if (t.kept) atomicAdd(&hist[2 * bin + 1], 1ull);
        }
      }
    }
#pragma unroll
    for (int x = 0; x < 2; ++x) store_group_len(len[x], x, u, units, n_groups, group_len);
  }
  // the statistics: a sum per wave into LDS, then ONE atomic per block and counter
  const bool first_lane = (threadIdx.x & 63) == 0;
#pragma unroll
  for (int x = 0; x < kCounters; ++x) {
    const uint64_t s = wave_sum(c[x]);
    if (first_lane && s) atomicAdd(&sum_sh[x], (unsigned long long)s);
  }
  __syncthreads();
  if (threadIdx.x < kCounters && sum_sh[threadIdx.x]) atomicAdd(&counters[threadIdx.x], sum_sh[threadIdx.x]);
  for (uint32_t x = threadIdx.x; x < 2 * in_lds; x += 256)
    if (hist_sh[x]) atomicAdd(&hist[x], (unsigned long long)hist_sh[x]);
}

// N3.  group_off: the two scanned arrays of N2's layout
__global__ __launch_bounds__(64 * kNmWaves) void nm_write(RecInput a, RecInput b, uint64_t stride, uint64_t second, uint32_t paired, uint64_t units,
                                                         const scfq_norm_rec* recs, NmRule rule, uint64_t n_groups, const uint64_t* group_off, RecOut o1,
                                                         RecOut o2) {
  const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // (when one result is more than its output holds, nothing is written to either)
  if (!(output_fits(o1, 0, n_groups, group_off) && output_fits(o2, 1, n_groups, group_off))) return;
  const uint64_t g = (uint64_t)blockIdx.x * kNmWaves + wave;
  if (g >= n_groups) return;
  const uint64_t u0 = g * kNmGroup;
  const uint32_t count = (uint32_t)std::min<uint64_t>(kNmGroup, units - u0);
  NmUnit mine = {};
  if (lane < count) mine = look_up(a, b, stride, second, paired, u0 + lane, recs, rule);
  const uint64_t len[2] = {mine.len1, mine.len2};
  uint64_t at[2];
  place_units(len, g, n_groups, group_off, lane, at);
  for (uint32_t q = 0; q < count; ++q) {
    const uint64_t l1 = bcast(mine.len1, q), l2 = bcast(mine.len2, q), first = bcast(mine.first, q), w1 = bcast(at[0], q), w2 = bcast(at[1], q);
    if (l1 + l2 == 0) continue;                            // (a unit that is not written, or the echo of nothing)
    const uint64_t u = u0 + q;
    const uint64_t i1 = paired ? u * stride : u, i2 = u * stride + second;
    if (o1.p && first) echo_record(a, i1, o1.p + w1, first, lane);
    if (paired) {
      if (second) { if (o1.p && l1 > first) echo_record(b, i2, o1.p + w1 + first, l1 - first, lane); }
      else if (o2.p && l2) echo_record(b, i2, o2.p + w2, l2, lane);
    }
  }
}

uint32_t lds_windows_env() {
  static const uint32_t v = [] {
    const uint32_t e = scfq_kcount_host::env_u32("SCFQ_NORM_LDS_WINDOWS");
    return e ? std::min(std::max(e, kNmMinC), kNmC) : kNmC;
  }();
  return v;
}

// K5 of the inputs and what follows from their line counts, into st; the per-read table's size is checked here, before anything is
// counted or written
int index_and_check(const uint8_t* d1, uint64_t n1, const uint8_t* d2, uint64_t n2, Mode mode, const Params& prm, bool check_rec_cap, uint64_t rec_cap,
                    scfq_overlap::Indexed& ix, scfq_norm_stats* st, hipStream_t stream) {
  for (double& m : g_stage_ms) m = 0;
  st->input_bytes1 = n1;
  st->input_bytes2 = n2;
  st->flags = prm.flags; st->target = prm.target; st->min_depth = prm.min_depth; st->weak_below = prm.weak_below; st->seed = prm.seed;
  const auto t_a = std::chrono::steady_clock::now();
  const int rc = scfq_reads::index_units(d1, n1, d2, n2, mode, stream, g_nerr, ix, &g_stage_ms[0], st, &st->units_in, &st->reads_in);
  // (index_units takes the time of paired input only; this pipeline reports the one index of single-end input as well)
  if (mode == Mode::single) g_stage_ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_a).count();
  if (rc) return rc;
  if (check_rec_cap && rec_cap < st->reads_in) {
    std::snprintf(g_nerr, sizeof g_nerr, "the per-read table holds %llu entries, the input has %llu reads", (unsigned long long)rec_cap,
                  (unsigned long long)st->reads_in);
    return SCFQ_EARG;
  }
  return SCFQ_OK;
}

// the two-pass form: the resident inputs, with the line indexes they already have, into a table of their own
int count_inputs(const uint8_t* d1, uint64_t n1, const uint8_t* d2, uint64_t n2, Mode mode, const Params& prm, const scfq_overlap::Indexed& ix,
                 scfq_kcount** table, hipStream_t stream) {
  scfq_kcount_internal::Resident in[2];
  in[0].d = d1; in[0].n = n1; in[0].line_off = static_cast<const uint64_t*>(ix.off1.p); in[0].lines = ix.lines1; in[0].has_cr = ix.cr1;
  in[1].d = d2; in[1].n = n2; in[1].line_off = static_cast<const uint64_t*>(ix.off2.p); in[1].lines = ix.lines2; in[1].has_cr = ix.cr2;
  scfq_kcount_opts ko;
  ko.struct_size = sizeof ko; ko.k = prm.k; ko.flags = prm.table_flags; ko.table_bits = prm.table_bits; ko.reserved = 0;
  const int rc = scfq_kcount_internal::count_resident(in, mode == Mode::two ? 2 : 1, ko, table, nullptr, stream);
  if (rc) std::snprintf(g_nerr, sizeof g_nerr, "counting the inputs: %s", scfq_kcount_error_detail());
  return rc;
}

// recs_out: the caller's per-read table (device memory), or nullptr; recs_keep: where the table stays for the caller of this function
// to copy it (the file entry point)
int norm_device(const scfq_kcount_internal::View& tv, const uint8_t* d1, uint64_t n1, const uint8_t* d2, uint64_t n2, Mode mode, const Params& prm,
                const scfq_overlap::Indexed& ix, scfq_norm_rec* recs_out, DevBuf& recs_keep, bool own_outputs, Dest dst[2], DevBuf own[2], bool check_caps,
                uint64_t* hist_host, uint64_t bins, scfq_norm_stats* st, hipStream_t stream) {
  const bool paired = mode != Mode::single, interleaved = mode == Mode::interleaved;
  st->k = tv.k; st->table_flags = tv.flags; st->distinct = tv.distinct; st->slots = tv.n_slots; st->passes = tv.passes;
  const uint64_t units = st->units_in, reads = st->reads_in;
  if (hist_host) std::memset(hist_host, 0, 2 * bins * 8);
  if (units == 0) return SCFQ_OK;           // (two empty outputs: they fit into anything)
  const uint64_t n_groups = (units + kNmGroup - 1) / kNmGroup;
  const size_t hist_bytes = hist_host ? 2 * bins * 8 : 0;
  int rc = SCFQ_OK;
  DevBuf group_len, group_off, counters, cursors, tmp, hist, long_counts;
  scfq_reads::GroupScan gs(2, n_groups, group_len, group_off, stream, g_nerr);
  if ((!recs_out && (rc = recs_keep.alloc(reads * sizeof(scfq_norm_rec), stream, g_nerr))) || (rc = gs.alloc()) ||
      (rc = counters.alloc(kCounters * 8, stream, g_nerr)) ||
      (rc = cursors.alloc(kCuWords * 8, stream, g_nerr)) || (hist_bytes && (rc = hist.alloc(hist_bytes, stream, g_nerr))))
    return rc;
  scfq_norm_rec* const recs = recs_out ? recs_out : recs_keep.as<scfq_norm_rec>();
  size_t scan_bytes = 0;
  if ((rc = gs.scratch_bytes(&scan_bytes)) || (rc = tmp.alloc(scan_bytes, stream, g_nerr))) return rc;
  static const bool timing = scfq_scratch::env_switch("SCFQ_NORM_TIMING");
  const uint32_t lds_windows = lds_windows_env();
  SCFQ_SCRATCH_CHK(g_nerr, hipMemsetAsync(counters.p, 0, kCounters * 8, stream));
  SCFQ_SCRATCH_CHK(g_nerr, hipMemsetAsync(cursors.p, 0, kCuWords * 8, stream));
  if ((rc = gs.zero())) return rc;
  if (hist_bytes) SCFQ_SCRATCH_CHK(g_nerr, hipMemsetAsync(hist.p, 0, hist_bytes, stream));
  const RecInput a = {d1, n1, static_cast<const uint64_t*>(ix.off1.p), ix.lines1, ix.cr1};
  const RecInput b = mode == Mode::two ? RecInput{d2, n2, static_cast<const uint64_t*>(ix.off2.p), ix.lines2, ix.cr2} : a;
  const uint64_t stride = interleaved ? 2 : 1, second = interleaved ? 1 : 0;
  const NmRule rule = {prm.target, prm.min_depth, (prm.flags & SCFQ_NORM_KEEP_NO_KMERS) ? 1u : 0u, prm.seed};
  const NmTable table = {static_cast<const KcSlot*>(tv.slots), tv.n_slots - 1, tv.ones, tv.max_probe, tv.k, prm.weak_below};
  unsigned long long* const cu = cursors.as<unsigned long long>();
  // N0, and the device array of the long reads' counts: allocated here, with the call's other buffers
  hipLaunchKernelGGL(nm_long_windows, dim3((unsigned)std::min<uint64_t>((reads + 255) / 256, 1024)), dim3(256), 0, stream, a, b, stride, second, paired ? 1u : 0u,
                     reads, tv.k, lds_windows, cu);
  SCFQ_SCRATCH_CHK(g_nerr, hipGetLastError());
  uint64_t hcu[kCuWords];
  SCFQ_SCRATCH_CHK(g_nerr, hipMemcpyAsync(hcu, cursors.p, sizeof hcu, hipMemcpyDeviceToHost, stream));
  SCFQ_SCRATCH_CHK(g_nerr, hipStreamSynchronize(stream));
  const uint64_t long_cap = hcu[kCuLongWindows];
  if (long_cap && (rc = long_counts.alloc(long_cap * 4, stream, g_nerr))) return rc;
  scfq_scratch::StageClock clk(stream, timing);
  clk.mark(0);
  const dim3 grid1((unsigned)std::min<uint64_t>((reads + kNmWaves - 1) / kNmWaves, kNmMaxBlocks));
  if (tv.flags & SCFQ_KCOUNT_CANONICAL)
    hipLaunchKernelGGL(nm_depth<true>, grid1, dim3(64 * kNmWaves), 0, stream, a, b, stride, second, paired ? 1u : 0u, reads, table, lds_windows,
                       long_counts.as<uint32_t>(), long_cap, cu, recs);
  else
    hipLaunchKernelGGL(nm_depth<false>, grid1, dim3(64 * kNmWaves), 0, stream, a, b, stride, second, paired ? 1u : 0u, reads, table, lds_windows,
                       long_counts.as<uint32_t>(), long_cap, cu, recs);
  SCFQ_SCRATCH_CHK(g_nerr, hipGetLastError());
  clk.mark(1);
  hipLaunchKernelGGL(nm_decide, dim3((unsigned)std::min<uint64_t>((units + 255) / 256, kNmDecideBlocks)), dim3(256), 0, stream, a, b, stride, second,
                     paired ? 1u : 0u, units, recs, rule, tv.k, n_groups, gs.len(), hist.as<unsigned long long>(), bins,
                     counters.as<unsigned long long>());
  SCFQ_SCRATCH_CHK(g_nerr, hipGetLastError());
  if ((rc = gs.scan(tmp.p, scan_bytes))) return rc;
  clk.mark(2);
  // the sizes and the statistics come back first: pool memory for the outputs is taken to fit, and a caller's buffer that is too small
  // is known here
  uint64_t h[kCounters];
  if ((rc = gs.read_totals())) return rc;
  SCFQ_SCRATCH_CHK(g_nerr, hipMemcpyAsync(h, counters.p, sizeof h, hipMemcpyDeviceToHost, stream));
  SCFQ_SCRATCH_CHK(g_nerr, hipMemcpyAsync(hcu, cursors.p, sizeof hcu, hipMemcpyDeviceToHost, stream));
  SCFQ_SCRATCH_CHK(g_nerr, hipStreamSynchronize(stream));
  if (hist_bytes) SCFQ_SCRATCH_CHK(g_nerr, hipMemcpy(hist_host, hist.p, hist_bytes, hipMemcpyDeviceToHost));
  if (hcu[kCuOverrun] || hcu[kCuCursor] != long_cap) {
    std::snprintf(g_nerr, sizeof g_nerr, "N1 took %llu words for its long reads, N0 counted %llu", (unsigned long long)hcu[kCuCursor], (unsigned long long)long_cap);
    return SCFQ_EHIP;
  }
  st->out1_bytes = gs.total[0]; st->out2_bytes = gs.total[1];
  st->units_out = h[kOut]; st->reads_out = h[kOut] * (paired ? 2 : 1);
  st->dropped_no_kmers = h[kDropNoKmers]; st->dropped_low = h[kDropLow]; st->dropped_high = h[kDropHigh];
  st->short_reads = h[kShort]; st->bases_in = h[kBasesIn]; st->bases_out = h[kBasesOut];
  st->windows = h[kWindows]; st->kmers = h[kKmers]; st->skipped = h[kWindows] - h[kKmers];
  st->weak_kmers = h[kWeak]; st->absent_kmers = hcu[kCuAbsent];
  const scfq_reads::Placement put = scfq_reads::place_outputs(gs, scfq_reads::kOutNames, dst, own_outputs, check_caps, false, own, stream, g_nerr);
  if (put.rc) return put.rc;
  if (put.out[0].p || put.out[1].p) {
    hipLaunchKernelGGL(nm_write, dim3((unsigned)((n_groups + kNmWaves - 1) / kNmWaves)), dim3(64 * kNmWaves), 0, stream, a, b, stride, second, paired ? 1u : 0u,
                       units, recs, rule, n_groups, gs.off(), put.out[0], put.out[1]);
    SCFQ_SCRATCH_CHK(g_nerr, hipGetLastError());
  }
  clk.mark(3);
  SCFQ_SCRATCH_CHK(g_nerr, hipStreamSynchronize(stream));
  g_stage_ms[1] = clk.between(0, 1);
  g_stage_ms[2] = clk.between(1, 2);
  g_stage_ms[3] = clk.between(2, 3);
  return put.verdict;      // (SCFQ_EARG for an output that is too small: place_outputs has left the text)
}

struct OwnTable {          // the table of the two-pass form
  scfq_kcount* t = nullptr;
  ~OwnTable() { scfq_kcount_free(t); }
};

int check(const scfq_kcount* table, const scfq_norm_opts* opts, const scfq_norm_stats* stats, bool first, bool second, bool out2, bool have_hist, uint64_t bins,
          Params& prm) {
  scfq_kcount_internal::View tv;
  const bool have = scfq_kcount_internal::view(table, &tv);
  return check_args(opts, stats, have, tv.k, first, second, out2, have_hist, bins, prm, g_nerr, sizeof g_nerr);
}

}  // namespace

extern "C" {

const char* scfq_norm_error_detail(void) { return g_nerr; }

int scfq_debug_norm_stages(double* ms, uint32_t cap) { return scfq_scratch::copy_stage_ms(g_stage_ms, ms, cap); }

int scfq_format_norm_row_tsv(const scfq_norm_stats* s, int header, char* buf, uint64_t cap) { return format_row(s, header, buf, cap); }

int scfq_format_norm_hist_tsv(uint64_t depth, uint64_t units_in, uint64_t units_out, char* buf, uint64_t cap) {
  return format_hist(depth, units_in, units_out, buf, cap);
}

int scfq_norm_buffers(const scfq_kcount* table, const void* r1, uint64_t n1, const void* r2, uint64_t n2, int is_device, const scfq_norm_opts* opts,
                      scfq_norm_rec* recs_device, uint64_t rec_cap, void* out1, uint64_t cap1, void* out2, uint64_t cap2, int out_is_device,
                      uint64_t* hist_host, uint64_t bins, scfq_norm_stats* stats) {
  g_nerr[0] = '\0';
  Params prm;
  int rc = check(table, opts, stats, r1 != nullptr, r2 != nullptr, out2 != nullptr, hist_host != nullptr, bins, prm);
  if (rc) return rc;
  if ((!r1 && n1) || (!r2 && n2) || (!out1 && cap1) || (!out2 && cap2) || (!recs_device && rec_cap)) {
    std::snprintf(g_nerr, sizeof g_nerr, "a NULL pointer with a size above 0");
    return SCFQ_EARG;
  }
  const bool interleaved = (prm.flags & SCFQ_NORM_INTERLEAVED) != 0;
  const Mode mode = interleaved ? Mode::interleaved : (r2 ? Mode::two : Mode::single);
  scfq_scratch::clear_keep_size(stats);
  Dest dst[2] = {{static_cast<uint8_t*>(out1), cap1, out1 != nullptr}, {static_cast<uint8_t*>(out2), cap2, out2 != nullptr}};
  const bool any_out = out1 || out2, direct = any_out && out_is_device;
  scfq_scratch::ResidentInput in1, in2;
  rc = in1.from_buffer(r1, n1, is_device != 0, is_device || direct || recs_device, g_nerr);
  if (rc) return rc;
  if (mode == Mode::two && (rc = in2.from_buffer(r2, n2, is_device != 0, false, g_nerr))) return rc;
  scfq_overlap::Indexed ix;
  if ((rc = index_and_check(in1.d_in, in1.n, in2.d_in, in2.n, mode, prm, recs_device != nullptr, rec_cap, ix, stats, in1.stream))) return finish(in1, rc);
  OwnTable mine;
  if (!table) {
    if ((rc = count_inputs(in1.d_in, in1.n, in2.d_in, in2.n, mode, prm, ix, &mine.t, in1.stream))) return finish(in1, rc);
    table = mine.t;
  }
  scfq_kcount_internal::View tv;
  scfq_kcount_internal::view(table, &tv);
  DevBuf own[2], recs_keep;
  rc = norm_device(tv, in1.d_in, in1.n, in2.d_in, in2.n, mode, prm, ix, recs_device, recs_keep, /*own_outputs=*/!direct, dst, own, /*check_caps=*/true, hist_host,
                   bins, stats, in1.stream);
  if (rc) return finish(in1, rc);
  if (!direct) {
    const uint64_t bytes[2] = {stats->out1_bytes, stats->out2_bytes};
    if ((rc = scfq_reads::outputs_to_host(2, dst, own, bytes, in1.stream, g_nerr))) return rc;
    SCFQ_SCRATCH_CHK(g_nerr, hipStreamSynchronize(in1.stream));
  }
  for (DevBuf& o : own) o.drop();
  recs_keep.drop();
  ix.off1.drop();
  ix.off2.drop();
  in1.mark_clean();      // (the last act was to wait for the stream; behind it lie returns of pool memory only)
  return SCFQ_OK;
}

int scfq_norm_files(const scfq_kcount* table, const char* path1, const char* path2, const scfq_opts* opts, const scfq_norm_opts* nopts, int out1_fd, int out2_fd,
                    scfq_norm_rec* recs_host, uint64_t rec_cap, uint64_t* hist_host, uint64_t bins, scfq_norm_stats* stats) {
  g_nerr[0] = '\0';
  Params prm;
  int rc = check(table, nopts, stats, path1 != nullptr, path2 != nullptr, out2_fd >= 0, hist_host != nullptr, bins, prm);
  if (rc) return rc;
  if (!path1) { std::snprintf(g_nerr, sizeof g_nerr, "path1 is NULL"); return SCFQ_EARG; }
  if (!recs_host && rec_cap) { std::snprintf(g_nerr, sizeof g_nerr, "a NULL pointer with a size above 0"); return SCFQ_EARG; }
  const bool interleaved = (prm.flags & SCFQ_NORM_INTERLEAVED) != 0;
  const Mode mode = interleaved ? Mode::interleaved : (path2 ? Mode::two : Mode::single);
  scfq_scratch::clear_keep_size(stats);
  scfq_scratch::ResidentInput in1, in2;
  rc = in1.from_file(path1, opts, g_nerr);
  if (rc) return rc;
  if (mode == Mode::two && (rc = in2.from_file(path2, opts, g_nerr))) return rc;      // (staged when this returns)
  // every buffer of the call is pool memory taken below, before either staged file goes back; the table of the two-pass form is the one
  // hipMalloc, and it is freed before them as well (OwnTable is destroyed first)
  scfq_overlap::Indexed ix;
  if ((rc = index_and_check(in1.d_in, in1.n, in2.d_in, in2.n, mode, prm, recs_host != nullptr, rec_cap, ix, stats, in1.stream))) return finish(in1, rc);
  OwnTable mine;
  if (!table) {
    if ((rc = count_inputs(in1.d_in, in1.n, in2.d_in, in2.n, mode, prm, ix, &mine.t, in1.stream))) return finish(in1, rc);
    table = mine.t;
  }
  scfq_kcount_internal::View tv;
  scfq_kcount_internal::view(table, &tv);
  const int fd[2] = {out1_fd, out2_fd};
  Dest dst[2] = {{nullptr, 0, out1_fd >= 0}, {nullptr, 0, out2_fd >= 0}};
  DevBuf own[2], recs_keep;
  rc = norm_device(tv, in1.d_in, in1.n, in2.d_in, in2.n, mode, prm, ix, nullptr, recs_keep, /*own_outputs=*/true, dst, own, /*check_caps=*/false, hist_host, bins,
                   stats, in1.stream);
  if (rc) return finish(in1, rc);
  if (recs_host && stats->reads_in) {
    SCFQ_SCRATCH_CHK(g_nerr, hipMemcpyAsync(recs_host, recs_keep.p, stats->reads_in * sizeof(scfq_norm_rec), hipMemcpyDeviceToHost, in1.stream));
    SCFQ_SCRATCH_CHK(g_nerr, hipStreamSynchronize(in1.stream));
  }
  const uint64_t bytes[2] = {stats->out1_bytes, stats->out2_bytes};
  return scfq_reads::outputs_to_fds(2, own, bytes, fd, in1, g_nerr);
}

}  // extern "C"

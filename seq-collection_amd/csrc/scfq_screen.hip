// scfq_screen.hip — `sc fq-screen` on the MI355X (gfx950): which reads share k-mers with a set of references, and the reads that do not.
// Not in the reference; definitions in include/sc_fqcount.h.
//
// The index (once per set of references):
//   S0  parse_references      host (scfq_screen_host.hpp): the references as one upper-cased byte string, a separator behind every contig
//   S1  sc_build              a thread per run of kRun window starts rolls the forward and the reverse-complement word along its bytes and
//                             inserts min(fwd, rc): a 64-bit compare-and-swap on the key array with linear probing, then an atomic OR of
//                             the reference's bit into the slot's mask word; the key's prefilter bit is set on the way
//       sc_count_slots        distinct / shared per reference, over the slots
// A call, the inputs in HBM whole (one FASTQ, two, or one interleaved):
//   K5  line index            (scfq_scratch::build_line_index) of each input
//   S2  sc_lookup             the hot path: a wave per read, kScWaves waves per block, persistent blocks that stride over the reads and
//                             hold the prefilter bitmap in LDS.  The read goes through LDS in chunks of 512 window starts (512 + k - 1
//                             bases): 2 bits per base, 32 bases per 64-bit word with the first base on top, and a plane with a bit per
//                             base that is not exactly A C G T.  Lane l takes the windows l, l + 64, ... of the chunk: a funnel shift of
//                             two words is the forward index, complement + byte swap + two swap steps the reverse complement, one masked
//                             test of the invalid plane rejects the window.  A key whose prefilter bit is clear is in no reference; any
//                             other one is looked for by linear probing, the mask word loaded on a key hit only, and the hits counted per
//                             reference in LDS.  Lane 0 stores 16 bytes per read.
//   S3  sc_lengths            a thread per read (single-end) or pair: kept or not, the bytes it adds to each output summed per group of
//                             kScGroup, and the statistics, one atomic per block and counter
//       exclusive scans       one per output over the groups (rocprim), each with a last entry that is the output's size
//   S4  sc_write              a wave per group echoes the kept records, each one wave_copy where the echo is the record's own bytes
// The empty key is all ones.  No canonical key equals it: the only index of all ones is that of k = 32 times 'T', whose reverse
// complement is 32 times 'A' with the index 0, and the key is the minimum of the two.
// Every probe loop, in S1 and in S2, makes at most `slots` steps, and the host makes the table larger than the number of windows, so
// that an empty slot always exists: a table that cannot hold the keys is refused before any launch (pick_slots) and, should an insert
// run out of steps all the same, S1 raises a flag that fails the build.  There is no CPU fallback.
#include "../../include/sc_fqcount.h"
#include "../../include/sc_fqcount_debug.h"

#include <cstring>        // (rocprim's texture iterator calls memset from host code)
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "scfq_reads_host.hpp"
#include "scfq_screen_host.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

static_assert(sizeof(scfq_screen_rec) == 16 && sizeof(scfq_screen_stats) == 94 * 8 && sizeof(scfq_screen_summary) == (6 + 16 * 6) * 8, "the ABI's sizes");
static_assert(scfq_screen_host::kErrBytes == scfq_scratch::kErrBytes, "one error buffer for both");

// the index: the table on the device, everything else on the host
struct scfq_screen_index {
  int dev = -1;
  uint32_t k = 0;
  uint64_t slots = 0, distinct = 0;
  uint64_t* d_keys = nullptr;
  uint32_t* d_masks = nullptr;
  uint32_t* d_filter = nullptr;      // nullptr: no prefilter
  uint32_t filter_bits = 0;          // bits of the bitmap, a power of two
  double build_ms = 0;               // S1, by HIP events
  std::vector<scfq_screen_host::RefInfo> refs;
  ~scfq_screen_index() {
    if (d_keys) (void)hipFree(d_keys);
    if (d_masks) (void)hipFree(d_masks);
    if (d_filter) (void)hipFree(d_filter);
  }
};

namespace {

thread_local char g_serr[scfq_scratch::kErrBytes] = "";
thread_local double g_stage_ms[4] = {0, 0, 0, 0};

using scfq_reads::Dest;
using scfq_reads::DevBuf;
using scfq_reads::finish;
using scfq_reads::Mode;

constexpr uint64_t kEmpty = ~0ull;
constexpr uint32_t kRun = 64;                            // window starts of a thread of S1
constexpr uint32_t kScWaves = 4;                         // reads a block of S2 works on at a time; groups of a block of S4
constexpr uint32_t kScMaxBlocks = 2048;                  // of S2
constexpr uint32_t kScGroup = kRecGroup;                 // reads or pairs of a group: one wave of S4, one entry of the scans
constexpr uint32_t kChunk = 512;                         // window starts of a chunk of S2
constexpr uint32_t kCodeWords = 18, kInvWords = 10;      // 64-bit words of a wave's two planes: 9 rounds of 64 bases, and the word behind
constexpr uint32_t kWaveLds = (kCodeWords + kInvWords) * 8 + SCFQ_SCREEN_MAX_REFS * 4;      // bytes of LDS of a wave of S2
static_assert(kChunk + SCFQ_SCREEN_MAX_K - 1 <= 9 * 64, "a chunk's bases are nine rounds of the wave");

__host__ __device__ __forceinline__ uint64_t mix64(uint64_t x) {      // (MurmurHash3's finalizer)
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}
// the slot a key starts at: the low bits; the prefilter's bit: bits 40 and up (a table has at most 2^30 slots, a bitmap 2^19 bits)
__device__ __forceinline__ uint32_t filter_bit(uint64_t h, uint32_t filter_bits) { return (uint32_t)(h >> 40) & (filter_bits - 1u); }

struct ScRefs { uint64_t begin[SCFQ_SCREEN_MAX_REFS + 1]; };

// S1.  text: S0's string of n bytes; kmask: the low 2k bits
__global__ __launch_bounds__(256) void sc_build(const uint8_t* text, uint64_t n, ScRefs refs, uint32_t k, uint64_t kmask, unsigned long long* keys,
                                               uint32_t* masks, uint64_t slots, uint32_t* filter, uint32_t filter_bits, uint32_t* failed) {
  const uint64_t p0 = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * kRun;
  if (p0 >= n) return;
  const uint64_t end = std::min<uint64_t>(n, p0 + kRun + k - 1);      // the window that starts at p0 + kRun - 1 ends here
  uint32_t r = 0, run = 0;
  uint64_t fwd = 0, rc = 0;
  for (uint64_t i = p0; i < end; ++i) {
    const uint32_t b = text[i];
    while (i >= refs.begin[r + 1]) ++r;                  // (i < n = begin[n_refs])
    if (b != 'A' && b != 'C' && b != 'G' && b != 'T') { run = 0; continue; }
    const uint64_t c = ((b >> 1) & 3u) ^ ((b >> 2) & 1u);      // A C G T -> 0 1 2 3
    fwd = ((fwd << 2) | c) & kmask;
    rc = (rc >> 2) | ((3u - c) << (2 * (k - 1)));
    if (++run < k) continue;
    // the window [i - k + 1, i]: it starts in [p0, p0 + kRun) and nowhere else
    const uint64_t key = fwd < rc ? fwd : rc, h = mix64(key);
    uint64_t slot = h & (slots - 1);
    bool done = false;
    for (uint64_t step = 0; step < slots; ++step) {
      unsigned long long cur = __atomic_load_n(&keys[slot], __ATOMIC_RELAXED);      // (a slot that holds a key keeps it)
      if (cur == kEmpty) cur = atomicCAS(&keys[slot], (unsigned long long)kEmpty, (unsigned long long)key);
      if (cur == kEmpty || cur == key) {
        atomicOr(&masks[slot], 1u << r);
        done = true;
        break;
      }
      slot = (slot + 1) & (slots - 1);
    }
    if (!done) atomicOr(failed, 1u);
    if (filter) {
      const uint32_t fb = filter_bit(h, filter_bits);
      atomicOr(&filter[fb >> 5], 1u << (fb & 31u));
    }
  }
}

// counts[r]: slots with bit r; counts[16 + r]: with bit r and another one; counts[32]: slots with a key
__global__ __launch_bounds__(256) void sc_count_slots(const unsigned long long* keys, const uint32_t* masks, uint64_t slots, unsigned long long* counts) {
  __shared__ unsigned long long c_sh[2 * SCFQ_SCREEN_MAX_REFS + 1];
  if (threadIdx.x < 2 * SCFQ_SCREEN_MAX_REFS + 1) c_sh[threadIdx.x] = 0;
  __syncthreads();
  for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * 256) {
    if (keys[s] == kEmpty) continue;
    const uint32_t m = masks[s];
    const bool several = (m & (m - 1)) != 0;
    atomicAdd(&c_sh[2 * SCFQ_SCREEN_MAX_REFS], 1ull);
    for (uint32_t rest = m; rest; rest &= rest - 1) {
      const uint32_t r = (uint32_t)__builtin_ctz(rest);
      atomicAdd(&c_sh[r], 1ull);
      if (several) atomicAdd(&c_sh[SCFQ_SCREEN_MAX_REFS + r], 1ull);
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 * SCFQ_SCREEN_MAX_REFS + 1 && c_sh[threadIdx.x]) atomicAdd(&counts[threadIdx.x], c_sh[threadIdx.x]);
}

struct ScTable {          // the index as S2 sees it
  const unsigned long long* keys;
  const uint32_t* masks;
  uint64_t slots;
  const uint32_t* filter;      // nullptr: none
  uint32_t filter_bits;
  uint32_t k;
  uint32_t min_hits, min_hit_pct;
};

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
  return r >> (64 - 2 * k);                              // (k >= 8: a shift of 0 .. 48)
}

// S2.  Read r is record r of `a` (single-end: paired = 0) or mate r & 1 of pair r >> 1: record p * stride of a, record p * stride + second
// of b.  Dynamic LDS: the bitmap (t.filter_bits / 8 bytes, or nothing), then kWaveLds bytes per wave.
__global__ __launch_bounds__(64 * kScWaves) void sc_lookup(RecInput a, RecInput b, uint64_t stride, uint64_t second, uint32_t paired, uint64_t reads, ScTable t,
                                                          scfq_screen_rec* recs, unsigned long long* ref_hits) {
  extern __shared__ uint64_t lds64[];
  const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t filter_words = t.filter ? t.filter_bits / 32 : 0;
  uint32_t* const flt = reinterpret_cast<uint32_t*>(lds64);
  uint64_t* const code = lds64 + filter_words / 2 + (uint64_t)wave * (kWaveLds / 8);
  uint64_t* const inv = code + kCodeWords;
  uint32_t* const hits = reinterpret_cast<uint32_t*>(inv + kInvWords);
  uint8_t* const code_bytes = reinterpret_cast<uint8_t*>(code);
  for (uint32_t w = threadIdx.x; w < filter_words; w += 64 * kScWaves) flt[w] = t.filter[w];
  __syncthreads();                                       // (the only block-wide wait: from here the waves go their own ways)
  const uint32_t k = t.k;
  const uint64_t kbits = (1ull << k) - 1;                // (k <= 32)
  for (uint64_t r0 = (uint64_t)blockIdx.x * kScWaves; r0 < reads; r0 += (uint64_t)gridDim.x * kScWaves) {
    const uint64_t r = r0 + wave;
    if (r >= reads) continue;
    const uint64_t p = paired ? r >> 1 : r;
    const bool mate2 = paired && (r & 1);
    const RecInput& in = mate2 ? b : a;
    const uint64_t i = paired ? p * stride + (mate2 ? second : 0) : r;
    uint64_t ss, se;
    text_span(in, 4 * i + 1, ss, se);
    const uint64_t len = se - ss;
    if (lane < SCFQ_SCREEN_MAX_REFS) hits[lane] = 0;
    uint32_t kmers = 0, hit_kmers = 0;
    for (uint64_t c0 = 0; c0 + k <= len; c0 += kChunk) {      // the chunk has a window
      const uint32_t lc = (uint32_t)std::min<uint64_t>(len - c0, kChunk + k - 1), n_win = lc - k + 1, rounds = (lc + 63) / 64;
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
      for (uint32_t q = lane; q < n_win; q += 64) {
        // (q + k <= lc: every bit looked at below lies in a round that was written; what the funnel shifts pull in from the word
        // behind is cut off by kbits and by the shift down to 2k bits)
        const uint32_t o = q & 63u, w = q >> 6;
        const uint64_t ib = o ? (inv[w] >> o) | (inv[w + 1] << (64 - o)) : inv[w];
        if (ib & kbits) continue;
        ++kmers;
        const uint32_t off = 2 * (q & 31u), j = q >> 5;
        const uint64_t hi = code[j], lo = code[j + 1];
        const uint64_t x = off ? (hi << off) | (lo >> (64 - off)) : hi;      // (never a shift by 64)
        const uint64_t fwd = x >> (64 - 2 * k), rc = rev_comp(fwd, k);
        const uint64_t key = fwd < rc ? fwd : rc, h = mix64(key);
        if (filter_words) {
          const uint32_t fb = filter_bit(h, t.filter_bits);
          if (!((flt[fb >> 5] >> (fb & 31u)) & 1u)) continue;      // in no reference
        }
        uint64_t slot = h & (t.slots - 1);
        for (uint64_t step = 0; step < t.slots; ++step) {
          const unsigned long long at = t.keys[slot];
          if (at == key) {
            ++hit_kmers;
            for (uint32_t rest = t.masks[slot]; rest; rest &= rest - 1) atomicAdd(&hits[__builtin_ctz(rest)], 1u);
            break;
          }
          if (at == kEmpty) break;
          slot = (slot + 1) & (t.slots - 1);
        }
      }
    }
    wave_lds_sync();
    const uint32_t n_kmers = (uint32_t)wave_sum(kmers), n_hit = (uint32_t)wave_sum(hit_kmers);
    const uint32_t mine = lane < SCFQ_SCREEN_MAX_REFS ? hits[lane] : 0u;
    const bool match = mine >= std::max(1u, t.min_hits) && 100ull * mine >= (uint64_t)t.min_hit_pct * n_kmers;
    const uint32_t mask = (uint32_t)__builtin_amdgcn_ballot_w64(match) & 0xFFFFu;
    // the most hits, the lowest reference on a tie
    const uint64_t top = wave_max(match ? ((uint64_t)mine << 8) | (255u - lane) : 0ull);
    if (mine) atomicAdd(&ref_hits[lane], (unsigned long long)mine);
    if (lane == 0) {
      scfq_screen_rec out;
      out.kmers = n_kmers;
      out.hit_kmers = n_hit;
      out.best_hits = mask ? (uint32_t)(top >> 8) : 0u;
      out.mask = (uint16_t)mask;
      out.best = mask ? (uint8_t)(255u - (uint32_t)(top & 0xFFu)) : (uint8_t)0xFF;
      out.reserved = 0;
      recs[r] = out;
    }
  }
}

// a unit: a single-end read, or a pair.  S3 and S4 both get it from here, so the lengths the scans saw are the lengths S4 writes
struct ScUnit {
  uint64_t len1, len2;                 // bytes for out1 and out2 (0 for a unit that is not written)
  uint64_t first;                      // of len1, mate 1's record (interleaved input: mate 2's follows it)
  bool kept;
};

__device__ __forceinline__ ScUnit look_up(const RecInput& a, const RecInput& b, uint64_t stride, uint64_t second, uint32_t paired, uint64_t u,
                                          const scfq_screen_rec* recs, uint32_t keep_matched) {
  ScUnit t = {};
  const bool matched = paired ? (recs[2 * u].mask | recs[2 * u + 1].mask) != 0 : recs[u].mask != 0;
  t.kept = matched == (keep_matched != 0);
  if (!t.kept) return t;
  t.first = echo_len(a, paired ? u * stride : u);
  const uint64_t m2 = paired ? echo_len(b, u * stride + second) : 0;
  t.len1 = t.first + (second ? m2 : 0);
  t.len2 = second ? 0 : m2;
  return t;
}

// the counters of S3
enum { kDropped = 0, kMatchedReads, kMatchedPairs, kMulti, kShort, kBasesIn, kBasesOut, kWindows, kKmers, kHitKmers, kRefReads,
       kRefOnly = kRefReads + SCFQ_SCREEN_MAX_REFS, kRefBest = kRefOnly + SCFQ_SCREEN_MAX_REFS, kCounters = kRefBest + SCFQ_SCREEN_MAX_REFS };

// S3.  group_len: two arrays of n_groups + 1 entries, one after the other (the last entry of each stays 0: the scan's total)
__global__ __launch_bounds__(256) void sc_lengths(RecInput a, RecInput b, uint64_t stride, uint64_t second, uint32_t paired, uint64_t units,
                                                 const scfq_screen_rec* recs, uint32_t keep_matched, uint32_t k, uint64_t n_groups, uint64_t* group_len,
                                                 unsigned long long* counters) {
  __shared__ unsigned long long sum_sh[kCounters];
  if (threadIdx.x < kCounters) sum_sh[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = u < units;
  uint64_t len[2] = {0, 0}, c[kRefReads];
#pragma unroll
  for (int x = 0; x < kRefReads; ++x) c[x] = 0;
  scfq_screen_rec rec[2] = {};
  const uint32_t mates = paired ? 2u : 1u;
  if (live) {
    const ScUnit t = look_up(a, b, stride, second, paired, u, recs, keep_matched);
    len[0] = t.len1; len[1] = t.len2;
    bool any = false;
#pragma unroll
    for (uint32_t m = 0; m < 2; ++m) {                     // (constant bounds: rec[] stays in registers)
      if (m >= mates) continue;
      rec[m] = recs[paired ? 2 * u + m : u];
      uint64_t s, e;
      text_span(m ? b : a, 4 * (paired ? u * stride + (m ? second : 0) : u) + 1, s, e);
      const uint64_t L = e - s, windows = L >= k ? L - k + 1 : 0;
      c[kDropped] += !t.kept;
      c[kMatchedReads] += rec[m].mask != 0;
      c[kMulti] += (rec[m].mask & (rec[m].mask - 1)) != 0;
      c[kShort] += L < k;
      c[kBasesIn] += L;
      c[kBasesOut] += t.kept ? L : 0;
      c[kWindows] += windows;
      c[kKmers] += rec[m].kmers;
      c[kHitKmers] += rec[m].hit_kmers;
      any = any || rec[m].mask != 0;
    }
    c[kMatchedPairs] = paired && any;
  }
#pragma unroll
  for (int x = 0; x < 2; ++x) store_group_len(len[x], x, u, units, n_groups, group_len);
  // the statistics: a sum per wave into LDS, then ONE atomic per block and counter.  The counts per reference are ballots
  const bool first_lane = (threadIdx.x & 63) == 0;
#pragma unroll
  for (int x = 0; x < kRefReads; ++x) {
    const uint64_t s = wave_sum(c[x]);
    if (first_lane && s) atomicAdd(&sum_sh[x], (unsigned long long)s);
  }
#pragma unroll
  for (uint32_t m = 0; m < 2; ++m) {
    const uint32_t mask = live && m < mates ? rec[m].mask : 0u;
    if (!__builtin_amdgcn_ballot_w64(mask != 0)) continue;      // (wave-uniform) most waves of a clean run
    for (uint32_t r = 0; r < SCFQ_SCREEN_MAX_REFS; ++r) {
      const uint32_t has = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64((mask >> r) & 1u));
      const uint32_t only = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(mask == (1u << r)));
      const uint32_t best = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(mask != 0 && rec[m].best == r));
      if (first_lane) {
        if (has) atomicAdd(&sum_sh[kRefReads + r], (unsigned long long)has);
        if (only) atomicAdd(&sum_sh[kRefOnly + r], (unsigned long long)only);
        if (best) atomicAdd(&sum_sh[kRefBest + r], (unsigned long long)best);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < kCounters && sum_sh[threadIdx.x]) atomicAdd(&counters[threadIdx.x], sum_sh[threadIdx.x]);
}

// S4.  group_off: the two scanned arrays of S3's layout
__global__ __launch_bounds__(64 * kScWaves) void sc_write(RecInput a, RecInput b, uint64_t stride, uint64_t second, uint32_t paired, uint64_t units,
                                                         const scfq_screen_rec* recs, uint32_t keep_matched, uint64_t n_groups, const uint64_t* group_off,
                                                         RecOut o1, RecOut o2) {
  const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // (when one result is more than its output holds, nothing is written to either)
  if (!(output_fits(o1, 0, n_groups, group_off) && output_fits(o2, 1, n_groups, group_off))) return;
  const uint64_t g = (uint64_t)blockIdx.x * kScWaves + wave;
  if (g >= n_groups) return;
  const uint64_t u0 = g * kScGroup;
  const uint32_t count = (uint32_t)std::min<uint64_t>(kScGroup, units - u0);
  ScUnit mine = {};
  if (lane < count) mine = look_up(a, b, stride, second, paired, u0 + lane, recs, keep_matched);
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

struct Params { uint32_t flags, min_hits, min_hit_pct; };

bool args_ok(const scfq_screen_opts* opts, const scfq_screen_stats* st, Params& p) {
  if (!st || st->struct_size != sizeof(scfq_screen_stats)) return false;
  p = Params{0, 1, 0};
  if (opts) {
    if (opts->struct_size != sizeof(scfq_screen_opts)) return false;
    p = Params{opts->flags, opts->min_hits, opts->min_hit_pct};
    const uint32_t known = SCFQ_SCREEN_INTERLEAVED | SCFQ_SCREEN_KEEP_MATCHED;
    if (p.flags & ~known) { std::snprintf(g_serr, sizeof g_serr, "unknown flag bits 0x%x", p.flags & ~known); return false; }
    if (p.min_hits < 1 || p.min_hits > 65535) { std::snprintf(g_serr, sizeof g_serr, "min_hits %u is not in 1 .. 65535", p.min_hits); return false; }
    if (p.min_hit_pct > 100) { std::snprintf(g_serr, sizeof g_serr, "min_hit_pct %u is not in 0 .. 100", p.min_hit_pct); return false; }
    if (opts->reserved) { std::snprintf(g_serr, sizeof g_serr, "the reserved word is %u, not 0", opts->reserved); return false; }
  }
  return true;
}

bool have_index(const scfq_screen_index* index) {
  if (!index) std::snprintf(g_serr, sizeof g_serr, "the index is NULL");
  return index != nullptr;
}

// recs_out / rec_cap: the caller's per-read table (device memory), or nullptr; recs_keep: where the table stays for the caller of this
// function to copy it (the file entry point)
int screen_device(const scfq_screen_index* ix_, const uint8_t* d1, uint64_t n1, const uint8_t* d2, uint64_t n2, Mode mode, const Params& prm,
                  scfq_screen_rec* recs_out, uint64_t rec_cap, bool check_rec_cap, DevBuf& recs_keep, bool own_outputs, Dest dst[2], DevBuf own[2],
                  bool check_caps, scfq_screen_stats* st, hipStream_t stream) {
  for (double& m : g_stage_ms) m = 0;
  const scfq_screen_index& idx = *ix_;
  int dev = -1;
  SCFQ_SCRATCH_CHK(g_serr, hipGetDevice(&dev));
  if (dev != idx.dev) { std::snprintf(g_serr, sizeof g_serr, "the index lives on device %d, the call runs on device %d", idx.dev, dev); return SCFQ_EARG; }
  const bool paired = mode != Mode::single, interleaved = mode == Mode::interleaved;
  st->input_bytes1 = n1;
  st->input_bytes2 = n2;
  st->flags = prm.flags; st->min_hits = prm.min_hits; st->min_hit_pct = prm.min_hit_pct; st->k = idx.k; st->n_refs = idx.refs.size();
  scfq_overlap::Indexed ix;
  int rc = SCFQ_OK;
  double index_ms = 0;
  uint64_t units = 0, reads = 0;
  if ((rc = scfq_reads::index_units(d1, n1, d2, n2, mode, stream, g_serr, ix, &index_ms, st, &units, &reads))) return rc;
  st->reads_in = reads;
  if (check_rec_cap && recs_out && rec_cap < reads) {
    std::snprintf(g_serr, sizeof g_serr, "the per-read table holds %llu entries, the input has %llu reads", (unsigned long long)rec_cap, (unsigned long long)reads);
    return SCFQ_EARG;
  }
  if (units == 0) return SCFQ_OK;           // (two empty outputs: they fit into anything)
  const uint64_t n_groups = (units + kScGroup - 1) / kScGroup;
  DevBuf group_len, group_off, counters, tmp;
  scfq_reads::GroupScan gs(2, n_groups, group_len, group_off, stream, g_serr);
  if ((!recs_out && (rc = recs_keep.alloc(reads * sizeof(scfq_screen_rec), stream, g_serr))) || (rc = gs.alloc()) ||
      (rc = counters.alloc((kCounters + SCFQ_SCREEN_MAX_REFS) * 8, stream, g_serr)))
    return rc;
  scfq_screen_rec* const recs = recs_out ? recs_out : recs_keep.as<scfq_screen_rec>();
  size_t scan_bytes = 0;
  if ((rc = gs.scratch_bytes(&scan_bytes)) || (rc = tmp.alloc(scan_bytes, stream, g_serr))) return rc;
  static const bool timing = scfq_scratch::env_switch("SCFQ_SCREEN_TIMING");
  scfq_scratch::StageClock clk(stream, timing);
  SCFQ_SCRATCH_CHK(g_serr, hipMemsetAsync(counters.p, 0, (kCounters + SCFQ_SCREEN_MAX_REFS) * 8, stream));
  if ((rc = gs.zero())) return rc;
  const RecInput a = {d1, n1, ix.off1.as<uint64_t>(), ix.lines1, ix.cr1};
  const RecInput b = mode == Mode::two ? RecInput{d2, n2, ix.off2.as<uint64_t>(), ix.lines2, ix.cr2} : a;
  const uint64_t stride = interleaved ? 2 : 1, second = interleaved ? 1 : 0;
  const uint32_t keep_matched = (prm.flags & SCFQ_SCREEN_KEEP_MATCHED) ? 1u : 0u;
  const ScTable table = {reinterpret_cast<const unsigned long long*>(idx.d_keys), idx.d_masks, idx.slots, idx.d_filter, idx.filter_bits, idx.k, prm.min_hits,
                         prm.min_hit_pct};
  unsigned long long* const ref_hits = counters.as<unsigned long long>() + kCounters;
  const size_t lds = (idx.d_filter ? idx.filter_bits / 8 : 0) + (size_t)kScWaves * kWaveLds;
  SCFQ_SCRATCH_CHK(g_serr, hipFuncSetAttribute(reinterpret_cast<const void*>(sc_lookup), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  clk.mark(0);
  hipLaunchKernelGGL(sc_lookup, dim3((unsigned)std::min<uint64_t>((reads + kScWaves - 1) / kScWaves, kScMaxBlocks)), dim3(64 * kScWaves), lds, stream, a, b, stride,
                     second, paired ? 1u : 0u, reads, table, recs, ref_hits);
  SCFQ_SCRATCH_CHK(g_serr, hipGetLastError());
  clk.mark(1);
  hipLaunchKernelGGL(sc_lengths, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, stream, a, b, stride, second, paired ? 1u : 0u, units, recs, keep_matched,
                     idx.k, n_groups, gs.len(), counters.as<unsigned long long>());
  SCFQ_SCRATCH_CHK(g_serr, hipGetLastError());
  if ((rc = gs.scan(tmp.p, scan_bytes))) return rc;
  clk.mark(2);
  // the sizes and the statistics come back first: pool memory for the outputs is taken to fit, and a caller's buffer that is too small
  // is known here
  uint64_t h[kCounters + SCFQ_SCREEN_MAX_REFS];
  if ((rc = gs.read_totals())) return rc;
  SCFQ_SCRATCH_CHK(g_serr, hipMemcpyAsync(h, counters.p, sizeof h, hipMemcpyDeviceToHost, stream));
  SCFQ_SCRATCH_CHK(g_serr, hipStreamSynchronize(stream));
  st->out1_bytes = gs.total[0]; st->out2_bytes = gs.total[1];
  st->dropped_reads = h[kDropped]; st->reads_out = reads - h[kDropped];
  st->matched_reads = h[kMatchedReads]; st->matched_pairs = h[kMatchedPairs]; st->multi_reads = h[kMulti]; st->short_reads = h[kShort];
  st->bases_in = h[kBasesIn]; st->bases_out = h[kBasesOut];
  st->windows = h[kWindows]; st->kmers = h[kKmers]; st->skipped = h[kWindows] - h[kKmers]; st->hit_kmers = h[kHitKmers];
  for (uint32_t r = 0; r < SCFQ_SCREEN_MAX_REFS; ++r) {
    st->ref_reads[r] = h[kRefReads + r]; st->ref_only_reads[r] = h[kRefOnly + r]; st->ref_best_reads[r] = h[kRefBest + r];
    st->ref_kmer_hits[r] = h[kCounters + r];
  }
  const scfq_reads::Placement put = scfq_reads::place_outputs(gs, scfq_reads::kOutNames, dst, own_outputs, check_caps, false, own, stream, g_serr);
  if (put.rc) return put.rc;
  if (put.out[0].p || put.out[1].p) {
    hipLaunchKernelGGL(sc_write, dim3((unsigned)((n_groups + kScWaves - 1) / kScWaves)), dim3(64 * kScWaves), 0, stream, a, b, stride, second, paired ? 1u : 0u,
                       units, recs, keep_matched, n_groups, gs.off(), put.out[0], put.out[1]);
    SCFQ_SCRATCH_CHK(g_serr, hipGetLastError());
  }
  clk.mark(3);
  SCFQ_SCRATCH_CHK(g_serr, hipStreamSynchronize(stream));
  g_stage_ms[0] = index_ms;
  g_stage_ms[1] = clk.between(0, 1);
  g_stage_ms[2] = clk.between(1, 2);
  g_stage_ms[3] = clk.between(2, 3);
  return put.verdict;      // (SCFQ_EARG for an output that is too small: place_outputs has left the text)
}

int env_number(const char* name, int fallback) {
  const char* e = std::getenv(name);
  return e && *e ? std::atoi(e) : fallback;
}

// S1 and the counting pass for what S0 left
int build_index(const scfq_screen_host::Parsed& parsed, uint32_t k, uint64_t slots, scfq_screen_index* idx) {
  SCFQ_SCRATCH_CHK(g_serr, hipGetDevice(&idx->dev));
  idx->k = k;
  idx->slots = slots;
  const bool prefilter = env_number("SCFQ_SCREEN_PREFILTER", 1) != 0;
  const int kb = env_number("SCFQ_SCREEN_PREFILTER_KB", 32);
  if (prefilter) {
    if (kb != 16 && kb != 32 && kb != 64) { std::snprintf(g_serr, sizeof g_serr, "SCFQ_SCREEN_PREFILTER_KB=%d: 16, 32 and 64 are allowed", kb); return SCFQ_EARG; }
    idx->filter_bits = (uint32_t)kb * 1024u * 8u;
  }
  const uint64_t n = parsed.text.size();
  uint8_t* d_text = nullptr;
  unsigned long long* d_counts = nullptr;
  uint32_t* d_failed = nullptr;
  struct Temp { uint8_t*& t; unsigned long long*& c; uint32_t*& f; ~Temp() { if (t) (void)hipFree(t); if (c) (void)hipFree(c); if (f) (void)hipFree(f); } } temp{d_text, d_counts, d_failed};
  constexpr uint32_t kCounts = 2 * SCFQ_SCREEN_MAX_REFS + 1;
  SCFQ_SCRATCH_CHK(g_serr, hipMalloc(&d_text, n));
  SCFQ_SCRATCH_CHK(g_serr, hipMalloc(&d_counts, kCounts * 8));
  SCFQ_SCRATCH_CHK(g_serr, hipMalloc(&d_failed, 4));
  SCFQ_SCRATCH_CHK(g_serr, hipMalloc(&idx->d_keys, slots * 8));
  SCFQ_SCRATCH_CHK(g_serr, hipMalloc(&idx->d_masks, slots * 4));
  if (prefilter) SCFQ_SCRATCH_CHK(g_serr, hipMalloc(&idx->d_filter, idx->filter_bits / 8));
  scfq_scratch::StreamLease lease;
  int rc = lease.acquire(g_serr);
  if (rc) return rc;
  hipStream_t s = lease.s;
  SCFQ_SCRATCH_CHK(g_serr, hipMemcpyAsync(d_text, parsed.text.data(), n, hipMemcpyHostToDevice, s));
  SCFQ_SCRATCH_CHK(g_serr, hipMemsetAsync(idx->d_keys, 0xFF, slots * 8, s));
  SCFQ_SCRATCH_CHK(g_serr, hipMemsetAsync(idx->d_masks, 0, slots * 4, s));
  if (prefilter) SCFQ_SCRATCH_CHK(g_serr, hipMemsetAsync(idx->d_filter, 0, idx->filter_bits / 8, s));
  SCFQ_SCRATCH_CHK(g_serr, hipMemsetAsync(d_counts, 0, kCounts * 8, s));
  SCFQ_SCRATCH_CHK(g_serr, hipMemsetAsync(d_failed, 0, 4, s));
  ScRefs refs;
  for (uint32_t r = 0; r <= SCFQ_SCREEN_MAX_REFS; ++r) refs.begin[r] = r <= idx->refs.size() ? parsed.ref_begin[r] : n;
  scfq_scratch::StageClock clk(s, true);
  clk.mark(0);
  const uint64_t threads = (n + kRun - 1) / kRun;
  hipLaunchKernelGGL(sc_build, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, d_text, n, refs, k, k == 32 ? ~0ull : (1ull << (2 * k)) - 1,
                     reinterpret_cast<unsigned long long*>(idx->d_keys), idx->d_masks, slots, idx->d_filter, idx->filter_bits, d_failed);
  SCFQ_SCRATCH_CHK(g_serr, hipGetLastError());
  clk.mark(1);
  hipLaunchKernelGGL(sc_count_slots, dim3((unsigned)std::min<uint64_t>((slots + 255) / 256, 1024)), dim3(256), 0, s,
                     reinterpret_cast<const unsigned long long*>(idx->d_keys), idx->d_masks, slots, d_counts);
  SCFQ_SCRATCH_CHK(g_serr, hipGetLastError());
  unsigned long long counts[kCounts];
  uint32_t failed = 0;
  SCFQ_SCRATCH_CHK(g_serr, hipMemcpyAsync(counts, d_counts, sizeof counts, hipMemcpyDeviceToHost, s));
  SCFQ_SCRATCH_CHK(g_serr, hipMemcpyAsync(&failed, d_failed, 4, hipMemcpyDeviceToHost, s));
  SCFQ_SCRATCH_CHK(g_serr, hipStreamSynchronize(s));
  lease.clean = true;
  idx->build_ms = clk.between(0, 1);
  if (failed) { std::snprintf(g_serr, sizeof g_serr, "the table of %llu slots did not hold the keys", (unsigned long long)slots); return SCFQ_EARG; }
  idx->distinct = counts[2 * SCFQ_SCREEN_MAX_REFS];
  for (size_t r = 0; r < idx->refs.size(); ++r) {
    idx->refs[r].distinct = counts[r];
    idx->refs[r].shared = counts[SCFQ_SCREEN_MAX_REFS + r];
  }
  return SCFQ_OK;
}

void fill_summary(const scfq_screen_index& idx, scfq_screen_summary* sum) {
  scfq_scratch::clear_keep_size(sum);
  sum->n_refs = idx.refs.size();
  sum->k = idx.k;
  sum->distinct = idx.distinct;
  sum->slots = idx.slots;
  for (size_t r = 0; r < idx.refs.size(); ++r) {
    const scfq_screen_host::RefInfo& i = idx.refs[r];
    sum->ref[r] = scfq_screen_ref_summary{i.contigs, i.bases, i.windows, i.kmers, i.distinct, i.shared};
  }
}

}  // namespace

extern "C" {

const char* scfq_screen_error_detail(void) { return g_serr; }

int scfq_debug_screen_stages(double* ms, uint32_t cap) { return scfq_scratch::copy_stage_ms(g_stage_ms, ms, cap); }

double scfq_debug_screen_build_ms(const scfq_screen_index* index) { return index ? index->build_ms : 0.0; }

int scfq_screen_index_buffers(const scfq_screen_ref* refs, uint32_t n_refs, uint32_t k, scfq_screen_index** out, scfq_screen_summary* sum) {
  g_serr[0] = '\0';
  if (out) *out = nullptr;
  if (!out || (sum && sum->struct_size != sizeof(scfq_screen_summary))) return SCFQ_EARG;
  scfq_screen_index* idx = new scfq_screen_index();
  scfq_screen_host::Parsed parsed;
  uint64_t slots = 0;
  int rc = SCFQ_EARG;
  // every argument error is decided here, before any device call
  if (scfq_screen_host::parse_references(refs, n_refs, k, idx->refs, parsed, g_serr) &&
      scfq_screen_host::pick_slots(parsed.windows, env_number("SCFQ_SCREEN_TABLE_BITS", 0), &slots, g_serr))
    rc = build_index(parsed, k, slots, idx);
  if (rc) { delete idx; return rc; }
  if (sum) fill_summary(*idx, sum);
  *out = idx;
  return SCFQ_OK;
}

int scfq_screen_index_files(const char* const* names, const char* const* paths, uint32_t n_refs, uint32_t k, const scfq_opts* opts, scfq_screen_index** out,
                            scfq_screen_summary* sum) {
  g_serr[0] = '\0';
  if (out) *out = nullptr;
  if (!out || (sum && sum->struct_size != sizeof(scfq_screen_summary))) return SCFQ_EARG;
  if (!paths || n_refs < 1 || n_refs > SCFQ_SCREEN_MAX_REFS) { std::snprintf(g_serr, sizeof g_serr, "%u references: 1 .. %d are allowed", paths ? n_refs : 0u, SCFQ_SCREEN_MAX_REFS); return SCFQ_EARG; }
  if (k < 8 || k > SCFQ_SCREEN_MAX_K) { std::snprintf(g_serr, sizeof g_serr, "k = %u is not in 8 .. %d", k, SCFQ_SCREEN_MAX_K); return SCFQ_EARG; }
  std::vector<std::string> own_names(n_refs);
  std::vector<std::vector<uint8_t>> texts(n_refs);
  std::vector<scfq_screen_ref> refs(n_refs);
  for (uint32_t r = 0; r < n_refs; ++r) {
    if (!paths[r]) { std::snprintf(g_serr, sizeof g_serr, "reference %u has no path", r); return SCFQ_EARG; }
    if (names && names[r]) own_names[r] = names[r];
    else {                                               // the base name up to its first '.'
      const char* slash = std::strrchr(paths[r], '/');
      own_names[r] = slash ? slash + 1 : paths[r];
      own_names[r] = own_names[r].substr(0, own_names[r].find('.'));
    }
    if (!scfq_screen_host::name_ok(own_names[r].c_str(), r, g_serr)) return SCFQ_EARG;
  }
  for (uint32_t r = 0; r < n_refs; ++r) {
    // the library's readers leave the (inflated) file on the device; S0 is host work, so it comes back once
    void* d = nullptr;
    uint64_t n = 0;
    int rc = scfq_stage_file(paths[r], opts, &d, &n);
    if (rc) return rc;
    texts[r].resize(n);
    const hipError_t e = n ? hipMemcpy(texts[r].data(), d, n, hipMemcpyDeviceToHost) : hipSuccess;
    (void)scfq_device_free(d);
    if (e != hipSuccess) { std::snprintf(g_serr, sizeof g_serr, "reference %u: %s", r, hipGetErrorString(e)); return SCFQ_EHIP; }
    refs[r] = scfq_screen_ref{own_names[r].c_str(), texts[r].data(), n};
  }
  return scfq_screen_index_buffers(refs.data(), n_refs, k, out, sum);
}

void scfq_screen_index_free(scfq_screen_index* index) { delete index; }

int scfq_screen_index_summary(const scfq_screen_index* index, scfq_screen_summary* sum) {
  if (!index || !sum || sum->struct_size != sizeof(scfq_screen_summary)) return SCFQ_EARG;
  fill_summary(*index, sum);
  return SCFQ_OK;
}

const char* scfq_screen_ref_name(const scfq_screen_index* index, uint32_t r) {
  return index && r < index->refs.size() ? index->refs[r].name.c_str() : nullptr;
}

int scfq_format_screen_row_tsv(const scfq_screen_stats* s, const scfq_screen_index* index, uint32_t r, char* buf, uint64_t cap) {
  if (!index) return SCFQ_EARG;
  return scfq_screen_host::format_row(s, index->refs, index->k, r, buf, cap);
}

int scfq_screen_buffers(const scfq_screen_index* index, const void* r1, uint64_t n1, const void* r2, uint64_t n2, int is_device, const scfq_screen_opts* opts,
                        scfq_screen_rec* recs_device, uint64_t rec_cap, void* out1, uint64_t cap1, void* out2, uint64_t cap2, int out_is_device,
                        scfq_screen_stats* stats) {
  g_serr[0] = '\0';
  Params prm;
  if (!args_ok(opts, stats, prm) || (!r1 && n1) || (!r2 && n2) || (!out1 && cap1) || (!out2 && cap2) || (!recs_device && rec_cap)) return SCFQ_EARG;
  const bool interleaved = (prm.flags & SCFQ_SCREEN_INTERLEAVED) != 0;
  if (interleaved && (r2 || n2)) { std::snprintf(g_serr, sizeof g_serr, "interleaved input takes no second buffer"); return SCFQ_EARG; }
  const Mode mode = interleaved ? Mode::interleaved : (r2 ? Mode::two : Mode::single);
  if (mode != Mode::two && out2) { std::snprintf(g_serr, sizeof g_serr, "one input has no second output (out2)"); return SCFQ_EARG; }
  if (!have_index(index)) return SCFQ_EARG;
  scfq_scratch::clear_keep_size(stats);
  Dest dst[2] = {{static_cast<uint8_t*>(out1), cap1, out1 != nullptr}, {static_cast<uint8_t*>(out2), cap2, out2 != nullptr}};
  const bool any_out = out1 || out2, direct = any_out && out_is_device;
  scfq_scratch::ResidentInput in1, in2;
  int rc = in1.from_buffer(r1, n1, is_device != 0, is_device || direct || recs_device, g_serr);
  if (rc) return rc;
  if (mode == Mode::two && (rc = in2.from_buffer(r2, n2, is_device != 0, false, g_serr))) return rc;
  DevBuf own[2], recs_keep;
  rc = screen_device(index, in1.d_in, in1.n, in2.d_in, in2.n, mode, prm, recs_device, rec_cap, true, recs_keep, /*own_outputs=*/!direct, dst, own,
                     /*check_caps=*/true, stats, in1.stream);
  if (rc) return finish(in1, rc);
  if (!direct) {
    const uint64_t bytes[2] = {stats->out1_bytes, stats->out2_bytes};
    if ((rc = scfq_reads::outputs_to_host(2, dst, own, bytes, in1.stream, g_serr))) return rc;
    SCFQ_SCRATCH_CHK(g_serr, hipStreamSynchronize(in1.stream));
  }
  for (DevBuf& o : own) o.drop();
  recs_keep.drop();
  in1.mark_clean();      // (the last act was to wait for the stream; behind it lie returns of pool memory only)
  return SCFQ_OK;
}

int scfq_screen_files(const scfq_screen_index* index, const char* path1, const char* path2, const scfq_opts* opts, const scfq_screen_opts* sopts, int out1_fd,
                      int out2_fd, scfq_screen_rec* recs_host, uint64_t rec_cap, scfq_screen_stats* stats) {
  g_serr[0] = '\0';
  Params prm;
  if (!path1 || !args_ok(sopts, stats, prm) || (!recs_host && rec_cap)) return SCFQ_EARG;
  const bool interleaved = (prm.flags & SCFQ_SCREEN_INTERLEAVED) != 0;
  if (interleaved && path2) { std::snprintf(g_serr, sizeof g_serr, "interleaved input takes no second file"); return SCFQ_EARG; }
  const Mode mode = interleaved ? Mode::interleaved : (path2 ? Mode::two : Mode::single);
  if (mode != Mode::two && out2_fd >= 0) { std::snprintf(g_serr, sizeof g_serr, "one input has no second output (out2)"); return SCFQ_EARG; }
  if (!have_index(index)) return SCFQ_EARG;
  scfq_scratch::clear_keep_size(stats);
  scfq_scratch::ResidentInput in1, in2;
  int rc = in1.from_file(path1, opts, g_serr);
  if (rc) return rc;
  if (mode == Mode::two && (rc = in2.from_file(path2, opts, g_serr))) return rc;      // (staged when this returns)
  const int fd[2] = {out1_fd, out2_fd};
  Dest dst[2] = {{nullptr, 0, out1_fd >= 0}, {nullptr, 0, out2_fd >= 0}};
  DevBuf own[2], recs_keep;
  rc = screen_device(index, in1.d_in, in1.n, in2.d_in, in2.n, mode, prm, nullptr, 0, false, recs_keep, /*own_outputs=*/true, dst, own, /*check_caps=*/false, stats,
                     in1.stream);
  if (rc) return finish(in1, rc);
  if (recs_host && stats->reads_in) {
    if (rec_cap < stats->reads_in) {
      std::snprintf(g_serr, sizeof g_serr, "the per-read table holds %llu entries, the input has %llu reads", (unsigned long long)rec_cap, (unsigned long long)stats->reads_in);
      return finish(in1, SCFQ_EARG);
    }
    SCFQ_SCRATCH_CHK(g_serr, hipMemcpyAsync(recs_host, recs_keep.p, stats->reads_in * sizeof(scfq_screen_rec), hipMemcpyDeviceToHost, in1.stream));
    SCFQ_SCRATCH_CHK(g_serr, hipStreamSynchronize(in1.stream));
  }
  const uint64_t bytes[2] = {stats->out1_bytes, stats->out2_bytes};
  return scfq_reads::outputs_to_fds(2, own, bytes, fd, in1, g_serr);
}

}  // extern "C"

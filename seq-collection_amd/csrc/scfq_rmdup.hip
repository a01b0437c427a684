// scfq_rmdup.hip — `sc fq-rmdup` on the MI355X (gfx950): duplicate reads and pairs removed by sequence.
// Not in the reference; definitions in include/sc_fqcount.h.
//
// The input sits in HBM whole (one FASTQ, two, or one interleaved).  A unit is a read or a pair; its key is the first `prefix` bytes of
// its sequence text(s) with their length(s).
//   K5  line index            (scfq_scratch::build_line_index) of each input
//   U1  ru_hash               the first hot path: EIGHT lanes per unit, eight units per wave and step.  Lane g of a group takes the 8-byte
//                             words g, g + 8, ... of a key (one 64-byte line per group and step), adds their contributions to the two sums
//                             of scfq_hdrhash.hpp, and the group folds the sums with three shuffles behind the loop.  A word is one
//                             unaligned 8-byte load when its 8 bytes lie inside the input and is built from byte loads when they do not;
//                             the bytes behind the key are masked off.  The two mates' hashes are combined in order, or, with
//                             SCFQ_RMDUP_SWAPPED, smaller first.  key = the hash's low hash_bits bits.
//       radix sort            rocprim::radix_sort_pairs of (key, unit) over hash_bits bits; stable: equal keys stay in input order
//   rounds over a LIST of sorted positions (round 0: all of them, implicit; later: what the round before left over, ascending)
//   U2  ru_heads              an entry whose key differs from its predecessor's starts a run: its unit is a representative.  Every
//                             other entry is a candidate: compacted, 2048 entries and ONE atomic per block (dd_find_equal's lesson).
//       max-scan              over "my own place if I start a run, else 0": every entry's head
//   U3  ru_compare            the second hot path: eight lanes per candidate compare its unit with the unit of its run's HEAD, never
//                             with any other member: lengths first, then 8-byte words as in U1.  Equal: rep = the head's unit.  Not
//                             equal: the entry's flag is set.  (A class of 200 000 identical reads reads one head 200 000 times; a scan
//                             over "the earlier members of the run" would be quadratic.)
//       rocprim::select       the flagged entries, in order, are the next round's list; its length comes back (4 bytes a round)
//   The list shrinks strictly — every run loses its head at the least — so the loop needs no bound of its own.
//   U3c ru_class_sizes        a thread per sorted position: adjacent lanes with one rep are merged and the first adds the run's length
//   U4  ru_lengths            a thread per unit: kept iff rep == unit, the table, output lengths per group of kGroup, the statistics — one
//                             atomic per block and counter — and the histogram (LDS, then one atomic per block and non-empty bin)
//       exclusive scans       one per output over the groups, each with a last entry that is the output's size
//   U5  ru_write              a wave per group echoes the kept records (sc_write's shape)
// U5 compares the two totals with the capacities before it stores anything.  Everything is integer / byte work; there is no CPU fallback.
#include "../../include/sc_fqcount.h"
#include "../../include/sc_fqcount_debug.h"

#include <cstring>        // (rocprim's texture iterator calls memset from host code)
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "scfq_hdrhash.hpp"
#include "scfq_reads_host.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

static_assert(sizeof(scfq_rmdup_rec) == 8 && sizeof(scfq_rmdup_stats) == 26 * 8 && sizeof(scfq_rmdup_opts) == 32, "the ABI's sizes");

namespace {

constexpr uint32_t kStages = 7;
thread_local char g_rerr[scfq_scratch::kErrBytes] = "";
thread_local double g_stage_ms[kStages] = {0, 0, 0, 0, 0, 0, 0};

using scfq_reads::Dest;
using scfq_reads::DevBuf;
using scfq_reads::finish;
using scfq_reads::Mode;

constexpr uint32_t kLanes = 8;                 // lanes of a group: one unit of U1, one candidate of U3
constexpr uint32_t kMaxBlocks = 8192;          // of U1 and U3: the blocks stride
constexpr uint32_t kGroup = kRecGroup;         // units of a group: one wave of U5, one entry of the scans
constexpr uint32_t kWaves = 4;                 // groups of a block of U5
constexpr uint32_t kDefaultHashBits = 40;      // (five radix passes instead of eight; measured beside 32 and 64: DESIGN.md §fq-rmdup)
constexpr uint64_t kSeed = 0x5DEECE66D1CE4E5Bull;

// the counters of U4; the histogram follows them
enum { kUnitsOut = 0, kDupClasses, kBasesIn, kBasesOut, kMaxCopies, kCounters };

struct RuPlan {           // where the units are: record u * stride of a, record u * stride + second of b
  uint64_t stride, second, units;
  uint32_t paired, swapped, prefix;
};

// a key: len bytes at p, of which `room` bytes (>= len) lie inside the input
struct RuKey {
  const uint8_t* p;
  uint64_t len, room;
};

__device__ __forceinline__ RuKey key_of(const RecInput& in, uint64_t record, uint32_t prefix) {
  uint64_t s, e;
  text_span(in, 4 * record + 1, s, e);
  uint64_t len = e - s;
  if (prefix && len > prefix) len = prefix;
  return RuKey{in.base + s, len, in.n - s};
}

__device__ __forceinline__ RuKey mate_key(const RecInput& a, const RecInput& b, const RuPlan& pl, uint64_t u, uint32_t mate) {
  return mate ? key_of(b, u * pl.stride + pl.second, pl.prefix) : key_of(a, pl.paired ? u * pl.stride : u, pl.prefix);
}

// word w of a key (8 w < len), little-endian, zero behind the key.  No byte outside [p, p + room) is touched
__device__ __forceinline__ uint64_t key_word(const RuKey& k, uint64_t w) {
  const uint64_t at = 8 * w, left = k.len - at;
  uint64_t v = 0;
  if (at + 8 <= k.room) {
    __builtin_memcpy(&v, k.p + at, 8);                     // (arbitrarily aligned)
    if (left < 8) v &= (1ull << (8 * left)) - 1ull;
  } else {
    for (uint64_t i = 0; i < left && i < 8; ++i) v |= (uint64_t)k.p[at + i] << (8 * i);      // (at + left <= room)
  }
  return v;
}

__device__ __forceinline__ uint32_t group_sum(uint32_t v) {        // over the kLanes lanes of a group
#pragma unroll
  for (int o = 1; o < (int)kLanes; o <<= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}
__device__ __forceinline__ uint32_t group_or(uint32_t v) {
#pragma unroll
  for (int o = 1; o < (int)kLanes; o <<= 1) v |= (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}

// the hash of a key, by the group (g: the lane's place in it); `on` is the group's: a group that is off walks no word.  Every lane of
// the wave gets here, so the shuffles behind the loop meet all their partners
__device__ __forceinline__ uint64_t group_hash(const RuKey& k, uint32_t g, bool on) {
  uint32_t A = 0, B = 0;
  const uint64_t words = on ? (k.len + 7) / 8 : 0;
  for (uint64_t w = g; w < words; w += kLanes) {
    const uint64_t v = key_word(k, w);
    scfq_hdrhash::hh_word((uint32_t)v, (uint32_t)(v >> 32), (uint32_t)w, A, B);
  }
  A = group_sum(A);
  B = group_sum(B);
  // (hh_final keeps 24 bits of B; the rest goes in through the seed's place)
  return scfq_hdrhash::hh_final(A, B, k.len, kSeed ^ ((uint64_t)(B >> 24) << 40));
}

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
  return x;
}

// U1
__global__ __launch_bounds__(256) void ru_hash(RecInput a, RecInput b, RuPlan pl, uint32_t hash_bits, uint64_t* keys, uint32_t* idx) {
  const uint32_t g = threadIdx.x & (kLanes - 1);
  const uint64_t per_step = (uint64_t)gridDim.x * (256 / kLanes);
  const uint64_t steps = (pl.units + per_step - 1) / per_step;            // (the same for every lane: the shuffles are never divergent)
  uint64_t u = (uint64_t)blockIdx.x * (256 / kLanes) + threadIdx.x / kLanes;
  for (uint64_t step = 0; step < steps; ++step, u += per_step) {
    const bool on = u < pl.units;
    const uint64_t uu = on ? u : 0;
    uint64_t h = group_hash(on ? mate_key(a, b, pl, uu, 0) : RuKey{nullptr, 0, 0}, g, on);
    if (pl.paired) {
      uint64_t h2 = group_hash(on ? mate_key(a, b, pl, uu, 1) : RuKey{nullptr, 0, 0}, g, on);
      if (pl.swapped && h2 < h) { const uint64_t t = h; h = h2; h2 = t; }
      h = mix64(h ^ mix64(h2 + 0x9E3779B97F4A7C15ull));
    }
    if (on && g == 0) {
      keys[u] = hash_bits >= 64 ? h : h & ((1ull << hash_bits) - 1ull);
      idx[u] = (uint32_t)u;
    }
  }
}

// U2.  list: the sorted positions of this round, ascending (nullptr: all of them); m entries.  start_at[t]: t for an entry that starts a
// run, else 0.  left[t] = 0.  The candidates (entries that start no run) are compacted into cand, counted in *n_cand.
__global__ __launch_bounds__(256) void ru_heads(const uint64_t* keys_sorted, const uint32_t* idx_sorted, const uint32_t* list, uint64_t m, uint32_t* rep,
                                               uint32_t* start_at, uint8_t* left, uint32_t* cand, uint32_t* n_cand) {
  __shared__ uint32_t wave_cnt[8][4], block_base;
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t base = (uint64_t)blockIdx.x * 2048;
  uint64_t bal[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint64_t t = base + 256u * j + threadIdx.x;
    bool is_cand = false;
    if (t < m) {
      const uint32_t p = list ? list[t] : (uint32_t)t;
      const bool start = t == 0 || keys_sorted[p] != keys_sorted[list ? list[t - 1] : (uint32_t)(t - 1)];
      if (start) { const uint32_t unit = idx_sorted[p]; rep[unit] = unit; }
      start_at[t] = start ? (uint32_t)t : 0u;
      left[t] = 0;
      is_cand = !start;
    }
    bal[j] = __builtin_amdgcn_ballot_w64(is_cand);
    if (lane == 0) wave_cnt[j][w] = (uint32_t)__popcll(bal[j]);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t tot = 0;
    for (int j = 0; j < 8; ++j) for (int k = 0; k < 4; ++k) tot += wave_cnt[j][k];
    block_base = tot ? atomicAdd(n_cand, tot) : 0u;
  }
  __syncthreads();
  uint32_t before = block_base;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    for (uint32_t k = 0; k < w; ++k) before += wave_cnt[j][k];
    if ((bal[j] >> lane) & 1ull) cand[before + (uint32_t)__popcll(bal[j] & ((1ull << lane) - 1))] = (uint32_t)(base + 256u * j + threadIdx.x);
    for (uint32_t k = w; k < 4; ++k) before += wave_cnt[j][k];
  }
}

// are the two keys different?  By the group; `on` is the group's.  Lengths first, then the words
__device__ __forceinline__ bool group_differs(const RuKey& x, const RuKey& y, uint32_t g, bool on) {
  uint32_t diff = on && x.len != y.len;
  const uint64_t words = (on && !diff) ? (x.len + 7) / 8 : 0;
  for (uint64_t w = g; w < words; w += kLanes) diff |= key_word(x, w) != key_word(y, w);
  return group_or(diff) != 0;
}

// U3.  cand: entries t of the list; head[t]: the entry that starts t's run
__global__ __launch_bounds__(256) void ru_compare(RecInput a, RecInput b, RuPlan pl, const uint32_t* idx_sorted, const uint32_t* list, const uint32_t* head,
                                                 const uint32_t* cand, const uint32_t* n_cand, uint32_t* rep, uint8_t* left, unsigned long long* collisions) {
  __shared__ uint32_t wave_miss[4];
  const uint32_t g = threadIdx.x & (kLanes - 1), lane = threadIdx.x & 63;
  const uint64_t total = *n_cand;
  const uint64_t per_step = (uint64_t)gridDim.x * (256 / kLanes);
  const uint64_t steps = (total + per_step - 1) / per_step;               // (kernel-uniform)
  uint64_t c = (uint64_t)blockIdx.x * (256 / kLanes) + threadIdx.x / kLanes;
  uint32_t missed = 0;
  for (uint64_t step = 0; step < steps; ++step, c += per_step) {
    const bool on = c < total;
    uint32_t t = 0, mine = 0, heads = 0;
    if (on) {
      t = cand[c];
      const uint32_t ht = head[t];
      mine = idx_sorted[list ? list[t] : t];
      heads = idx_sorted[list ? list[ht] : ht];
    }
    const RuKey none = {nullptr, 0, 0};
    const RuKey m1 = on ? mate_key(a, b, pl, mine, 0) : none, h1 = on ? mate_key(a, b, pl, heads, 0) : none;
    bool differs = group_differs(m1, h1, g, on);
    if (pl.paired) {
      const RuKey m2 = on ? mate_key(a, b, pl, mine, 1) : none, h2 = on ? mate_key(a, b, pl, heads, 1) : none;
      differs = group_differs(m2, h2, g, on && !differs) || differs;
      if (pl.swapped) {
        const bool try_swapped = on && differs;
        const bool d1 = group_differs(m1, h2, g, try_swapped);
        const bool d2 = group_differs(m2, h1, g, try_swapped && !d1);
        if (try_swapped && !d1 && !d2) differs = false;
      }
    }
    if (on && g == 0) {
      if (differs) { left[t] = 1; ++missed; }
      else rep[mine] = heads;
    }
  }
  // the collisions: one atomic per block
  const uint64_t s = wave_sum((uint64_t)missed);
  if (lane == 0) wave_miss[threadIdx.x >> 6] = (uint32_t)s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t tot = wave_miss[0] + wave_miss[1] + wave_miss[2] + wave_miss[3];
    if (tot) atomicAdd(collisions, (unsigned long long)tot);
  }
}

// the class sizes: position p of the sorted order adds to copies[rep of its unit]; adjacent lanes with one rep add once
__global__ __launch_bounds__(256) void ru_class_sizes(const uint32_t* idx_sorted, const uint32_t* rep, uint64_t units, uint32_t* copies) {
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63;
  const bool on = p < units;
  const uint32_t r = on ? rep[idx_sorted[p]] : 0u;
  const uint32_t before = (uint32_t)__shfl_up((int)r, 1, 64);
  const uint64_t edge = __builtin_amdgcn_ballot_w64(!on || lane == 0 || r != before);      // a lane that is off ends the run in front of it
  if (on && ((edge >> lane) & 1ull)) {
    const uint64_t above = edge & ~((2ull << lane) - 1ull);
    const uint32_t len = above ? (uint32_t)__builtin_ctzll(above) - lane : 64u - lane;
    atomicAdd(&copies[r], len);
  }
}

// what a unit adds to the two outputs if it is kept.  U4 and U5 both get it from here
struct RuUnit {
  uint64_t len1, len2;                 // bytes for out1 and out2
  uint64_t first;                      // of len1, mate 1's record (interleaved input: mate 2's follows it)
};

__device__ __forceinline__ RuUnit unit_lengths(const RecInput& a, const RecInput& b, const RuPlan& pl, uint64_t u) {
  RuUnit t = {};
  t.first = echo_len(a, pl.paired ? u * pl.stride : u);
  const uint64_t l2 = pl.paired ? echo_len(b, u * pl.stride + pl.second) : 0;
  t.len1 = t.first + (pl.second ? l2 : 0);
  t.len2 = pl.second ? 0 : l2;
  return t;
}

// U4.  group_len: two arrays of n_groups + 1 entries, one after the other (the last entry of each stays 0: the scan's total).  counters:
// kCounters words, then the SCFQ_RMDUP_HIST_BINS of the histogram.  recs: the table, or nullptr
__global__ __launch_bounds__(256) void ru_lengths(RecInput a, RecInput b, RuPlan pl, const uint32_t* rep, const uint32_t* copies, scfq_rmdup_rec* recs,
                                                 uint64_t n_groups, uint64_t* group_len, unsigned long long* counters) {
  __shared__ uint64_t sum_sh[kCounters][4];
  __shared__ uint32_t hist_sh[SCFQ_RMDUP_HIST_BINS];
  for (uint32_t k = threadIdx.x; k < SCFQ_RMDUP_HIST_BINS; k += 256) hist_sh[k] = 0;
  __syncthreads();
  const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint64_t len[2] = {0, 0}, c[kCounters];
#pragma unroll
  for (int k = 0; k < kCounters; ++k) c[k] = 0;
  uint32_t bin = 0;
  if (u < pl.units) {
    const uint32_t r = rep[u];
    const bool kept = r == (uint32_t)u;
    const uint32_t n = kept ? copies[u] : 0u;
    if (recs) recs[u] = scfq_rmdup_rec{r, n};
    uint64_t bases = 0;
    for (uint32_t mate = 0; mate <= pl.paired; ++mate) {
      uint64_t s, e;
      text_span(mate ? b : a, 4 * (mate ? u * pl.stride + pl.second : (pl.paired ? u * pl.stride : u)) + 1, s, e);
      bases += e - s;
    }
    c[kBasesIn] = bases;
    if (kept) {
      const RuUnit t = unit_lengths(a, b, pl, u);
      len[0] = t.len1; len[1] = t.len2;
      c[kUnitsOut] = 1;
      c[kDupClasses] = n >= 2;
      c[kBasesOut] = bases;
      c[kMaxCopies] = n;
      bin = std::min<uint32_t>(n, SCFQ_RMDUP_HIST_BINS - 1);
    }
  }
  // the histogram: the classes of one member — nearly all of them — are counted by a ballot, the others one by one
  const uint64_t ones = __builtin_amdgcn_ballot_w64(bin == 1);
  if ((threadIdx.x & 63) == 0 && ones) atomicAdd(&hist_sh[1], (uint32_t)__popcll(ones));
  if (bin > 1) atomicAdd(&hist_sh[bin], 1u);
#pragma unroll
  for (int k = 0; k < 2; ++k) store_group_len(len[k], k, u, pl.units, n_groups, group_len);
  // the statistics: ONE atomic per block and counter (dd_count_marks: an atomic per wave on one address costs more than the kernel)
#pragma unroll
  for (int k = 0; k < kCounters; ++k) {
    const uint64_t s = k == kMaxCopies ? wave_max(c[k]) : wave_sum(c[k]);
    if ((threadIdx.x & 63) == 0) sum_sh[k][threadIdx.x >> 6] = s;
  }
  __syncthreads();
  if (threadIdx.x < kCounters) {
    const uint64_t* v = sum_sh[threadIdx.x];
    if (threadIdx.x == kMaxCopies) {
      const uint64_t t = std::max(std::max(v[0], v[1]), std::max(v[2], v[3]));
      if (t) atomicMax(&counters[threadIdx.x], (unsigned long long)t);
    } else {
      const uint64_t t = v[0] + v[1] + v[2] + v[3];
      if (t) atomicAdd(&counters[threadIdx.x], (unsigned long long)t);
    }
  }
  for (uint32_t k = threadIdx.x; k < SCFQ_RMDUP_HIST_BINS; k += 256)
    if (hist_sh[k]) atomicAdd(&counters[kCounters + k], (unsigned long long)hist_sh[k]);
}

// U5.  group_off: the two scanned arrays of U4's layout
__global__ __launch_bounds__(64 * kWaves) void ru_write(RecInput a, RecInput b, RuPlan pl, const uint32_t* rep, uint64_t n_groups, const uint64_t* group_off,
                                                       RecOut o1, RecOut o2) {
  const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // (when one result is more than its output holds, nothing is written to either)
  if (!(output_fits(o1, 0, n_groups, group_off) && output_fits(o2, 1, n_groups, group_off))) return;
  const uint64_t g = (uint64_t)blockIdx.x * kWaves + wave;
  if (g >= n_groups) return;
  const uint64_t u0 = g * kGroup;
  const uint32_t count = (uint32_t)std::min<uint64_t>(kGroup, pl.units - u0);
  RuUnit mine = {};
  uint32_t kept = 0;
  if (lane < count && rep[u0 + lane] == (uint32_t)(u0 + lane)) { mine = unit_lengths(a, b, pl, u0 + lane); kept = 1; }
  const uint64_t len[2] = {mine.len1, mine.len2};
  uint64_t at[2];
  place_units(len, g, n_groups, group_off, lane, at);
  const uint64_t keep_mask = __builtin_amdgcn_ballot_w64(kept != 0);
  for (uint32_t q = 0; q < count; ++q) {
    if (!((keep_mask >> q) & 1ull)) continue;                 // (wave-uniform)
    const uint64_t l1 = bcast(mine.len1, q), l2 = bcast(mine.len2, q), first = bcast(mine.first, q), w1 = bcast(at[0], q), w2 = bcast(at[1], q);
    const uint64_t u = u0 + q;
    const uint64_t i1 = pl.paired ? u * pl.stride : u, i2 = u * pl.stride + pl.second;
    if (o1.p && first) echo_record(a, i1, o1.p + w1, first, lane);
    if (pl.paired) {
      if (pl.second) { if (o1.p && l1 > first) echo_record(b, i2, o1.p + w1 + first, l1 - first, lane); }
      else if (o2.p && l2) echo_record(b, i2, o2.p + w2, l2, lane);
    }
  }
}

struct Params { uint32_t flags, prefix, hash_bits; };

bool args_ok(const scfq_rmdup_opts* opts, const scfq_rmdup_stats* st, Params& p) {
  if (!st || st->struct_size != sizeof(scfq_rmdup_stats)) return false;
  p = Params{0, 0, kDefaultHashBits};
  if (opts) {
    if (opts->struct_size != sizeof(scfq_rmdup_opts)) return false;
    p.flags = opts->flags;
    p.prefix = opts->prefix;
    const uint32_t known = SCFQ_RMDUP_INTERLEAVED | SCFQ_RMDUP_SWAPPED;
    if (p.flags & ~known) { std::snprintf(g_rerr, sizeof g_rerr, "unknown flag bits 0x%x", p.flags & ~known); return false; }
    if (p.prefix > SCFQ_RMDUP_MAX_PREFIX) { std::snprintf(g_rerr, sizeof g_rerr, "prefix %u is not in 0 .. %d", p.prefix, SCFQ_RMDUP_MAX_PREFIX); return false; }
    if (opts->hash_bits > 64) { std::snprintf(g_rerr, sizeof g_rerr, "hash_bits %u is not in 0 .. 64", opts->hash_bits); return false; }
    if (opts->hash_bits) p.hash_bits = opts->hash_bits;
    if (opts->reserved[0] || opts->reserved[1] || opts->reserved[2]) {
      std::snprintf(g_rerr, sizeof g_rerr, "the reserved words are %u, %u and %u, not 0", opts->reserved[0], opts->reserved[1], opts->reserved[2]);
      return false;
    }
  }
  return true;
}

bool mode_ok(const Params& prm, bool second, bool out2, const char* what, Mode& mode) {
  const bool interleaved = (prm.flags & SCFQ_RMDUP_INTERLEAVED) != 0;
  if (interleaved && second) { std::snprintf(g_rerr, sizeof g_rerr, "interleaved input takes no second %s", what); return false; }
  mode = interleaved ? Mode::interleaved : (second ? Mode::two : Mode::single);
  if (mode == Mode::single && (prm.flags & SCFQ_RMDUP_SWAPPED)) {
    std::snprintf(g_rerr, sizeof g_rerr, "SCFQ_RMDUP_SWAPPED compares the mates of pairs: single-end input has none");
    return false;
  }
  if (mode != Mode::two && out2) { std::snprintf(g_rerr, sizeof g_rerr, "one input has no second output (out2)"); return false; }
  return true;
}

// recs_dev / recs_cap: the caller's per-unit table in device memory, or nullptr; want_recs with check_recs: a table of recs_cap entries is
// wanted wherever it lives, and one that is too small is an error once the statistics are complete.  recs_keep: where the table stays
// for the caller of this function when it is not the caller's device memory.  hist_host: nullptr, or SCFQ_RMDUP_HIST_BINS words
int rmdup_device(const uint8_t* d1, uint64_t n1, const uint8_t* d2, uint64_t n2, Mode mode, const Params& prm, scfq_rmdup_rec* recs_dev, bool want_recs,
                 uint64_t recs_cap, bool check_recs, DevBuf& recs_keep, uint64_t* hist_host, bool own_outputs, Dest dst[2], DevBuf own[2], bool check_caps,
                 scfq_rmdup_stats* st, hipStream_t stream) {
  for (double& m : g_stage_ms) m = 0;
  const bool paired = mode != Mode::single, interleaved = mode == Mode::interleaved;
  st->input_bytes1 = n1;
  st->input_bytes2 = n2;
  st->flags = prm.flags; st->prefix = prm.prefix; st->hash_bits = prm.hash_bits;
  if (hist_host) std::memset(hist_host, 0, SCFQ_RMDUP_HIST_BINS * 8);
  scfq_overlap::Indexed ix;
  int rc = SCFQ_OK;
  double index_ms = 0;
  uint64_t units = 0, reads = 0;
  if ((rc = scfq_reads::index_units(d1, n1, d2, n2, mode, stream, g_rerr, ix, &index_ms, st, &units, &reads))) return rc;
  st->units_in = units;
  st->reads_in = reads;
  const bool recs_small = check_recs && want_recs && recs_cap < units;
  if (units == 0) return SCFQ_OK;           // (two empty outputs: they fit into anything)
  const uint64_t n_groups = (units + kGroup - 1) / kGroup;
  const bool to_caller = recs_dev && !recs_small;
  const bool make_recs = want_recs && !recs_small;
  constexpr size_t kWordsOut = kCounters + SCFQ_RMDUP_HIST_BINS;
  DevBuf keys, keys2, idx, idx2, rep, copies, start_at, head, cand, left, list[2], words, group_len, group_off, counters, tmp;
  scfq_reads::GroupScan gs(2, n_groups, group_len, group_off, stream, g_rerr);
  if ((make_recs && !to_caller && (rc = recs_keep.alloc(units * sizeof(scfq_rmdup_rec), stream, g_rerr))) || (rc = keys.alloc(units * 8, stream, g_rerr)) ||
      (rc = keys2.alloc(units * 8, stream, g_rerr)) || (rc = idx.alloc(units * 4, stream, g_rerr)) || (rc = idx2.alloc(units * 4, stream, g_rerr)) ||
      (rc = rep.alloc(units * 4, stream, g_rerr)) || (rc = copies.alloc(units * 4, stream, g_rerr)) || (rc = start_at.alloc(units * 4, stream, g_rerr)) ||
      (rc = head.alloc(units * 4, stream, g_rerr)) || (rc = cand.alloc(units * 4, stream, g_rerr)) || (rc = left.alloc(units, stream, g_rerr)) ||
      (rc = words.alloc(32, stream, g_rerr)) || (rc = gs.alloc()) ||
      (rc = counters.alloc(kWordsOut * 8, stream, g_rerr)))
    return rc;
  scfq_rmdup_rec* const recs = to_caller ? recs_dev : (make_recs ? recs_keep.as<scfq_rmdup_rec>() : nullptr);
  // words: [0] the candidates of the round, [1] what it leaves over, [2 .. 3] the collisions (64 bits)
  uint32_t* const n_cand = words.as<uint32_t>();
  uint32_t* const n_left = n_cand + 1;
  unsigned long long* const collisions = reinterpret_cast<unsigned long long*>(words.as<uint32_t>() + 2);
  size_t sort_bytes = 0, scan_bytes = 0, max_bytes = 0, select_bytes = 0;
  SCFQ_SCRATCH_CHK(g_rerr, rocprim::radix_sort_pairs(nullptr, sort_bytes, keys.as<uint64_t>(), keys2.as<uint64_t>(), idx.as<uint32_t>(), idx2.as<uint32_t>(),
                                                     (size_t)units, 0u, prm.hash_bits, stream));
  if ((rc = gs.scratch_bytes(&scan_bytes))) return rc;
  SCFQ_SCRATCH_CHK(g_rerr, rocprim::inclusive_scan(nullptr, max_bytes, start_at.as<uint32_t>(), head.as<uint32_t>(), (size_t)units, rocprim::maximum<uint32_t>(), stream));
  SCFQ_SCRATCH_CHK(g_rerr, rocprim::select(nullptr, select_bytes, rocprim::counting_iterator<uint32_t>(0), left.as<uint8_t>(), cand.as<uint32_t>(), n_left,
                                           (size_t)units, stream));
  if ((rc = tmp.alloc(std::max(std::max(sort_bytes, scan_bytes), std::max(max_bytes, select_bytes)), stream, g_rerr))) return rc;
  const size_t tmp_bytes = std::max(std::max(sort_bytes, scan_bytes), std::max(max_bytes, select_bytes));
  static const bool timing = scfq_scratch::env_switch("SCFQ_RMDUP_TIMING");
  scfq_scratch::StageClock clk(stream, timing), clk2(stream, timing);
  SCFQ_SCRATCH_CHK(g_rerr, hipMemsetAsync(counters.p, 0, kWordsOut * 8, stream));
  if ((rc = gs.zero())) return rc;
  SCFQ_SCRATCH_CHK(g_rerr, hipMemsetAsync(copies.p, 0, units * 4, stream));
  SCFQ_SCRATCH_CHK(g_rerr, hipMemsetAsync(words.p, 0, 32, stream));
  const RecInput a = {d1, n1, ix.off1.as<uint64_t>(), ix.lines1, ix.cr1};
  const RecInput b = mode == Mode::two ? RecInput{d2, n2, ix.off2.as<uint64_t>(), ix.lines2, ix.cr2} : a;
  const RuPlan pl = {interleaved ? 2ull : 1ull, interleaved ? 1ull : 0ull, units, paired ? 1u : 0u, (prm.flags & SCFQ_RMDUP_SWAPPED) ? 1u : 0u, prm.prefix};
  auto group_blocks = [](uint64_t items) { return dim3((unsigned)std::min<uint64_t>((items + 256 / kLanes - 1) / (256 / kLanes), kMaxBlocks)); };
  clk.mark(0);
  hipLaunchKernelGGL(ru_hash, group_blocks(units), dim3(256), 0, stream, a, b, pl, prm.hash_bits, keys.as<uint64_t>(), idx.as<uint32_t>());
  SCFQ_SCRATCH_CHK(g_rerr, hipGetLastError());
  clk.mark(1);
  SCFQ_SCRATCH_CHK(g_rerr, rocprim::radix_sort_pairs(tmp.p, sort_bytes, keys.as<uint64_t>(), keys2.as<uint64_t>(), idx.as<uint32_t>(), idx2.as<uint32_t>(),
                                                     (size_t)units, 0u, prm.hash_bits, stream));
  clk.mark(2);
  // the rounds.  m: the entries of this round's list (round 0: every sorted position; list[] is not used)
  uint64_t m = units, rounds = 0;
  const uint32_t* cur = nullptr;
  for (uint32_t round = 0; m > 0; ++round) {
    DevBuf& next = list[round & 1];
    if ((rc = next.alloc(m * 4, stream, g_rerr))) return rc;             // (at most m - 1 are left over)
    SCFQ_SCRATCH_CHK(g_rerr, hipMemsetAsync(n_cand, 0, 8, stream));      // n_cand and n_left
    hipLaunchKernelGGL(ru_heads, dim3((unsigned)((m + 2047) / 2048)), dim3(256), 0, stream, keys2.as<uint64_t>(), idx2.as<uint32_t>(), cur, m, rep.as<uint32_t>(),
                       start_at.as<uint32_t>(), left.as<uint8_t>(), cand.as<uint32_t>(), n_cand);
    SCFQ_SCRATCH_CHK(g_rerr, hipGetLastError());
    size_t bytes = tmp_bytes;
    SCFQ_SCRATCH_CHK(g_rerr, rocprim::inclusive_scan(tmp.p, bytes, start_at.as<uint32_t>(), head.as<uint32_t>(), (size_t)m, rocprim::maximum<uint32_t>(), stream));
    // (the launch covers the worst case; its blocks stride over the candidates there are)
    hipLaunchKernelGGL(ru_compare, group_blocks(m), dim3(256), 0, stream, a, b, pl, idx2.as<uint32_t>(), cur, head.as<uint32_t>(), cand.as<uint32_t>(), n_cand,
                       rep.as<uint32_t>(), left.as<uint8_t>(), collisions);
    SCFQ_SCRATCH_CHK(g_rerr, hipGetLastError());
    bytes = tmp_bytes;
    if (cur) SCFQ_SCRATCH_CHK(g_rerr, rocprim::select(tmp.p, bytes, cur, left.as<uint8_t>(), next.as<uint32_t>(), n_left, (size_t)m, stream));
    else SCFQ_SCRATCH_CHK(g_rerr, rocprim::select(tmp.p, bytes, rocprim::counting_iterator<uint32_t>(0), left.as<uint8_t>(), next.as<uint32_t>(), n_left, (size_t)m, stream));
    uint32_t back[2] = {0, 0};
    SCFQ_SCRATCH_CHK(g_rerr, hipMemcpyAsync(back, n_cand, 8, hipMemcpyDeviceToHost, stream));
    SCFQ_SCRATCH_CHK(g_rerr, hipStreamSynchronize(stream));
    if (back[0]) ++rounds;
    if (back[1] >= m) { std::snprintf(g_rerr, sizeof g_rerr, "round %u left %u of %llu entries over", round, back[1], (unsigned long long)m); return SCFQ_EHIP; }
    m = back[1];
    cur = next.as<uint32_t>();
  }
  clk.mark(3);
  hipLaunchKernelGGL(ru_class_sizes, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, stream, idx2.as<uint32_t>(), rep.as<uint32_t>(), units, copies.as<uint32_t>());
  SCFQ_SCRATCH_CHK(g_rerr, hipGetLastError());
  clk.mark(4);
  clk2.mark(0);
  hipLaunchKernelGGL(ru_lengths, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, stream, a, b, pl, rep.as<uint32_t>(), copies.as<uint32_t>(), recs, n_groups,
                     gs.len(), counters.as<unsigned long long>());
  SCFQ_SCRATCH_CHK(g_rerr, hipGetLastError());
  if ((rc = gs.scan(tmp.p, tmp_bytes))) return rc;
  clk2.mark(1);
  // the sizes and the statistics come back first: pool memory for the outputs is taken to fit, and a caller's buffer that is too small
  // is known here
  uint64_t coll = 0;
  std::vector<uint64_t> h(kWordsOut);
  if ((rc = gs.read_totals())) return rc;
  SCFQ_SCRATCH_CHK(g_rerr, hipMemcpyAsync(h.data(), counters.p, kWordsOut * 8, hipMemcpyDeviceToHost, stream));
  SCFQ_SCRATCH_CHK(g_rerr, hipMemcpyAsync(&coll, collisions, 8, hipMemcpyDeviceToHost, stream));
  SCFQ_SCRATCH_CHK(g_rerr, hipStreamSynchronize(stream));
  st->out1_bytes = gs.total[0]; st->out2_bytes = gs.total[1];
  st->units_out = h[kUnitsOut];
  st->reads_out = paired ? 2 * h[kUnitsOut] : h[kUnitsOut];
  st->duplicate_units = units - h[kUnitsOut];
  st->duplicated_classes = h[kDupClasses];
  st->max_copies = h[kMaxCopies];
  st->bases_in = h[kBasesIn]; st->bases_out = h[kBasesOut];
  st->collisions = coll;
  st->rounds = rounds;
  if (hist_host) std::memcpy(hist_host, h.data() + kCounters, SCFQ_RMDUP_HIST_BINS * 8);
  const scfq_reads::Placement put = scfq_reads::place_outputs(gs, scfq_reads::kOutNames, dst, own_outputs, check_caps, recs_small, own, stream, g_rerr);
  if (put.rc) return put.rc;
  if (put.out[0].p || put.out[1].p) {
    hipLaunchKernelGGL(ru_write, dim3((unsigned)((n_groups + kWaves - 1) / kWaves)), dim3(64 * kWaves), 0, stream, a, b, pl, rep.as<uint32_t>(), n_groups,
                       gs.off(), put.out[0], put.out[1]);
    SCFQ_SCRATCH_CHK(g_rerr, hipGetLastError());
  }
  clk2.mark(2);
  SCFQ_SCRATCH_CHK(g_rerr, hipStreamSynchronize(stream));
  g_stage_ms[0] = index_ms;
  for (int k = 0; k < 4; ++k) g_stage_ms[1 + k] = clk.between(k, k + 1);
  g_stage_ms[5] = clk2.between(0, 1);
  g_stage_ms[6] = clk2.between(1, 2);
  if (recs_small) {
    std::snprintf(g_rerr, sizeof g_rerr, "the per-unit table holds %llu entries, the input has %llu units", (unsigned long long)recs_cap, (unsigned long long)units);
    return SCFQ_EARG;
  }
  return put.verdict;      // (SCFQ_EARG for an output that is too small: place_outputs has left the text)
}

}  // namespace

extern "C" {

const char* scfq_rmdup_error_detail(void) { return g_rerr; }

int scfq_debug_rmdup_stages(double* ms, uint32_t cap) {
  for (uint32_t k = 0; ms && k < cap && k < kStages; ++k) ms[k] = g_stage_ms[k];
  return (int)kStages;
}

int scfq_format_rmdup_stats_tsv(const scfq_rmdup_stats* s, int header, char* buf, uint64_t cap) {
  static const char kNames[] = "units_in\tunits_out\tduplicate_units\tduplicate_pct\tduplicated_classes\tmax_copies\treads_in\treads_out\tpairs\tunpaired\t"
                               "bases_in\tbases_out\tout1_bytes\tout2_bytes";
  if (header) return scfq_reads::copy_text(kNames, (int)sizeof kNames - 1, buf, cap);
  if (!s) return SCFQ_EARG;
  // floor(10000 d / u): the product may pass 64 bits
  uint64_t pct = 0;
  if (s->units_in) {
    const unsigned __int128 x = (unsigned __int128)s->duplicate_units * 10000u / s->units_in;
    pct = (uint64_t)x;
  }
  const uint64_t tail[] = {s->duplicated_classes, s->max_copies, s->reads_in, s->reads_out, s->pairs, s->unpaired, s->bases_in, s->bases_out, s->out1_bytes,
                           s->out2_bytes};
  char tmp[512];
  int m = std::snprintf(tmp, sizeof tmp, "%llu\t%llu\t%llu\t%llu.%02llu", (unsigned long long)s->units_in, (unsigned long long)s->units_out,
                        (unsigned long long)s->duplicate_units, (unsigned long long)(pct / 100), (unsigned long long)(pct % 100));
  for (const uint64_t x : tail) m += std::snprintf(tmp + m, sizeof tmp - m, "\t%llu", (unsigned long long)x);
  return scfq_reads::copy_text(tmp, m, buf, cap);
}

int scfq_format_rmdup_rec_tsv(uint64_t unit, const scfq_rmdup_rec* rec, char* buf, uint64_t cap) {
  static const char kNames[] = "unit\trep\tcopies";
  if (!rec) return scfq_reads::copy_text(kNames, (int)sizeof kNames - 1, buf, cap);
  char tmp[96];
  const int m = std::snprintf(tmp, sizeof tmp, "%llu\t%u\t%u", (unsigned long long)unit, (unsigned)rec->rep, (unsigned)rec->copies);
  return scfq_reads::copy_text(tmp, m, buf, cap);
}

int scfq_rmdup_buffers(const void* r1, uint64_t n1, const void* r2, uint64_t n2, int is_device, const scfq_rmdup_opts* opts, scfq_rmdup_rec* recs, uint64_t recs_cap,
                       uint64_t* hist_host, void* out1, uint64_t cap1, void* out2, uint64_t cap2, int out_is_device, scfq_rmdup_stats* stats) {
  g_rerr[0] = '\0';
  Params prm;
  Mode mode;
  if (!args_ok(opts, stats, prm) || (!r1 && n1) || (!r2 && n2) || (!out1 && cap1) || (!out2 && cap2) || (!recs && recs_cap)) return SCFQ_EARG;
  if (!mode_ok(prm, r2 || n2, out2 != nullptr, "buffer", mode)) return SCFQ_EARG;
  scfq_scratch::clear_keep_size(stats);
  Dest dst[2] = {{static_cast<uint8_t*>(out1), cap1, out1 != nullptr}, {static_cast<uint8_t*>(out2), cap2, out2 != nullptr}};
  const bool any_out = out1 || out2, direct = any_out && out_is_device, recs_on_device = recs && out_is_device;
  scfq_scratch::ResidentInput in1, in2;
  int rc = in1.from_buffer(r1, n1, is_device != 0, is_device || direct || recs_on_device, g_rerr);
  if (rc) return rc;
  // (a host buffer's copy is waited for inside; device memory of the caller is ordered before in1's stream above)
  if (mode == Mode::two && (rc = in2.from_buffer(r2, n2, is_device != 0, false, g_rerr))) return rc;
  DevBuf own[2], recs_keep;
  rc = rmdup_device(in1.d_in, in1.n, in2.d_in, in2.n, mode, prm, recs_on_device ? recs : nullptr, recs != nullptr, recs_cap, true, recs_keep, hist_host,
                    /*own_outputs=*/!direct, dst, own, /*check_caps=*/true, stats, in1.stream);
  if (rc) return finish(in1, rc);
  if (recs && !recs_on_device && stats->units_in)
    SCFQ_SCRATCH_CHK(g_rerr, hipMemcpyAsync(recs, recs_keep.p, stats->units_in * sizeof(scfq_rmdup_rec), hipMemcpyDeviceToHost, in1.stream));
  if (!direct) {
    const uint64_t bytes[2] = {stats->out1_bytes, stats->out2_bytes};
    if ((rc = scfq_reads::outputs_to_host(2, dst, own, bytes, in1.stream, g_rerr))) return rc;
  }
  SCFQ_SCRATCH_CHK(g_rerr, hipStreamSynchronize(in1.stream));
  for (DevBuf& o : own) o.drop();
  recs_keep.drop();
  in1.mark_clean();      // (the last act was to wait for the stream; behind it lie returns of pool memory only)
  return SCFQ_OK;
}

int scfq_rmdup_files(const char* path1, const char* path2, const scfq_rmdup_opts* opts, const scfq_opts* ropts, int out1_fd, int out2_fd, int per_read_fd,
                     uint64_t* hist_host, scfq_rmdup_stats* stats) {
  g_rerr[0] = '\0';
  Params prm;
  Mode mode;
  if (!path1 || !args_ok(opts, stats, prm)) return SCFQ_EARG;
  if (!mode_ok(prm, path2 != nullptr, out2_fd >= 0, "file", mode)) return SCFQ_EARG;
  scfq_scratch::clear_keep_size(stats);
  scfq_scratch::ResidentInput in1, in2;
  int rc = in1.from_file(path1, ropts, g_rerr);
  if (rc) return rc;
  if (mode == Mode::two && (rc = in2.from_file(path2, ropts, g_rerr))) return rc;      // (staged when this returns)
  const int fd[2] = {out1_fd, out2_fd};
  Dest dst[2] = {{nullptr, 0, out1_fd >= 0}, {nullptr, 0, out2_fd >= 0}};
  DevBuf own[2], recs_keep;
  rc = rmdup_device(in1.d_in, in1.n, in2.d_in, in2.n, mode, prm, nullptr, per_read_fd >= 0, 0, false, recs_keep, hist_host, /*own_outputs=*/true, dst, own,
                    /*check_caps=*/false, stats, in1.stream);
  if (rc) return finish(in1, rc);
  if (per_read_fd >= 0 && stats->units_in) {
    // the table comes to the host whole; the rows leave in pieces of about 1 MiB
    const uint64_t units = stats->units_in;
    std::vector<scfq_rmdup_rec> recs(units);
    SCFQ_SCRATCH_CHK(g_rerr, hipMemcpyAsync(recs.data(), recs_keep.p, units * sizeof(scfq_rmdup_rec), hipMemcpyDeviceToHost, in1.stream));
    SCFQ_SCRATCH_CHK(g_rerr, hipStreamSynchronize(in1.stream));
    std::string text;
    char row[96];
    for (uint64_t i = 0; i < units; ++i) {
      const int m = scfq_format_rmdup_rec_tsv(i, &recs[i], row, sizeof row);
      text.append(row, (size_t)m);
      text.push_back('\n');
      if (text.size() >= (1u << 20) || i + 1 == units) {
        if ((rc = scfq_fdwrite::write_all(per_read_fd, reinterpret_cast<const uint8_t*>(text.data()), text.size(), g_rerr))) return finish(in1, rc);
        text.clear();
      }
    }
  }
  const uint64_t bytes[2] = {stats->out1_bytes, stats->out2_bytes};
  return scfq_reads::outputs_to_fds(2, own, bytes, fd, in1, g_rerr);
}

}  // extern "C"

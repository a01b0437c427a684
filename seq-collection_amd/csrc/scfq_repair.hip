// scfq_repair.hip — `sc fq-repair` on the MI355X (gfx950): R1 and R2 re-paired by read name.
// Not in the reference; definitions in include/sc_fqcount.h.
//
// Both inputs sit in HBM whole.  The units are the union: R1's records 0 .. reads1 - 1, then R2's records reads1 .. reads1 + reads2 - 1.
//   K5  line index            (scfq_scratch::build_line_index) of each input
//   P1  rp_names              a thread per unit: the name's (start, length), stored for every later step.  The lane owns its record's
//                             search for the first blank or tab, over 8-byte words; no cross-lane operation is in that loop
//   F   rp_same               reads1 == reads2 only: eight lanes per record compare name i of R1 with name i of R2; the number of
//                             records that differ comes back.  None: the table is the identity (path 0) and only R1's names are
//                             put into classes, for `repeated`
//   P2  rp_hash               eight lanes per unit over the name's words (hh_word / hh_final); key = the hash's low hash_bits bits
//       radix sort            rocprim::radix_sort_pairs of (key, unit), stable
//   rounds, as fq-rmdup's U2 + U3 (rp_heads is ru_heads, rp_compare is ru_compare with one key per unit): rep[u] = the first unit
//                             that carries u's name
//   M   second sort           (rep, unit), stable: every class is one run, its R1 members ascending, then its R2 members ascending
//       rp_runs + two scans   run starts (max-scan: every entry's run start s) and "is an R1 record" (exclusive sum c)
//       rp_mates              a thread per entry.  An R2 entry at place p has a = c[p] - c[s] R1 records in its run and is R2's rank
//                             r = p - s - a; its mate, if r < a, is the entry at s + r.  It writes both table entries.  An R1 entry
//                             only counts whether it repeats.  No loop over a run
//   L   rocprim::select       the table's R1 half without the singles: pair number k -> R2 record j
//       rp_lengths            out1 / singles1 per group of 32 R1 records, singles2 per group of 32 R2 records, out2 per group of 32
//                             pair numbers; one exclusive scan per output
//   W1  rp_write              sequential (sc_write's shape): a wave per group echoes R1's records into out1 or singles1 and R2's
//                             unmatched records into singles2
//   W2  rp_gather             X3's shape: a wave per group of 32 pair numbers, sources anywhere in R2, one sequential destination
// W1 and W2 compare the four totals with the capacities before they store anything.  An index read from a sorted array, the list or
// the table is compared with its bound before it is used.  Everything is integer / byte work; there is no CPU fallback.
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

static_assert(sizeof(scfq_repair_stats) == 24 * 8 && sizeof(scfq_repair_opts) == 32, "the ABI's sizes");
static_assert(scfq_reads::kMaxOutputs >= 4, "four outputs");

namespace {

constexpr uint32_t kStages = 9;
thread_local char g_perr[scfq_scratch::kErrBytes] = "";
thread_local double g_stage_ms[kStages] = {0, 0, 0, 0, 0, 0, 0, 0, 0};

using scfq_reads::Dest;
using scfq_reads::DevBuf;
using scfq_reads::finish;

constexpr uint32_t kLanes = 8;                 // lanes of a group: one unit of P2 and F, one candidate of the rounds
constexpr uint32_t kMaxBlocks = 8192;          // of P2, F and the compare: the blocks stride
constexpr uint32_t kGroup = kRecGroup;         // records of a group: one wave of a writer, one entry of the scans
constexpr uint32_t kWaves = 4;                 // groups of a block of a writer
constexpr uint32_t kDefaultHashBits = 40;      // (fq-rmdup's: five radix passes)
constexpr uint32_t kNone = SCFQ_REPAIR_SINGLE;
constexpr uint64_t kSeed = 0x5DEECE66D1CE4E5Bull;
constexpr const char* kNames[4] = {"out1", "out2", "singles1", "singles2"};
enum { kRowOut1 = 0, kRowOut2, kRowSingles1, kRowSingles2, kRows };
enum { kPairs = 0, kMoved, kRepeated1, kRepeated2, kCounters };

struct RpUnits {          // the union of the two inputs' records
  RecInput a, b;
  uint64_t reads1, reads2;
};

// a name: len bytes at p, of which `room` bytes (>= len) lie inside the input
struct RpKey {
  const uint8_t* p;
  uint64_t len, room;
};

// word w of a key (8 w < len), little-endian, zero behind the key.  No byte outside [p, p + room) is touched
__device__ __forceinline__ uint64_t key_word(const RpKey& k, uint64_t w) {
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

// the stored name of unit u (u below the units there are)
__device__ __forceinline__ RpKey name_of(const RpUnits& un, const uint64_t* nstart, const uint64_t* nlen, uint64_t u) {
  const RecInput& in = u < un.reads1 ? un.a : un.b;
  uint64_t s = nstart[u], len = nlen[u];
  if (s > in.n) s = in.n;                                  // (what P1 stored lies inside the input: checked all the same)
  if (len > in.n - s) len = in.n - s;
  return RpKey{in.base + s, len, in.n - s};
}

// the bytes of x that are 0: the lowest bit set is exact (a borrow only reaches bytes above the first 0 byte)
__device__ __forceinline__ uint64_t zero_bytes(uint64_t x) { return (x - 0x0101010101010101ull) & ~x & 0x8080808080808080ull; }

// P1.  nstart: the name's first byte as an offset into the unit's own input; nlen: its bytes
__global__ __launch_bounds__(256) void rp_names(RpUnits un, uint64_t units, uint64_t* nstart, uint64_t* nlen) {
  const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= units) return;
  const bool second = u >= un.reads1;
  const RecInput& in = second ? un.b : un.a;
  uint64_t s, e;
  text_span(in, 4 * (second ? u - un.reads1 : u), s, e);
  if (e > s) ++s;                                          // the first byte goes, whatever it is
  const RpKey k = {in.base + s, e - s, in.n - s};
  uint64_t len = k.len;
  const uint64_t words = (k.len + 7) / 8;
  for (uint64_t w = 0; w < words; ++w) {                   // (this lane's own search: nothing in here crosses lanes)
    const uint64_t v = key_word(k, w);
    // (the bytes behind the text are 0 in v: neither a blank nor a tab)
    const uint64_t hit = zero_bytes(v ^ 0x2020202020202020ull) | zero_bytes(v ^ 0x0909090909090909ull);
    if (hit) { len = 8 * w + ((uint64_t)__builtin_ctzll(hit) >> 3); break; }
  }
  if (len >= 2 && k.p[len - 2] == '/' && (k.p[len - 1] == '1' || k.p[len - 1] == '2')) len -= 2;
  nstart[u] = s;
  nlen[u] = len;
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
__device__ __forceinline__ uint64_t group_hash(const RpKey& k, uint32_t g, bool on) {
  uint32_t A = 0, B = 0;
  const uint64_t words = on ? (k.len + 7) / 8 : 0;
  for (uint64_t w = g; w < words; w += kLanes) {
    const uint64_t v = key_word(k, w);
    scfq_hdrhash::hh_word((uint32_t)v, (uint32_t)(v >> 32), (uint32_t)w, A, B);
  }
  A = group_sum(A);
  B = group_sum(B);
  return scfq_hdrhash::hh_final(A, B, k.len, kSeed ^ ((uint64_t)(B >> 24) << 40));
}

// are the two keys different?  By the group; `on` is the group's.  Lengths first, then the words
__device__ __forceinline__ bool group_differs(const RpKey& x, const RpKey& y, uint32_t g, bool on) {
  uint32_t diff = on && x.len != y.len;
  const uint64_t words = (on && !diff) ? (x.len + 7) / 8 : 0;
  for (uint64_t w = g; w < words; w += kLanes) diff |= key_word(x, w) != key_word(y, w);
  return group_or(diff) != 0;
}

// the sum of v over the block's 256 threads into *dst: one atomic per block.  Every thread of the block gets here
__device__ __forceinline__ void block_add(uint64_t v, unsigned long long* dst, uint64_t (&sh)[4]) {
  const uint64_t s = wave_sum(v);
  __syncthreads();                                         // (sh may still be read from the call before)
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint64_t t = sh[0] + sh[1] + sh[2] + sh[3];
    if (t) atomicAdd(dst, (unsigned long long)t);
  }
}

// F.  *differing: the records i whose names in R1 and R2 differ (reads1 == reads2 == count)
__global__ __launch_bounds__(256) void rp_same(RpUnits un, uint64_t count, const uint64_t* nstart, const uint64_t* nlen, unsigned long long* differing) {
  __shared__ uint64_t sh[4];
  const uint32_t g = threadIdx.x & (kLanes - 1);
  const uint64_t per_step = (uint64_t)gridDim.x * (256 / kLanes);
  const uint64_t steps = (count + per_step - 1) / per_step;               // (kernel-uniform: the shuffles are never divergent)
  uint64_t i = (uint64_t)blockIdx.x * (256 / kLanes) + threadIdx.x / kLanes;
  uint64_t diff = 0;
  const RpKey none = {nullptr, 0, 0};
  for (uint64_t step = 0; step < steps; ++step, i += per_step) {
    const bool on = i < count;
    const bool d = group_differs(on ? name_of(un, nstart, nlen, i) : none, on ? name_of(un, nstart, nlen, un.reads1 + i) : none, g, on);
    if (on && g == 0 && d) ++diff;
  }
  block_add(diff, differing, sh);
}

// P2
__global__ __launch_bounds__(256) void rp_hash(RpUnits un, uint64_t units, const uint64_t* nstart, const uint64_t* nlen, uint32_t hash_bits, uint64_t* keys,
                                              uint32_t* idx) {
  const uint32_t g = threadIdx.x & (kLanes - 1);
  const uint64_t per_step = (uint64_t)gridDim.x * (256 / kLanes);
  const uint64_t steps = (units + per_step - 1) / per_step;               // (the same for every lane)
  uint64_t u = (uint64_t)blockIdx.x * (256 / kLanes) + threadIdx.x / kLanes;
  for (uint64_t step = 0; step < steps; ++step, u += per_step) {
    const bool on = u < units;
    const uint64_t h = group_hash(on ? name_of(un, nstart, nlen, u) : RpKey{nullptr, 0, 0}, g, on);
    if (on && g == 0) {
      keys[u] = hash_bits >= 64 ? h : h & ((1ull << hash_bits) - 1ull);
      idx[u] = (uint32_t)u;
    }
  }
}

// Run starts of a round (fq-rmdup's U2, which does not depend on what a key is; a copy, so that fq-rmdup's kernels stay as they are).
// list: the sorted positions of this round, ascending (nullptr: all of them); m entries.  start_at[t]: t for an entry that starts a
// run, else 0.  left[t] = 0.  The candidates (entries that start no run) are compacted into cand, counted in *n_cand.
__global__ __launch_bounds__(256) void rp_heads(const uint64_t* keys_sorted, const uint32_t* idx_sorted, const uint32_t* list, uint64_t m, uint64_t units,
                                               uint32_t* rep, uint32_t* start_at, uint8_t* left, uint32_t* cand, uint32_t* n_cand) {
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
      const uint32_t before = t == 0 ? 0u : (list ? list[t - 1] : (uint32_t)(t - 1));
      bool start = true;
      if (p < units && before < units) {                   // (a position that is none starts a run of its own and is no candidate)
        start = t == 0 || keys_sorted[p] != keys_sorted[before];
        const uint32_t unit = idx_sorted[p];
        if (start && unit < units) rep[unit] = unit;
      }
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
    // (every candidate is one of the m entries, so before + its rank stays below m, the entries cand holds)
    if ((bal[j] >> lane) & 1ull) cand[before + (uint32_t)__popcll(bal[j] & ((1ull << lane) - 1))] = (uint32_t)(base + 256u * j + threadIdx.x);
    for (uint32_t k = w; k < 4; ++k) before += wave_cnt[j][k];
  }
}

// The compare of a round (fq-rmdup's U3 with one key per unit).  cand: entries t of the list; head[t]: the entry that starts t's run
__global__ __launch_bounds__(256) void rp_compare(RpUnits un, uint64_t units, const uint64_t* nstart, const uint64_t* nlen, const uint32_t* idx_sorted,
                                                 const uint32_t* list, uint64_t m, const uint32_t* head, const uint32_t* cand, const uint32_t* n_cand, uint32_t* rep,
                                                 uint8_t* left, unsigned long long* collisions) {
  __shared__ uint64_t sh[4];
  const uint32_t g = threadIdx.x & (kLanes - 1);
  const uint64_t total = std::min<uint64_t>(*n_cand, m);
  const uint64_t per_step = (uint64_t)gridDim.x * (256 / kLanes);
  const uint64_t steps = (total + per_step - 1) / per_step;               // (kernel-uniform)
  uint64_t c = (uint64_t)blockIdx.x * (256 / kLanes) + threadIdx.x / kLanes;
  uint64_t missed = 0;
  const RpKey none = {nullptr, 0, 0};
  for (uint64_t step = 0; step < steps; ++step, c += per_step) {
    bool on = c < total;
    uint32_t t = 0, mine = 0, heads = 0;
    if (on) {
      t = cand[c];
      on = t < m;
      const uint32_t ht = on ? head[t] : 0u;
      on = on && ht < m;
      const uint32_t pm = on ? (list ? list[t] : t) : 0u, ph = on ? (list ? list[ht] : ht) : 0u;
      on = on && pm < units && ph < units;
      if (on) { mine = idx_sorted[pm]; heads = idx_sorted[ph]; }
      on = on && mine < units && heads < units;
    }
    const bool differs = group_differs(on ? name_of(un, nstart, nlen, mine) : none, on ? name_of(un, nstart, nlen, heads) : none, g, on);
    if (on && g == 0) {
      if (differs) { left[t] = 1; ++missed; }
      else rep[mine] = heads;
    }
  }
  block_add(missed, collisions, sh);
}

// M.  rep_sorted / order: the second sort's keys and units.  start_at[p]: p where a run starts, else 0; is_r1[p]: the entry is a record of R1
__global__ __launch_bounds__(256) void rp_runs(const uint32_t* rep_sorted, const uint32_t* order, uint64_t units, uint64_t reads1, uint32_t* start_at, uint32_t* is_r1) {
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= units) return;
  start_at[p] = (p == 0 || rep_sorted[p] != rep_sorted[p - 1]) ? (uint32_t)p : 0u;
  is_r1[p] = order[p] < reads1 ? 1u : 0u;
}

// M.  head[p]: the start of p's run; r1_before[p]: the R1 entries in front of p.  table: reads1 + reads2 words, all kNone before
__global__ __launch_bounds__(256) void rp_mates(const uint32_t* order, const uint32_t* head, const uint32_t* r1_before, uint64_t units, uint64_t reads1, uint32_t* table,
                                               unsigned long long* counters) {
  __shared__ uint64_t sh[4];
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint64_t c[kCounters] = {0, 0, 0, 0};
  if (p < units) {
    const uint64_t u = order[p], s = head[p];
    if (u < units && s <= p) {
      if (u < reads1) {
        c[kRepeated1] = p != s;                            // (R1's members lead their run: the first one is the name's first record)
      } else {
        const uint64_t a = (uint64_t)r1_before[p] - r1_before[s];
        if (a <= p - s) {
          const uint64_t r = p - s - a;                    // this record's rank among R2's records of the name
          c[kRepeated2] = r != 0;
          if (r < a) {
            const uint64_t i = order[s + r], j = u - reads1;           // (s + r < s + a <= p)
            if (i < reads1) {
              table[i] = (uint32_t)j;
              table[u] = (uint32_t)i;
              c[kPairs] = 1;
              c[kMoved] = i != j;
            }
          }
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kCounters; ++k) block_add(c[k], &counters[k], sh);
}

// path 0: the table is the identity; rep (of R1's records alone) says which names repeat
__global__ __launch_bounds__(256) void rp_identity(const uint32_t* rep, uint64_t reads1, uint32_t* table, unsigned long long* counters) {
  __shared__ uint64_t sh[4];
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint64_t repeated = 0;
  if (i < reads1) {
    table[i] = (uint32_t)i;
    table[reads1 + i] = (uint32_t)i;
    repeated = rep[i] != (uint32_t)i;
  }
  block_add(repeated, &counters[kRepeated1], sh);
}

struct IsMate {
  __host__ __device__ bool operator()(const uint32_t& v) const { return v != kNone; }
};

// L.  pair_r2[k]: the R2 record of pair number k, *n_pairs of them.  group_len: kRows arrays of n_groups + 1 entries
__global__ __launch_bounds__(256) void rp_lengths(RpUnits un, const uint32_t* table, const uint32_t* pair_r2, const uint32_t* n_pairs, uint64_t n_groups,
                                                 uint64_t* group_len) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t pairs = std::min<uint64_t>(*n_pairs, std::min(un.reads1, un.reads2));
  uint64_t len[kRows] = {0, 0, 0, 0};
  if (t < un.reads1) len[table[t] != kNone ? kRowOut1 : kRowSingles1] = echo_len(un.a, t);
  if (t < un.reads2 && table[un.reads1 + t] == kNone) len[kRowSingles2] = echo_len(un.b, t);
  if (t < pairs) {
    const uint64_t j = pair_r2[t];
    if (j < un.reads2) len[kRowOut2] = echo_len(un.b, j);
  }
  store_group_len(len[kRowOut1], kRowOut1, t, un.reads1, n_groups, group_len);
  store_group_len(len[kRowOut2], kRowOut2, t, pairs, n_groups, group_len);
  store_group_len(len[kRowSingles1], kRowSingles1, t, un.reads1, n_groups, group_len);
  store_group_len(len[kRowSingles2], kRowSingles2, t, un.reads2, n_groups, group_len);
}

struct RpOuts { RecOut o[kRows]; };

__device__ __forceinline__ bool all_fit(const RpOuts& out, uint64_t n_groups, const uint64_t* group_off) {
  bool fit = true;
#pragma unroll
  for (int k = 0; k < kRows; ++k) fit = fit && output_fits(out.o[k], k, n_groups, group_off);
  return fit;
}

// where this lane's record goes in output `row`: group g's offset and the lengths in front of it in the group (place_units for one row)
__device__ __forceinline__ uint64_t place_in_row(uint64_t len, uint32_t row, uint64_t g, uint64_t n_groups, const uint64_t* group_off, uint32_t lane) {
  uint64_t v = len;
#pragma unroll
  for (int o = 1; o < (int)kGroup; o <<= 1) {
    const uint64_t up = __shfl_up((unsigned long long)v, o, 64);
    if (lane >= (uint32_t)o) v += up;
  }
  return v + group_off[(uint64_t)row * (n_groups + 1) + g] - len;
}

// W1.  group_off: the kRows scanned arrays of rp_lengths' layout
__global__ __launch_bounds__(64 * kWaves) void rp_write(RpUnits un, const uint32_t* table, uint64_t n_groups, const uint64_t* group_off, RpOuts out) {
  const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // (when one result is more than its output holds, nothing is written to any)
  if (!all_fit(out, n_groups, group_off)) return;
  const uint64_t g = (uint64_t)blockIdx.x * kWaves + wave;
  if (g >= n_groups) return;
  const uint64_t r0 = g * kGroup;
  // R1's group: matched records to out1, the others to singles1
  if (r0 < un.reads1) {
    const uint32_t count = (uint32_t)std::min<uint64_t>(kGroup, un.reads1 - r0);
    uint64_t len = 0;
    bool matched = false;
    if (lane < count) { len = echo_len(un.a, r0 + lane); matched = table[r0 + lane] != kNone; }
    const uint64_t at1 = place_in_row(matched ? len : 0, kRowOut1, g, n_groups, group_off, lane);
    const uint64_t at3 = place_in_row(matched ? 0 : len, kRowSingles1, g, n_groups, group_off, lane);
    const uint64_t mask = __builtin_amdgcn_ballot_w64(matched);
    for (uint32_t q = 0; q < count; ++q) {
      const bool mq = (mask >> q) & 1ull;                  // (wave-uniform)
      const uint64_t l = bcast(len, q), w = bcast(mq ? at1 : at3, q);
      uint8_t* const dst = mq ? out.o[kRowOut1].p : out.o[kRowSingles1].p;
      if (dst && l) echo_record(un.a, r0 + q, dst + w, l, lane);
    }
  }
  // R2's group: the unmatched records to singles2
  if (r0 < un.reads2 && out.o[kRowSingles2].p) {
    const uint32_t count = (uint32_t)std::min<uint64_t>(kGroup, un.reads2 - r0);
    uint64_t len = 0;
    if (lane < count && table[un.reads1 + r0 + lane] == kNone) len = echo_len(un.b, r0 + lane);
    const uint64_t at = place_in_row(len, kRowSingles2, g, n_groups, group_off, lane);
    const uint64_t mask = __builtin_amdgcn_ballot_w64(len != 0);
    for (uint32_t q = 0; q < count; ++q) {
      if (!((mask >> q) & 1ull)) continue;                 // (wave-uniform)
      echo_record(un.b, r0 + q, out.o[kRowSingles2].p + bcast(at, q), bcast(len, q), lane);
    }
  }
}

// W2.  A wave per group of kGroup pair numbers
__global__ __launch_bounds__(64 * kWaves) void rp_gather(RpUnits un, const uint32_t* pair_r2, uint64_t pairs, uint64_t n_groups, const uint64_t* group_off, RpOuts out) {
  const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (!all_fit(out, n_groups, group_off) || !out.o[kRowOut2].p) return;
  const uint64_t g = (uint64_t)blockIdx.x * kWaves + wave;
  const uint64_t k0 = g * kGroup;
  if (g >= n_groups || k0 >= pairs) return;
  const uint32_t count = (uint32_t)std::min<uint64_t>(kGroup, pairs - k0);
  uint64_t len = 0, j = un.reads2;
  if (lane < count) j = pair_r2[k0 + lane];
  if (j < un.reads2) len = echo_len(un.b, j);              // (a number that is no record of R2: nothing, as in rp_lengths)
  const uint64_t at = place_in_row(len, kRowOut2, g, n_groups, group_off, lane);
  for (uint32_t q = 0; q < count; ++q) {
    const uint64_t l = bcast(len, q), jq = bcast(j, q), w = bcast(at, q);
    if (l) echo_record(un.b, jq, out.o[kRowOut2].p + w, l, lane);
  }
}

struct Params { uint32_t flags, hash_bits; };

bool args_ok(const scfq_repair_opts* opts, const scfq_repair_stats* st, Params& p) {
  if (!st || st->struct_size != sizeof(scfq_repair_stats)) return false;
  p = Params{0, kDefaultHashBits};
  if (opts) {
    if (opts->struct_size != sizeof(scfq_repair_opts)) return false;
    p.flags = opts->flags;
    if (p.flags) { std::snprintf(g_perr, sizeof g_perr, "unknown flag bits 0x%x", p.flags); return false; }
    if (opts->hash_bits > 64) { std::snprintf(g_perr, sizeof g_perr, "hash_bits %u is not in 0 .. 64", opts->hash_bits); return false; }
    if (opts->hash_bits) p.hash_bits = opts->hash_bits;
    if (opts->reserved[0] || opts->reserved[1] || opts->reserved[2] || opts->reserved[3]) {
      std::snprintf(g_perr, sizeof g_perr, "the reserved words are %u, %u, %u and %u, not 0", opts->reserved[0], opts->reserved[1], opts->reserved[2],
                    opts->reserved[3]);
      return false;
    }
  }
  return true;
}

// HIP events around the stages (StageClock holds five)
struct Events {
  static constexpr int kN = 9;
  bool on;
  hipStream_t s;
  hipEvent_t ev[kN] = {};
  bool set[kN] = {};
  Events(hipStream_t stream, bool enabled) : on(enabled), s(stream) {
    if (on) for (auto& e : ev) if (hipEventCreate(&e) != hipSuccess) { on = false; break; }
  }
  Events(const Events&) = delete;
  Events& operator=(const Events&) = delete;
  ~Events() { for (auto e : ev) if (e) (void)hipEventDestroy(e); }
  void mark(int k) { if (on && hipEventRecord(ev[k], s) == hipSuccess) set[k] = true; }
  double between(int a, int b) {
    float ms = 0;
    return (on && set[a] && set[b] && hipEventElapsedTime(&ms, ev[a], ev[b]) == hipSuccess) ? (double)ms : 0.0;
  }
};

uint32_t bits_for(uint64_t n) {          // the bits that hold 0 .. n - 1, one at the least
  uint32_t bits = 1;
  while (bits < 32 && (1ull << bits) < n) ++bits;
  return bits;
}

dim3 group_blocks(uint64_t items) { return dim3((unsigned)std::min<uint64_t>(std::max<uint64_t>((items + 256 / kLanes - 1) / (256 / kLanes), 1), kMaxBlocks)); }
dim3 thread_blocks(uint64_t items) { return dim3((unsigned)std::max<uint64_t>((items + 255) / 256, 1)); }

// what the classes need: allocated once for the units there are
struct Work {
  DevBuf nstart, nlen, keys, keys2, idx, idx2, rep, start_at, head, cand, left, list[2], words, tmp;
  size_t tmp_bytes = 0, sort_bytes = 0;
};

// rep[u] for the units 0 .. units - 1: hash, sort and rounds.  *rounds: the rounds that had a candidate
int build_classes(const RpUnits& un, uint64_t units, uint32_t hash_bits, Work& w, hipStream_t stream, Events& clk, uint64_t* rounds) {
  int rc = SCFQ_OK;
  uint32_t* const n_cand = w.words.as<uint32_t>();
  unsigned long long* const collisions = reinterpret_cast<unsigned long long*>(w.words.as<uint32_t>() + 2);
  hipLaunchKernelGGL(rp_hash, group_blocks(units), dim3(256), 0, stream, un, units, w.nstart.as<uint64_t>(), w.nlen.as<uint64_t>(), hash_bits, w.keys.as<uint64_t>(),
                     w.idx.as<uint32_t>());
  SCFQ_SCRATCH_CHK(g_perr, hipGetLastError());
  clk.mark(3);
  size_t bytes = w.tmp_bytes;
  SCFQ_SCRATCH_CHK(g_perr, rocprim::radix_sort_pairs(w.tmp.p, bytes, w.keys.as<uint64_t>(), w.keys2.as<uint64_t>(), w.idx.as<uint32_t>(), w.idx2.as<uint32_t>(),
                                                     (size_t)units, 0u, hash_bits, stream));
  clk.mark(4);
  // the rounds.  m: the entries of this round's list (round 0: every sorted position; list[] is not used)
  uint64_t m = units;
  const uint32_t* cur = nullptr;
  for (uint32_t round = 0; m > 0; ++round) {
    DevBuf& next = w.list[round & 1];
    if ((rc = next.alloc(m * 4, stream, g_perr))) return rc;             // (at most m - 1 are left over)
    SCFQ_SCRATCH_CHK(g_perr, hipMemsetAsync(n_cand, 0, 8, stream));      // n_cand and n_left
    hipLaunchKernelGGL(rp_heads, dim3((unsigned)((m + 2047) / 2048)), dim3(256), 0, stream, w.keys2.as<uint64_t>(), w.idx2.as<uint32_t>(), cur, m, units,
                       w.rep.as<uint32_t>(), w.start_at.as<uint32_t>(), w.left.as<uint8_t>(), w.cand.as<uint32_t>(), n_cand);
    SCFQ_SCRATCH_CHK(g_perr, hipGetLastError());
    bytes = w.tmp_bytes;
    SCFQ_SCRATCH_CHK(g_perr, rocprim::inclusive_scan(w.tmp.p, bytes, w.start_at.as<uint32_t>(), w.head.as<uint32_t>(), (size_t)m, rocprim::maximum<uint32_t>(), stream));
    hipLaunchKernelGGL(rp_compare, group_blocks(m), dim3(256), 0, stream, un, units, w.nstart.as<uint64_t>(), w.nlen.as<uint64_t>(), w.idx2.as<uint32_t>(), cur, m,
                       w.head.as<uint32_t>(), w.cand.as<uint32_t>(), n_cand, w.rep.as<uint32_t>(), w.left.as<uint8_t>(), collisions);
    SCFQ_SCRATCH_CHK(g_perr, hipGetLastError());
    bytes = w.tmp_bytes;
    if (cur) SCFQ_SCRATCH_CHK(g_perr, rocprim::select(w.tmp.p, bytes, cur, w.left.as<uint8_t>(), next.as<uint32_t>(), n_cand + 1, (size_t)m, stream));
    else SCFQ_SCRATCH_CHK(g_perr, rocprim::select(w.tmp.p, bytes, rocprim::counting_iterator<uint32_t>(0), w.left.as<uint8_t>(), next.as<uint32_t>(), n_cand + 1, (size_t)m, stream));
    uint32_t back[2] = {0, 0};
    SCFQ_SCRATCH_CHK(g_perr, hipMemcpyAsync(back, n_cand, 8, hipMemcpyDeviceToHost, stream));
    SCFQ_SCRATCH_CHK(g_perr, hipStreamSynchronize(stream));
    if (back[0]) ++*rounds;
    if (back[1] >= m) { std::snprintf(g_perr, sizeof g_perr, "round %u left %u of %llu entries over", round, back[1], (unsigned long long)m); return SCFQ_EHIP; }
    m = back[1];
    cur = next.as<uint32_t>();
  }
  clk.mark(5);
  return SCFQ_OK;
}

// table_keep: where the table stays for the caller of this function (reads1 + reads2 words), unless the caller's is too small (then no
// table is kept and nothing is written)
int repair_device(const uint8_t* d1, uint64_t n1, const uint8_t* d2, uint64_t n2, const Params& prm, bool want_table, uint64_t table_cap, bool check_table,
                  DevBuf& table_keep, bool own_outputs, Dest dst[kRows], DevBuf own[kRows], bool check_caps, scfq_repair_stats* st, hipStream_t stream) {
  for (double& m : g_stage_ms) m = 0;
  st->input_bytes1 = n1;
  st->input_bytes2 = n2;
  st->flags = prm.flags; st->hash_bits = prm.hash_bits;
  scfq_overlap::Indexed ix;
  int rc = scfq_overlap::index_inputs(d1, n1, d2, n2, false, stream, g_perr, ix, &g_stage_ms[0]);
  st->lines1 = ix.lines1; st->lines2 = ix.lines2;
  st->reads1 = ix.reads1; st->reads2 = ix.reads2;
  if (rc) return rc;
  const uint64_t reads1 = ix.reads1, reads2 = ix.reads2, units = reads1 + reads2;       // (each below 2^31: units < 2^32 - 1)
  const bool table_small = check_table && want_table && table_cap < units;
  auto small_table = [&]() {
    std::snprintf(g_perr, sizeof g_perr, "the per-record table holds %llu entries, the inputs have %llu records", (unsigned long long)table_cap, (unsigned long long)units);
    return (int)SCFQ_EARG;
  };
  st->in_step = reads1 == reads2;
  if (units == 0) return SCFQ_OK;           // (four empty outputs: they fit into anything; in step)
  const uint64_t n_groups = (std::max(reads1, reads2) + kGroup - 1) / kGroup;
  Work w;
  DevBuf rep_sorted, order, r1_before, pair_r2, group_len, group_off, counters;
  scfq_reads::GroupScan gs(kRows, n_groups, group_len, group_off, stream, g_perr);
  if ((rc = table_keep.alloc(units * 4, stream, g_perr)) || (rc = w.nstart.alloc(units * 8, stream, g_perr)) || (rc = w.nlen.alloc(units * 8, stream, g_perr)) ||
      (rc = w.keys.alloc(units * 8, stream, g_perr)) || (rc = w.keys2.alloc(units * 8, stream, g_perr)) || (rc = w.idx.alloc(units * 4, stream, g_perr)) ||
      (rc = w.idx2.alloc(units * 4, stream, g_perr)) || (rc = w.rep.alloc(units * 4, stream, g_perr)) || (rc = w.start_at.alloc(units * 4, stream, g_perr)) ||
      (rc = w.head.alloc(units * 4, stream, g_perr)) || (rc = w.cand.alloc(units * 4, stream, g_perr)) || (rc = w.left.alloc(units, stream, g_perr)) ||
      (rc = w.words.alloc(32, stream, g_perr)) || (rc = rep_sorted.alloc(units * 4, stream, g_perr)) || (rc = order.alloc(units * 4, stream, g_perr)) ||
      (rc = r1_before.alloc(units * 4, stream, g_perr)) || (rc = pair_r2.alloc(std::max<uint64_t>(reads1, 1) * 4, stream, g_perr)) || (rc = gs.alloc()) ||
      (rc = counters.alloc(kCounters * 8, stream, g_perr)))
    return rc;
  uint32_t* const table = table_keep.as<uint32_t>();
  // words: [0] the candidates of the round, [1] what it leaves over, [2 .. 3] the collisions, [4 .. 5] the records F found different,
  // [6] the pairs the select counted
  uint32_t* const n_pairs = w.words.as<uint32_t>() + 6;
  unsigned long long* const differing = reinterpret_cast<unsigned long long*>(w.words.as<uint32_t>() + 4);
  const uint32_t rep_bits = bits_for(units);
  size_t sort2_bytes = 0, scan_bytes = 0, max_bytes = 0, sum_bytes = 0, select_bytes = 0, pick_bytes = 0;
  SCFQ_SCRATCH_CHK(g_perr, rocprim::radix_sort_pairs(nullptr, w.sort_bytes, w.keys.as<uint64_t>(), w.keys2.as<uint64_t>(), w.idx.as<uint32_t>(), w.idx2.as<uint32_t>(),
                                                     (size_t)units, 0u, prm.hash_bits, stream));
  SCFQ_SCRATCH_CHK(g_perr, rocprim::radix_sort_pairs(nullptr, sort2_bytes, w.rep.as<uint32_t>(), rep_sorted.as<uint32_t>(), w.idx.as<uint32_t>(), order.as<uint32_t>(),
                                                     (size_t)units, 0u, rep_bits, stream));
  if ((rc = gs.scratch_bytes(&scan_bytes))) return rc;
  SCFQ_SCRATCH_CHK(g_perr, rocprim::inclusive_scan(nullptr, max_bytes, w.start_at.as<uint32_t>(), w.head.as<uint32_t>(), (size_t)units, rocprim::maximum<uint32_t>(), stream));
  SCFQ_SCRATCH_CHK(g_perr, rocprim::exclusive_scan(nullptr, sum_bytes, w.cand.as<uint32_t>(), r1_before.as<uint32_t>(), 0u, (size_t)units, rocprim::plus<uint32_t>(), stream));
  SCFQ_SCRATCH_CHK(g_perr, rocprim::select(nullptr, select_bytes, rocprim::counting_iterator<uint32_t>(0), w.left.as<uint8_t>(), w.cand.as<uint32_t>(), n_pairs,
                                           (size_t)units, stream));
  SCFQ_SCRATCH_CHK(g_perr, rocprim::select(nullptr, pick_bytes, table, pair_r2.as<uint32_t>(), n_pairs, (size_t)std::max<uint64_t>(reads1, 1), IsMate(), stream));
  w.tmp_bytes = std::max({w.sort_bytes, sort2_bytes, scan_bytes, max_bytes, sum_bytes, select_bytes, pick_bytes});
  if ((rc = w.tmp.alloc(w.tmp_bytes, stream, g_perr))) return rc;
  static const bool timing = scfq_scratch::env_switch("SCFQ_REPAIR_TIMING");
  Events clk(stream, timing);
  const char* fast_env = std::getenv("SCFQ_REPAIR_FAST");               // (read per call)
  const bool try_fast = reads1 == reads2 && !(fast_env && std::strcmp(fast_env, "0") == 0);
  SCFQ_SCRATCH_CHK(g_perr, hipMemsetAsync(counters.p, 0, kCounters * 8, stream));
  if ((rc = gs.zero())) return rc;
  SCFQ_SCRATCH_CHK(g_perr, hipMemsetAsync(w.words.p, 0, 32, stream));
  SCFQ_SCRATCH_CHK(g_perr, hipMemsetAsync(table, 0xFF, units * 4, stream));
  const RpUnits un = {RecInput{d1, n1, ix.off1.as<uint64_t>(), ix.lines1, ix.cr1}, RecInput{d2, n2, ix.off2.as<uint64_t>(), ix.lines2, ix.cr2}, reads1, reads2};
  clk.mark(0);
  hipLaunchKernelGGL(rp_names, thread_blocks(units), dim3(256), 0, stream, un, units, w.nstart.as<uint64_t>(), w.nlen.as<uint64_t>());
  SCFQ_SCRATCH_CHK(g_perr, hipGetLastError());
  clk.mark(1);
  bool fast = false;
  if (try_fast) {
    hipLaunchKernelGGL(rp_same, group_blocks(reads1), dim3(256), 0, stream, un, reads1, w.nstart.as<uint64_t>(), w.nlen.as<uint64_t>(), differing);
    SCFQ_SCRATCH_CHK(g_perr, hipGetLastError());
    uint64_t back = 0;
    SCFQ_SCRATCH_CHK(g_perr, hipMemcpyAsync(&back, differing, 8, hipMemcpyDeviceToHost, stream));
    SCFQ_SCRATCH_CHK(g_perr, hipStreamSynchronize(stream));
    fast = back == 0;
  }
  clk.mark(2);
  uint64_t rounds = 0;
  // path 0 puts R1's names alone into classes: `repeated` does not depend on the path, and in step R2 repeats where R1 does
  if ((rc = build_classes(un, fast ? reads1 : units, prm.hash_bits, w, stream, clk, &rounds))) return rc;
  if (fast) {
    hipLaunchKernelGGL(rp_identity, thread_blocks(reads1), dim3(256), 0, stream, w.rep.as<uint32_t>(), reads1, table, counters.as<unsigned long long>());
    SCFQ_SCRATCH_CHK(g_perr, hipGetLastError());
  } else {
    size_t bytes = w.tmp_bytes;
    SCFQ_SCRATCH_CHK(g_perr, rocprim::radix_sort_pairs(w.tmp.p, bytes, w.rep.as<uint32_t>(), rep_sorted.as<uint32_t>(), w.idx.as<uint32_t>(), order.as<uint32_t>(),
                                                       (size_t)units, 0u, rep_bits, stream));
    // (start_at, head and cand are free again: the rounds are over.  cand holds "is an R1 record")
    hipLaunchKernelGGL(rp_runs, thread_blocks(units), dim3(256), 0, stream, rep_sorted.as<uint32_t>(), order.as<uint32_t>(), units, reads1, w.start_at.as<uint32_t>(),
                       w.cand.as<uint32_t>());
    SCFQ_SCRATCH_CHK(g_perr, hipGetLastError());
    bytes = w.tmp_bytes;
    SCFQ_SCRATCH_CHK(g_perr, rocprim::inclusive_scan(w.tmp.p, bytes, w.start_at.as<uint32_t>(), w.head.as<uint32_t>(), (size_t)units, rocprim::maximum<uint32_t>(), stream));
    bytes = w.tmp_bytes;
    SCFQ_SCRATCH_CHK(g_perr, rocprim::exclusive_scan(w.tmp.p, bytes, w.cand.as<uint32_t>(), r1_before.as<uint32_t>(), 0u, (size_t)units, rocprim::plus<uint32_t>(), stream));
    hipLaunchKernelGGL(rp_mates, thread_blocks(units), dim3(256), 0, stream, order.as<uint32_t>(), w.head.as<uint32_t>(), r1_before.as<uint32_t>(), units, reads1, table,
                       counters.as<unsigned long long>());
    SCFQ_SCRATCH_CHK(g_perr, hipGetLastError());
  }
  clk.mark(6);
  if (reads1) {
    size_t bytes = w.tmp_bytes;
    SCFQ_SCRATCH_CHK(g_perr, rocprim::select(w.tmp.p, bytes, table, pair_r2.as<uint32_t>(), n_pairs, (size_t)reads1, IsMate(), stream));
  }
  hipLaunchKernelGGL(rp_lengths, thread_blocks(std::max(reads1, reads2)), dim3(256), 0, stream, un, table, pair_r2.as<uint32_t>(), n_pairs, n_groups, gs.len());
  SCFQ_SCRATCH_CHK(g_perr, hipGetLastError());
  if ((rc = gs.scan(w.tmp.p, w.tmp_bytes))) return rc;
  clk.mark(7);
  // the sizes and the statistics come back first: pool memory for the outputs is taken to fit, and a caller's buffer that is too small
  // is known here
  uint64_t h[kCounters] = {0, 0, 0, 0}, coll = 0;
  uint32_t listed = 0;
  if ((rc = gs.read_totals())) return rc;
  SCFQ_SCRATCH_CHK(g_perr, hipMemcpyAsync(h, counters.p, kCounters * 8, hipMemcpyDeviceToHost, stream));
  SCFQ_SCRATCH_CHK(g_perr, hipMemcpyAsync(&coll, w.words.as<uint32_t>() + 2, 8, hipMemcpyDeviceToHost, stream));
  SCFQ_SCRATCH_CHK(g_perr, hipMemcpyAsync(&listed, n_pairs, 4, hipMemcpyDeviceToHost, stream));
  SCFQ_SCRATCH_CHK(g_perr, hipStreamSynchronize(stream));
  const uint64_t pairs = fast ? reads1 : h[kPairs];
  if (pairs != listed || pairs > std::min(reads1, reads2)) {
    std::snprintf(g_perr, sizeof g_perr, "%llu pairs were matched, the table lists %u", (unsigned long long)pairs, listed);
    return SCFQ_EHIP;
  }
  st->pairs = pairs;
  st->singles1 = reads1 - pairs; st->singles2 = reads2 - pairs;
  st->moved = fast ? 0 : h[kMoved];
  st->repeated1 = h[kRepeated1];
  st->repeated2 = fast ? h[kRepeated1] : h[kRepeated2];
  st->in_step = reads1 == reads2 && pairs == reads1 && st->moved == 0;
  st->collisions = coll;
  st->rounds = rounds;
  st->path = fast ? 0 : 1;
  st->out1_bytes = gs.total[kRowOut1]; st->out2_bytes = gs.total[kRowOut2];
  st->singles1_bytes = gs.total[kRowSingles1]; st->singles2_bytes = gs.total[kRowSingles2];
  const scfq_reads::Placement put = scfq_reads::place_outputs(gs, kNames, dst, own_outputs, check_caps, table_small, own, stream, g_perr);
  if (put.rc) return put.rc;
  RpOuts out;
  bool any = false;
  for (int k = 0; k < kRows; ++k) { out.o[k] = put.out[k]; any = any || put.out[k].p; }
  if (any) {
    hipLaunchKernelGGL(rp_write, dim3((unsigned)((n_groups + kWaves - 1) / kWaves)), dim3(64 * kWaves), 0, stream, un, table, n_groups, gs.off(), out);
    SCFQ_SCRATCH_CHK(g_perr, hipGetLastError());
    const uint64_t pair_groups = (pairs + kGroup - 1) / kGroup;
    if (out.o[kRowOut2].p && pair_groups) {
      hipLaunchKernelGGL(rp_gather, dim3((unsigned)((pair_groups + kWaves - 1) / kWaves)), dim3(64 * kWaves), 0, stream, un, pair_r2.as<uint32_t>(), pairs, n_groups,
                         gs.off(), out);
      SCFQ_SCRATCH_CHK(g_perr, hipGetLastError());
    }
  }
  clk.mark(8);
  SCFQ_SCRATCH_CHK(g_perr, hipStreamSynchronize(stream));
  for (int k = 1; k < (int)kStages; ++k) g_stage_ms[k] = clk.between(k - 1, k);
  if (table_small) { table_keep.drop(); return small_table(); }
  return put.verdict;      // (SCFQ_EARG for an output that is too small: place_outputs has left the text)
}

}  // namespace

extern "C" {

const char* scfq_repair_error_detail(void) { return g_perr; }

int scfq_debug_repair_stages(double* ms, uint32_t cap) {
  for (uint32_t k = 0; ms && k < cap && k < kStages; ++k) ms[k] = g_stage_ms[k];
  return (int)kStages;
}

int scfq_format_repair_stats_tsv(const scfq_repair_stats* s, int header, char* buf, uint64_t cap) {
  static const char kCols[] = "reads1\treads2\tpairs\tsingles1\tsingles2\tmoved\tin_step\trepeated1\trepeated2\tout1_bytes\tout2_bytes\tsingles1_bytes\tsingles2_bytes";
  if (header) return scfq_reads::copy_text(kCols, (int)sizeof kCols - 1, buf, cap);
  if (!s) return SCFQ_EARG;
  const uint64_t cols[] = {s->reads1, s->reads2, s->pairs, s->singles1, s->singles2, s->moved, s->in_step, s->repeated1, s->repeated2, s->out1_bytes, s->out2_bytes,
                           s->singles1_bytes, s->singles2_bytes};
  char tmp[512];
  int m = 0;
  for (const uint64_t x : cols) m += std::snprintf(tmp + m, sizeof tmp - m, m ? "\t%llu" : "%llu", (unsigned long long)x);
  return scfq_reads::copy_text(tmp, m, buf, cap);
}

int scfq_format_repair_rec_tsv(uint32_t input, uint64_t record, uint32_t mate, char* buf, uint64_t cap) {
  static const char kCols[] = "input\trecord\tmate";
  if (!input) return scfq_reads::copy_text(kCols, (int)sizeof kCols - 1, buf, cap);
  char tmp[96];
  const int m = mate == kNone ? std::snprintf(tmp, sizeof tmp, "%u\t%llu\t-", (unsigned)input, (unsigned long long)record)
                              : std::snprintf(tmp, sizeof tmp, "%u\t%llu\t%u", (unsigned)input, (unsigned long long)record, (unsigned)mate);
  return scfq_reads::copy_text(tmp, m, buf, cap);
}

int scfq_repair_buffers(const void* r1, uint64_t n1, const void* r2, uint64_t n2, int is_device, const scfq_repair_opts* opts, uint32_t* table, uint64_t table_cap,
                        void* out1, uint64_t cap1, void* out2, uint64_t cap2, void* singles1, uint64_t cap_s1, void* singles2, uint64_t cap_s2, int out_is_device,
                        scfq_repair_stats* stats) {
  g_perr[0] = '\0';
  Params prm;
  if (!args_ok(opts, stats, prm) || (!r1 && n1) || (!r2 && n2) || (!out1 && cap1) || (!out2 && cap2) || (!singles1 && cap_s1) || (!singles2 && cap_s2) ||
      (!table && table_cap))
    return SCFQ_EARG;
  scfq_scratch::clear_keep_size(stats);
  void* const outs[kRows] = {out1, out2, singles1, singles2};
  const uint64_t caps[kRows] = {cap1, cap2, cap_s1, cap_s2};
  Dest dst[kRows];
  bool any_out = false;
  for (int k = 0; k < kRows; ++k) { dst[k] = Dest{static_cast<uint8_t*>(outs[k]), caps[k], outs[k] != nullptr}; any_out = any_out || outs[k]; }
  const bool direct = any_out && out_is_device, table_on_device = table && out_is_device;
  scfq_scratch::ResidentInput in1, in2;
  int rc = in1.from_buffer(r1, n1, is_device != 0, is_device || direct || table_on_device, g_perr);
  if (rc) return rc;
  // (a host buffer's copy is waited for inside; device memory of the caller is ordered before in1's stream above)
  if ((rc = in2.from_buffer(r2, n2, is_device != 0, false, g_perr))) return rc;
  DevBuf own[kRows], table_keep;
  rc = repair_device(in1.d_in, in1.n, in2.d_in, in2.n, prm, table != nullptr, table_cap, true, table_keep, /*own_outputs=*/!direct, dst, own, /*check_caps=*/true, stats,
                     in1.stream);
  if (rc) return finish(in1, rc);
  const uint64_t units = stats->reads1 + stats->reads2;
  if (table && units)
    SCFQ_SCRATCH_CHK(g_perr, hipMemcpyAsync(table, table_keep.p, units * 4, table_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, in1.stream));
  if (!direct) {
    const uint64_t bytes[kRows] = {stats->out1_bytes, stats->out2_bytes, stats->singles1_bytes, stats->singles2_bytes};
    if ((rc = scfq_reads::outputs_to_host(kRows, dst, own, bytes, in1.stream, g_perr))) return rc;
  }
  SCFQ_SCRATCH_CHK(g_perr, hipStreamSynchronize(in1.stream));
  for (DevBuf& o : own) o.drop();
  table_keep.drop();
  in1.mark_clean();      // (the last act was to wait for the stream; behind it lie returns of pool memory only)
  return SCFQ_OK;
}

int scfq_repair_files(const char* path1, const char* path2, const scfq_repair_opts* opts, const scfq_opts* ropts, int out1_fd, int out2_fd, int singles1_fd,
                      int singles2_fd, int per_read_fd, scfq_repair_stats* stats) {
  g_perr[0] = '\0';
  Params prm;
  if (!args_ok(opts, stats, prm)) return SCFQ_EARG;
  if (!path1 || !path2) { std::snprintf(g_perr, sizeof g_perr, "fq-repair takes two files"); return SCFQ_EARG; }
  scfq_scratch::clear_keep_size(stats);
  scfq_scratch::ResidentInput in1, in2;
  int rc = in1.from_file(path1, ropts, g_perr);
  if (rc) return rc;
  if ((rc = in2.from_file(path2, ropts, g_perr))) return rc;      // (staged when this returns)
  const int fd[kRows] = {out1_fd, out2_fd, singles1_fd, singles2_fd};
  Dest dst[kRows];
  for (int k = 0; k < kRows; ++k) dst[k] = Dest{nullptr, 0, fd[k] >= 0};
  DevBuf own[kRows], table_keep;
  rc = repair_device(in1.d_in, in1.n, in2.d_in, in2.n, prm, per_read_fd >= 0, 0, false, table_keep, /*own_outputs=*/true, dst, own, /*check_caps=*/false, stats,
                     in1.stream);
  if (rc) return finish(in1, rc);
  const uint64_t units = stats->reads1 + stats->reads2;
  if (per_read_fd >= 0 && units) {
    // the table comes to the host whole; the rows leave in pieces of about 1 MiB
    std::vector<uint32_t> table(units);
    SCFQ_SCRATCH_CHK(g_perr, hipMemcpyAsync(table.data(), table_keep.p, units * 4, hipMemcpyDeviceToHost, in1.stream));
    SCFQ_SCRATCH_CHK(g_perr, hipStreamSynchronize(in1.stream));
    std::string text;
    char row[96];
    for (uint64_t u = 0; u < units; ++u) {
      const bool second = u >= stats->reads1;
      const int m = scfq_format_repair_rec_tsv(second ? 2u : 1u, second ? u - stats->reads1 : u, table[u], row, sizeof row);
      text.append(row, (size_t)m);
      text.push_back('\n');
      if (text.size() >= (1u << 20) || u + 1 == units) {
        if ((rc = scfq_fdwrite::write_all(per_read_fd, reinterpret_cast<const uint8_t*>(text.data()), text.size(), g_perr))) return finish(in1, rc);
        text.clear();
      }
    }
  }
  const uint64_t bytes[kRows] = {stats->out1_bytes, stats->out2_bytes, stats->singles1_bytes, stats->singles2_bytes};
  return scfq_reads::outputs_to_fds(kRows, own, bytes, fd, in1, g_perr);
}

}  // extern "C"

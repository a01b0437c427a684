// scfq_kcount.hip — `sc fq-kcount` on the MI355X (gfx950): k-mer counts for 13 <= k <= 32 in an open-addressing table in HBM.
// Not in the reference; definitions in include/sc_fqcount.h.
//
// The whole (inflated) input sits in HBM, as for fq-kmers, whose definitions and partition this file keeps:
//   K5  line index            (scfq_scratch::build_line_index) of each input
//   H0  kc_clear              every slot (key, count) of the table to (kEmpty, 0)
//   H1  kc_count              the hot path, once per input and pass.  km_count's geometry: 16-byte chunks on the ADDRESS grid, a chunk per
//                             lane, 512-thread blocks, 8 KiB steps, the same run of consecutive steps for every block, one binary search in
//                             line_off per block; the line of every byte follows from the '\n' the block sees.  A lane loads bytes
//                             [o, o + 48): 47 of them are the sixteen windows of up to 32 letters that START in its chunk, the 48th only
//                             says whether a '\r' in byte 46 stands before a '\n'.  The 47 bytes become 94 bits of 2-bit codes in two words
//                             (byte 0 on top), in canonical mode also their complement with byte 0 at the bottom; "not A C G T" and "no
//                             text" are 64-bit masks, and smear_down(mask, k) decides window or not and skipped or not for all sixteen
//                             starts at once.  Window i's key is a funnel shift of the two words (a second one and a minimum in canonical
//                             mode).  Equal keys of consecutive windows are one run — inside a lane, and across the lanes of a wave whose
//                             sixteen windows are all one key: poly-G tails would put a thousand adds per wave on one slot otherwise.
//                             A run (key, times) goes to slot mix64(key) & (slots - 1): a relaxed load of the slot's key (atomics execute
//                             at the memory side, the plain load is what the cache serves), a 64-bit compare-and-swap when it is empty,
//                             a no-return 64-bit add of `times` on the count next to it when the slot is the key's, else the next slot.
//                             EVERY LOOP IS BOUNDED: a run probes at most max_probe slots, then it sets `failed`; a lane reads that word
//                             before every run it inserts, and the block leaves at its next barrier once a lane saw it set.  Nothing
//                             spins, and no block waits for another.  A failed pass is thrown away whole.
//                             The key of 32 T (plain mode) equals kEmpty: it is counted in a register and a word of its own.
//   H2  kc_finish             one pass over the slots: distinct, unique, max_count and the sum of the counts (= kmers)
//   H3  kc_hist               scfq_kcount_hist: one pass; the first 8192 bins in LDS, global atomics for the rest
//   H4  kc_select             scfq_kcount_dump: the slots that qualify, counted, then written through a wave-aggregated cursor, a
//                             piece of the table (kDumpPiece slots) per launch
//   H5  kc_query              scfq_kcount_query: a lane per key, the same bounded probe, kQueryPiece keys per launch
// H3 – H5 work in 8 MiB of scratch that belong to the table and are allocated with it: a reader takes no device memory of its own.
// Everything is integer / byte work; there is no CPU fallback.
#include "../../include/sc_fqcount.h"
#include "../../include/sc_fqcount_debug.h"

#include <hip/hip_runtime.h>

#include "scfq_kcount_host.hpp"
#include "scfq_kcount_internal.hpp"
#include "scfq_record_device.hpp"
#include "scfq_scratch.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <new>
#include <vector>

struct scfq_kcount {
  void* slots_dev = nullptr;       // KcSlot[slots], hipMalloc
  void* scratch_dev = nullptr;     // behind the slots, in the same allocation: kScratchBytes for the readers (below), then their cursor
  void* cursor_dev = nullptr;
  mutable std::mutex mu;           // one reader (hist, dump, query) at a time: they share the scratch
  uint64_t slots = 0;
  uint64_t ones = 0;               // count of the key that equals kEmpty
  uint64_t distinct = 0, passes = 0;      // of the summary, for the readers of scfq_kcount_internal.hpp
  uint32_t k = 0, flags = 0, max_probe = 0;
};

namespace {

using namespace scfq_kcount_host;
using scfq_scratch::DevBuf;

thread_local char g_cerr[scfq_scratch::kErrBytes] = "";
thread_local double g_stage_ms[4] = {0, 0, 0, 0};

constexpr uint32_t kKcThreads = 512;                 // a chunk per lane and step
constexpr uint32_t kKcWaves = kKcThreads / 64;
constexpr uint32_t kKcMaxBlocks = 1024;
constexpr uint32_t kKcHistLds = 8192;                // bins of H3 that live in LDS
// The readers' device memory belongs to the table and is allocated with it: the bins of scfq_kcount_hist, the rows of a piece
// of scfq_kcount_dump, the keys and counts of a piece of scfq_kcount_query.  (Why not pool scratch per call: DESIGN.md, fq-kcount.)
constexpr uint64_t kScratchBytes = kMaxBins * 8;
constexpr uint64_t kDumpPiece = kScratchBytes / sizeof(scfq_kmer_count);      // slots per piece: every one of them may qualify
constexpr uint64_t kQueryPiece = kScratchBytes / 16;                          // keys per piece: 8 bytes of key and 8 of count each
static_assert(16 + SCFQ_KCOUNT_MAX_K - 1 <= 47 && 2 * SCFQ_KCOUNT_MAX_K <= 64, "47 bytes per lane, a 64-bit key");

struct alignas(16) KcSlot { unsigned long long key, count; };

enum : uint32_t { kStWindows = 0, kStSkipped = 1, kStShort = 2, kStOnes = 3, kStDistinct = 4, kStUnique = 5, kStMax = 6, kStSum = 7, kStWords = 8 };

// OR of x >> 0 .. x >> (k - 1): bit i says whether any of bits i .. i + k - 1 is set
__device__ __forceinline__ uint64_t smear_down(uint64_t x, uint32_t k) {
  uint32_t done = 1;
  while (done < k) {
    const uint32_t sh = done < k - done ? done : k - done;
    x |= x >> sh;
    done += sh;
  }
  return x;
}

__device__ __forceinline__ KcSlot load_slot(const KcSlot* t, uint64_t s) {
  const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(t + s);
  return KcSlot{v.x, v.y};
}

// H0
__global__ __launch_bounds__(256) void kc_clear(KcSlot* table, uint64_t slots) {
  for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * 256)
    *reinterpret_cast<ulonglong2*>(table + s) = make_ulonglong2(kEmpty, 0ull);
}

// H1.  chunks: 16-byte chunks of the address grid that hold a byte of the input or the position behind its last byte;
// steps_per_block * kKcThreads of them per block.  shift: address of the input mod 16.  slot_mask: slots - 1.
template <bool kCanon>
__global__ __launch_bounds__(kKcThreads) void kc_count(const uint8_t* base, uint64_t n, const uint64_t* line_off, uint64_t lines, uint32_t shift,
                                                      bool has_cr, uint32_t k, bool merge, uint64_t chunks, uint64_t steps_per_block, KcSlot* table,
                                                      uint64_t slot_mask, uint32_t max_probe, uint32_t* failed, unsigned long long* stats) {
  __shared__ uint32_t wave_nl[2][kKcWaves];
  __shared__ uint64_t first_line;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t kmask = key_mask(k);
  const uint32_t down = 64 - 2 * k;                                  // a window on top of a word -> its key

  const uint64_t step0 = (uint64_t)blockIdx.x * steps_per_block;
  const uint64_t c_first = step0 * kKcThreads;                       // (c_first < chunks: the grid is sized so)
  if (threadIdx.x == 0) {
    // the line of the block's first byte: the last j < lines with line_off[j] <= p0
    const uint64_t p0 = 16 * c_first > shift ? 16 * c_first - shift : 0;
    uint64_t a = 0, h = lines;
    while (a < h) {
      const uint64_t m = a + (h - a) / 2;
      if (line_off[m] <= p0) a = m + 1; else h = m;
    }
    first_line = a - 1;                                              // (line_off[0] = 0 <= p0)
  }
  __syncthreads();
  uint64_t line_run = first_line;                                    // line of the step's first byte
  uint64_t n_windows = 0, n_skipped = 0, n_short = 0, n_ones = 0;
  int saw_failed = 0;                                                // this lane read `failed` set, or set it

  // a run of `times` windows of one key into the table
  auto emit = [&](uint64_t key, uint32_t times) {
    if (key == kEmpty) { n_ones += times; return; }                  // (k = 32, plain mode: 32 T)
    if (saw_failed || __atomic_load_n(failed, __ATOMIC_RELAXED)) { saw_failed = 1; return; }
    uint64_t slot = mix64(key) & slot_mask;
    for (uint32_t p = 0; p < max_probe; ++p) {
      unsigned long long cur = __atomic_load_n(&table[slot].key, __ATOMIC_RELAXED);      // (a slot that holds a key keeps it)
      if (cur == kEmpty) cur = atomicCAS(&table[slot].key, (unsigned long long)kEmpty, (unsigned long long)key);
      if (cur == kEmpty || cur == key) {
        atomicAdd(&table[slot].count, (unsigned long long)times);    // (the value is not used: no return)
        return;
      }
      slot = (slot + 1) & slot_mask;
    }
    atomicOr(failed, 1u);
    saw_failed = 1;
  };

  for (uint64_t st = 0; st < steps_per_block; ++st) {
    const uint64_t c0 = c_first + st * kKcThreads;
    if (c0 >= chunks) break;                                         // (block-uniform)
    const uint64_t c = c0 + threadIdx.x;
    const int64_t o = 16 * (int64_t)c - (int64_t)shift;              // offset of this lane's byte 0; bytes [o, o + 48) are looked at
    uint32_t w[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) w[i] = 0;
    uint64_t outside = (1ull << 48) - 1ull;                          // bytes that are not the input's
    if (c < chunks) {
      if (o >= 0 && o + 48 <= (int64_t)n) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const uint4 v = *reinterpret_cast<const uint4*>(base + o + 16 * q);      // (aligned: shift + o = 0 mod 16)
          w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
        }
        outside = 0;
      } else {
        // the input's first chunk and its last ones: only its own bytes are read
#pragma unroll
        for (int i = 0; i < 48; ++i) {
          const int64_t p = o + i;
          if (p >= 0 && p < (int64_t)n) {
            w[i >> 2] |= (uint32_t)base[p] << (8 * (i & 3));
            outside &= ~(1ull << i);
          }
        }
      }
    }
    // bytes 0 .. 46: the 2-bit words with byte 0 (byte 32) on top, their complement with byte 0 (byte 32) at the bottom; the masks of 48
    uint64_t hi = 0, lo = 0, rlo = 0, rhi = 0, bad = 0, nl = 0, cr = 0;
#pragma unroll
    for (int i = 0; i < 48; ++i) {
      const uint32_t b = (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
      const uint32_t code = ((b >> 1) & 3u) ^ ((b >> 2) & 1u);                       // A C G T -> 0 1 2 3
      const bool ok = ((0x54474341u >> (8 * code)) & 0xffu) == b;
      if (i < 32) {
        hi |= (uint64_t)code << (62 - 2 * i);
        if (kCanon) rlo |= (uint64_t)(3u - code) << (2 * i);
      } else if (i < 47) {
        lo |= (uint64_t)code << (62 - 2 * (i - 32));
        if (kCanon) rhi |= (uint64_t)(3u - code) << (2 * (i - 32));
      }
      bad |= (uint64_t)(ok ? 0u : 1u) << i;
      nl |= (uint64_t)(b == '\n' ? 1u : 0u) << i;
      cr |= (uint64_t)(b == '\r' ? 1u : 0u) << i;
    }
    nl &= ~outside;
    uint64_t no_text = nl | outside;
    if (has_cr) no_text |= cr & (nl >> 1);                           // the '\r' directly before a real '\n'

    // the line of this lane's byte 0
    const uint32_t nl16 = (uint32_t)nl & 0xffffu;
    uint32_t incl = (uint32_t)__builtin_popcount(nl16);
    const uint32_t own = incl;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d, 64);
      if (lane >= (uint32_t)d) incl += up;
    }
    if (lane == 63) wave_nl[st & 1][wave] = incl;
    if (__syncthreads_or(saw_failed)) break;                         // (block-uniform: the pass has failed, here or in another block)
    uint32_t before = incl - own, step_nl = 0;
#pragma unroll
    for (uint32_t v = 0; v < kKcWaves; ++v) {
      const uint32_t t = wave_nl[st & 1][v];
      if (v < wave) before += t;
      step_nl += t;
    }
    const uint64_t line0 = line_run + before;
    line_run += step_nl;

    // the bytes of this chunk that lie in a sequence line (4i + 1), and the sequence lines that end in it
    uint32_t in_seq = 0, seq_ends = 0;
    {
      uint32_t rest = 0xffffu, ph = (uint32_t)line0 & 3u, m = nl16;
      while (m) {
        const uint32_t bit = (uint32_t)__builtin_ctz(m);
        m &= m - 1;
        const uint32_t seg = rest & ((2u << bit) - 1u);
        if (ph == 1) { in_seq |= seg; seq_ends |= 1u << bit; }
        rest &= ~seg;
        ph = (ph + 1) & 3u;
      }
      if (ph == 1) in_seq |= rest;
    }
    // short_lines: by the lane that holds the line's '\n', or the position behind the input when its last line has none
    while (seq_ends) {
      const uint32_t bit = (uint32_t)__builtin_ctz(seq_ends);
      seq_ends &= seq_ends - 1;
      const uint64_t j = line0 + (uint32_t)__builtin_popcount(nl16 & ((1u << bit) - 1u));
      uint64_t s, e;
      line_span(base, n, line_off, j, s, e, has_cr);
      if (e - s < k) ++n_short;
    }
    if (c < chunks && n > 0 && (int64_t)n >= o && (int64_t)n < o + 16 && base[n - 1] != '\n') {
      const uint64_t j = line0 + own;                                // (= lines - 1)
      if ((j & 3u) == 1) {
        uint64_t s, e;
        line_span(base, n, line_off, j, s, e, has_cr);
        if (e - s < k) ++n_short;
      }
    }

    // windows that start in this chunk: k bytes of text of one sequence line; a k-mer when all of them are A C G T
    const uint32_t win = in_seq & ~(uint32_t)smear_down(no_text, k) & 0xffffu;
    const uint32_t masked = (uint32_t)smear_down(bad, k);
    const uint32_t km = win & ~masked;
    n_windows += (uint32_t)__builtin_popcount(win);
    n_skipped += (uint32_t)__builtin_popcount(win & masked);

    uint64_t run_key = 0;
    uint32_t run_cnt = 0;
    // (not unrolled: the probe loop of emit stands once in the code, and the shifts are by a register either way)
    for (uint32_t rest = km; rest; rest &= rest - 1) {
      const uint32_t s2 = 2u * (uint32_t)__builtin_ctz(rest);        // window i: the 2 k bits from bit 2 i of hi:lo, counted from the top
      uint64_t key = ((hi << s2) | ((lo >> 1) >> (63 - s2))) >> down;
      if (kCanon) {
        const uint64_t rc = ((rlo >> s2) | ((rhi << 1) << (63 - s2))) & kmask;
        key = rc < key ? rc : key;
      }
      if (run_cnt && key == run_key) ++run_cnt;
      else {
        if (run_cnt) emit(run_key, run_cnt);
        run_key = key;
        run_cnt = 1;
      }
    }
    if (merge) {
      // lanes whose sixteen windows are one k-mer, the same as the lane's before them, leave their adds to the first of the run
      const bool full = run_cnt == 16;
      const uint64_t prev_key = __shfl_up((unsigned long long)run_key, 1, 64);
      const int prev_full = __shfl_up((int)full, 1, 64);
      const bool follows = full && lane > 0 && prev_full && prev_key == run_key;
      const uint64_t fm = __builtin_amdgcn_ballot_w64(follows);
      if (follows) run_cnt = 0;
      else if (full && lane < 63) run_cnt += 16u * (uint32_t)__builtin_ctzll(~(fm >> (lane + 1)));
    }
    if (run_cnt) emit(run_key, run_cnt);
  }
  n_windows = wave_sum(n_windows);
  n_skipped = wave_sum(n_skipped);
  n_short = wave_sum(n_short);
  n_ones = wave_sum(n_ones);
  if (lane == 0) {
    if (n_windows) atomicAdd(&stats[kStWindows], (unsigned long long)n_windows);
    if (n_skipped) atomicAdd(&stats[kStSkipped], (unsigned long long)n_skipped);
    if (n_short) atomicAdd(&stats[kStShort], (unsigned long long)n_short);
    if (n_ones) atomicAdd(&stats[kStOnes], (unsigned long long)n_ones);
  }
}

// H2: distinct, unique, max_count and the sum of the counts; stats[kStOnes], the counter of the key that has no slot, is included
__global__ __launch_bounds__(256) void kc_finish(const KcSlot* table, uint64_t slots, unsigned long long* stats) {
  uint64_t distinct = 0, unique = 0, mx = 0, sum = 0;
  for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * 256) {
    const KcSlot v = load_slot(table, s);
    if (v.key == kEmpty) continue;
    ++distinct;
    unique += v.count == 1;
    mx = v.count > mx ? v.count : mx;
    sum += v.count;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const uint64_t ones = stats[kStOnes];                            // (written by H1, before this launch)
    if (ones) {
      ++distinct;
      unique += ones == 1;
      mx = ones > mx ? ones : mx;
      sum += ones;
    }
  }
  distinct = wave_sum(distinct);
  unique = wave_sum(unique);
  sum = wave_sum(sum);
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0 && sum) {
    atomicAdd(&stats[kStDistinct], (unsigned long long)distinct);
    if (unique) atomicAdd(&stats[kStUnique], (unsigned long long)unique);
    atomicAdd(&stats[kStSum], (unsigned long long)sum);
    atomicMax(&stats[kStMax], (unsigned long long)mx);
  }
}

__global__ __launch_bounds__(256) void kc_zero(unsigned long long* words, uint64_t n) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) words[i] = 0;
}

// H3: hist[min(count, bins - 1)] += 1 per key.  A block sees fewer than 2^32 slots: 32-bit counters in LDS.
__global__ __launch_bounds__(256) void kc_hist(const KcSlot* table, uint64_t slots, unsigned long long* hist, uint64_t bins) {
  __shared__ uint32_t cnt[kKcHistLds];
  const uint32_t in_lds = (uint32_t)(bins < kKcHistLds ? bins : kKcHistLds);
  for (uint32_t b = threadIdx.x; b < in_lds; b += 256) cnt[b] = 0;
  __syncthreads();
  for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * 256) {
    const KcSlot v = load_slot(table, s);
    if (v.key == kEmpty) continue;
    const uint64_t b = v.count < bins - 1 ? v.count : bins - 1;
    if (b < in_lds) atomicAdd(&cnt[(uint32_t)b], 1u);
    else atomicAdd(&hist[b], 1ull);
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < in_lds; b += 256)
    if (cnt[b]) atomicAdd(&hist[b], (unsigned long long)cnt[b]);
}

// H4: the slots with lo <= count (<= hi unless hi = 0).  kWrite = false: *cursor += their number; true: they go to out[0 .. cap)
// in any order, a wave taking its places with one atomic.
template <bool kWrite>
__global__ __launch_bounds__(256) void kc_select(const KcSlot* table, uint64_t slots, uint64_t lo, uint64_t hi, scfq_kmer_count* out, uint64_t cap,
                                                unsigned long long* cursor) {
  const uint32_t lane = threadIdx.x & 63u;
  uint64_t mine = 0;
  for (uint64_t s0 = (uint64_t)blockIdx.x * 256; s0 < slots; s0 += (uint64_t)gridDim.x * 256) {      // (wave-uniform)
    const uint64_t s = s0 + threadIdx.x;
    KcSlot v{kEmpty, 0};
    if (s < slots) v = load_slot(table, s);
    const bool q = v.key != kEmpty && v.count >= lo && (hi == 0 || v.count <= hi);
    if (!kWrite) { mine += q; continue; }
    const uint64_t m = __builtin_amdgcn_ballot_w64(q);
    if (!m) continue;
    unsigned long long at = 0;
    if (lane == (uint32_t)__builtin_ctzll(m)) at = atomicAdd(cursor, (unsigned long long)__builtin_popcountll(m));
    at = __shfl((unsigned long long)at, __builtin_ctzll(m), 64) + (uint64_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
    if (q && at < cap) out[at] = scfq_kmer_count{v.key, v.count};
  }
  if (!kWrite) {
    mine = wave_sum(mine);
    if (lane == 0 && mine) atomicAdd(cursor, (unsigned long long)mine);
  }
}

// H5: counts[i] of keys[i] (already canonical); at most max_probe slots per key
__global__ __launch_bounds__(256) void kc_query(const KcSlot* table, uint64_t slot_mask, uint32_t max_probe, const uint64_t* keys, uint64_t n,
                                               uint64_t* counts) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t key = keys[i];
  uint64_t slot = mix64(key) & slot_mask, found = 0;
  for (uint32_t p = 0; p < max_probe; ++p) {
    const KcSlot v = load_slot(table, slot);
    if (v.key == key) { found = v.count; break; }
    if (v.key == kEmpty) break;
    slot = (slot + 1) & slot_mask;
  }
  counts[i] = found;
}

unsigned grid_for(uint64_t items) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((items + 255) / 256, 2048)); }

// off: the line index; the caller's (lines and has_cr with it), or nullptr: it is built here, into line_off
struct Input { const uint8_t* d = nullptr; uint64_t n = 0, lines = 0; bool has_cr = true; const uint64_t* off = nullptr; DevBuf line_off; };

int full_error(uint64_t slots, const char* why) {
  std::snprintf(g_cerr, sizeof g_cerr, "a table of %llu slots %s", (unsigned long long)slots, why);
  return SCFQ_EFULL;
}

// in[0 .. n_in): the resident inputs.  *out (if asked for) receives the table.
int kcount_device(Input* in, int n_in, const scfq_kcount_opts& o, scfq_kcount** out, scfq_kcount_summary* sum, hipStream_t stream) {
  for (double& m : g_stage_ms) m = 0;
  scfq_kcount_summary s;
  std::memset(&s, 0, sizeof s);
  s.struct_size = sizeof s;
  s.abi_version = SCFQ_ABI_VERSION;
  s.k = o.k;
  s.flags = o.flags;
  int rc = SCFQ_OK;
  {
    const auto t_a = std::chrono::steady_clock::now();
    for (int i = 0; i < n_in; ++i) {
      if (!in[i].off) {
        if ((rc = scfq_scratch::build_line_index(in[i].d, in[i].n, stream, g_cerr, in[i].line_off, &in[i].lines, &in[i].has_cr))) return rc;
        in[i].off = in[i].line_off.as<uint64_t>();
      }
      const uint64_t reads = (in[i].lines + 3) / 4;
      if (reads >= (1ull << 31)) { std::snprintf(g_cerr, sizeof g_cerr, "more than 2^31 records in one input"); return SCFQ_EARG; }
      s.reads += reads;
      s.lines += in[i].lines;
      s.input_bytes += in[i].n;
    }
    g_stage_ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_a).count();
  }
  static const bool timing = scfq_scratch::env_switch("SCFQ_KCOUNT_TIMING");
  static const bool merge = [] { const char* e = std::getenv("SCFQ_KCOUNT_MERGE"); return !e || std::atoi(e) != 0; }();
  static const uint32_t env_start = env_u32("SCFQ_KCOUNT_START_BITS"), env_probe = env_u32("SCFQ_KCOUNT_MAX_PROBE");
  const bool fixed = o.table_bits != 0;
  uint32_t bits = fixed ? o.table_bits : auto_bits(s.input_bytes, env_start);
  const bool canonical = (o.flags & SCFQ_KCOUNT_CANONICAL) != 0;

  DevBuf stats;              // kStWords words, then the `failed` word
  if ((rc = stats.alloc((kStWords + 1) * 8, stream, g_cerr))) return rc;
  unsigned long long* d_stats = stats.as<unsigned long long>();
  uint32_t* d_failed = reinterpret_cast<uint32_t*>(d_stats + kStWords);
  scfq_scratch::StageClock clk(stream, timing);
  struct Table {             // the table of the pass; the handle takes it over at the end
    void* p = nullptr;
    ~Table() { if (p) (void)hipFree(p); }
  } table;
  uint64_t h[kStWords + 1];
  for (;;) {
    const uint64_t slots = 1ull << bits;
    if (hipMalloc(&table.p, slots * sizeof(KcSlot) + (out ? kScratchBytes + 16 : 0)) != hipSuccess) {      // (+ the readers' scratch and cursor)
      (void)hipGetLastError();
      table.p = nullptr;
      return full_error(slots, "does not fit into the device memory");
    }
    ++s.passes;
    s.slots = slots;
    const uint32_t max_probe = probe_bound(slots, fixed, env_probe);
    SCFQ_SCRATCH_CHK(g_cerr, hipMemsetAsync(stats.p, 0, (kStWords + 1) * 8, stream));
    hipLaunchKernelGGL(kc_clear, dim3(grid_for(slots)), dim3(256), 0, stream, static_cast<KcSlot*>(table.p), slots);
    SCFQ_SCRATCH_CHK(g_cerr, hipGetLastError());
    clk.mark(0);
    for (int i = 0; i < n_in; ++i) {
      if (!in[i].lines) continue;
      const uint32_t shift = (uint32_t)((uintptr_t)in[i].d & 15u);
      const uint64_t chunks = (shift + in[i].n) / 16 + 1;      // the last one holds the position behind the input
      const uint64_t steps = (chunks + kKcThreads - 1) / kKcThreads;
      const uint64_t spb = (steps + kKcMaxBlocks - 1) / kKcMaxBlocks;
      const unsigned blocks = (unsigned)((steps + spb - 1) / spb);
      if (canonical)
        hipLaunchKernelGGL(kc_count<true>, dim3(blocks), dim3(kKcThreads), 0, stream, in[i].d, in[i].n, in[i].off, in[i].lines,
                           shift, in[i].has_cr, o.k, merge, chunks, spb, static_cast<KcSlot*>(table.p), slots - 1, max_probe, d_failed, d_stats);
      else
        hipLaunchKernelGGL(kc_count<false>, dim3(blocks), dim3(kKcThreads), 0, stream, in[i].d, in[i].n, in[i].off, in[i].lines,
                           shift, in[i].has_cr, o.k, merge, chunks, spb, static_cast<KcSlot*>(table.p), slots - 1, max_probe, d_failed, d_stats);
      SCFQ_SCRATCH_CHK(g_cerr, hipGetLastError());
    }
    clk.mark(1);
    hipLaunchKernelGGL(kc_finish, dim3(grid_for(slots)), dim3(256), 0, stream, static_cast<const KcSlot*>(table.p), slots, d_stats);
    SCFQ_SCRATCH_CHK(g_cerr, hipGetLastError());
    clk.mark(2);
    SCFQ_SCRATCH_CHK(g_cerr, hipMemcpyAsync(h, stats.p, sizeof h, hipMemcpyDeviceToHost, stream));
    SCFQ_SCRATCH_CHK(g_cerr, hipStreamSynchronize(stream));
    if (!(uint32_t)h[kStWords]) {
      if (out) {
        scfq_kcount* t = new (std::nothrow) scfq_kcount;
        if (!t) return SCFQ_ENOMEM;
        t->slots_dev = table.p;
        t->scratch_dev = static_cast<char*>(table.p) + slots * sizeof(KcSlot);
        t->cursor_dev = static_cast<char*>(t->scratch_dev) + kScratchBytes;
        table.p = nullptr;
        t->slots = slots;
        t->ones = h[kStOnes];
        t->distinct = h[kStDistinct];
        t->passes = s.passes;
        t->k = o.k;
        t->flags = o.flags;
        t->max_probe = max_probe;
        *out = t;
      }
      break;
    }
    // the pass failed: it is thrown away whole
    SCFQ_SCRATCH_CHK(g_cerr, hipFree(table.p));
    table.p = nullptr;
    if (fixed) return full_error(slots, "(table_bits) cannot hold the keys of this input");
    if (bits + 2 > kMaxBits) return full_error(slots, "cannot hold the keys, and four times as many are more than 2^32");
    size_t free_b = 0, total_b = 0;
    SCFQ_SCRATCH_CHK(g_cerr, hipMemGetInfo(&free_b, &total_b));
    if ((4 * slots) * sizeof(KcSlot) > free_b / 2) return full_error(slots, "cannot hold the keys, and four times as many do not fit into half of the free device memory");
    bits += 2;
  }
  s.windows = h[kStWindows];
  s.kmers = h[kStSum];
  s.skipped = h[kStSkipped];
  s.short_lines = h[kStShort];
  s.distinct = h[kStDistinct];
  s.unique = h[kStUnique];
  s.max_count = h[kStMax];
  g_stage_ms[1] = clk.between(0, 1);
  g_stage_ms[2] = clk.between(1, 2);
  if (sum) *sum = s;
  return SCFQ_OK;
}

// the call on one or two resident inputs, all kernels on the first one's stream; after a failure kernels that read the second
// input may still be queued there: they are waited for before the second input's memory goes back
int run(scfq_scratch::ResidentInput& in1, scfq_scratch::ResidentInput* in2, const scfq_kcount_opts& o, scfq_kcount** out, scfq_kcount_summary* sum) {
  Input in[2];
  in[0].d = in1.d_in; in[0].n = in1.n;
  if (in2) { in[1].d = in2->d_in; in[1].n = in2->n; }
  const int rc = kcount_device(in, in2 ? 2 : 1, o, out, sum, in1.stream);
  if (rc == SCFQ_OK) in1.mark_clean();      // (its last act was to wait for the stream)
  else (void)hipStreamSynchronize(in1.stream);
  return rc;
}

// a reader's result to the caller's (pageable) memory: the stream is waited for, then the copy is a synchronous one
int copy_down(void* dst_host, const void* src_dev, size_t bytes, hipStream_t stream) {
  SCFQ_SCRATCH_CHK(g_cerr, hipStreamSynchronize(stream));
  SCFQ_SCRATCH_CHK(g_cerr, hipMemcpy(dst_host, src_dev, bytes, hipMemcpyDeviceToHost));
  return SCFQ_OK;
}

// a private stream for a call on a handle
struct HandleCall {
  scfq_scratch::StreamLease lease;
  int begin() { return lease.acquire(g_cerr); }
  hipStream_t s() const { return lease.s; }
};

}  // namespace

namespace scfq_kcount_internal {

bool view(const scfq_kcount* t, View* out) {
  if (!t || !out) return false;
  out->slots = t->slots_dev;
  out->n_slots = t->slots;
  out->ones = t->ones;
  out->distinct = t->distinct;
  out->passes = t->passes;
  out->k = t->k;
  out->flags = t->flags;
  out->max_probe = t->max_probe;
  return true;
}

int count_resident(const Resident* r, int n_in, const scfq_kcount_opts& o, scfq_kcount** out, scfq_kcount_summary* sum, hipStream_t stream) {
  g_cerr[0] = '\0';
  if (out) *out = nullptr;
  Input in[2];
  for (int i = 0; i < n_in && i < 2; ++i) {
    in[i].d = r[i].d; in[i].n = r[i].n; in[i].off = r[i].line_off; in[i].lines = r[i].lines; in[i].has_cr = r[i].has_cr;
  }
  return kcount_device(in, n_in < 2 ? n_in : 2, o, out, sum, stream);
}

}  // namespace scfq_kcount_internal

extern "C" {

const char* scfq_kcount_error_detail(void) { return g_cerr; }

int scfq_debug_kcount_stages(double* ms, uint32_t cap) { return scfq_scratch::copy_stage_ms(g_stage_ms, ms, cap); }

int scfq_format_kcount_tsv(uint32_t k, uint64_t key, uint64_t count, char* buf, uint64_t cap) { return format_tsv(k, key, count, buf, cap); }

int scfq_kcount_buffers(const void* r1, uint64_t n1, const void* r2, uint64_t n2, int is_device, const scfq_kcount_opts* opts, scfq_kcount** out,
                        scfq_kcount_summary* sum) {
  g_cerr[0] = '\0';
  if (out) *out = nullptr;
  int rc = check_opts(opts, sum, out != nullptr, g_cerr, sizeof g_cerr);
  if (rc) return rc;
  if ((!r1 && n1) || (!r2 && n2)) { std::snprintf(g_cerr, sizeof g_cerr, "a NULL input with n > 0"); return SCFQ_EARG; }
  if (sum) scfq_scratch::clear_keep_size(sum);
  const bool two = r2 != nullptr;
  scfq_scratch::ResidentInput in1, in2;
  if ((rc = in1.from_buffer(r1, n1, is_device != 0, is_device != 0, g_cerr))) return rc;
  // (a host buffer's copy is waited for inside; device memory of the caller is ordered before in1's stream above)
  if (two && (rc = in2.from_buffer(r2, n2, is_device != 0, false, g_cerr))) return rc;
  return run(in1, two ? &in2 : nullptr, *opts, out, sum);
}

int scfq_kcount_files(const char* path1, const char* path2, const scfq_opts* opts, const scfq_kcount_opts* kopts, scfq_kcount** out,
                      scfq_kcount_summary* sum) {
  g_cerr[0] = '\0';
  if (out) *out = nullptr;
  int rc = check_opts(kopts, sum, out != nullptr, g_cerr, sizeof g_cerr);
  if (rc) return rc;
  if (!path1) { std::snprintf(g_cerr, sizeof g_cerr, "path1 is NULL"); return SCFQ_EARG; }
  if (sum) scfq_scratch::clear_keep_size(sum);
  scfq_scratch::ResidentInput in1, in2;
  if ((rc = in1.from_file(path1, opts, g_cerr))) return rc;
  if (path2 && (rc = in2.from_file(path2, opts, g_cerr))) return rc;      // (staged when this returns)
  return run(in1, path2 ? &in2 : nullptr, *kopts, out, sum);
}

int scfq_kcount_hist(const scfq_kcount* t, uint64_t* hist_host, uint64_t bins) {
  g_cerr[0] = '\0';
  if (!t || !hist_host) { std::snprintf(g_cerr, sizeof g_cerr, "a NULL argument"); return SCFQ_EARG; }
  if (bins < 2 || bins > kMaxBins) {
    std::snprintf(g_cerr, sizeof g_cerr, "bins = %llu is outside 2 .. %llu", (unsigned long long)bins, (unsigned long long)kMaxBins);
    return SCFQ_EARG;
  }
  g_stage_ms[3] = 0;
  std::lock_guard<std::mutex> lk(t->mu);
  HandleCall call;
  int rc = call.begin();
  if (rc) return rc;
  // the bins live in the table's scratch, as every reader's memory does (fq-kcount, open point)
  unsigned long long* hist = static_cast<unsigned long long*>(t->scratch_dev);
  static const bool timing = scfq_scratch::env_switch("SCFQ_KCOUNT_TIMING");
  scfq_scratch::StageClock clk(call.s(), timing);
  hipLaunchKernelGGL(kc_zero, dim3(grid_for(bins)), dim3(256), 0, call.s(), hist, bins);
  SCFQ_SCRATCH_CHK(g_cerr, hipGetLastError());
  clk.mark(0);
  hipLaunchKernelGGL(kc_hist, dim3(grid_for(t->slots)), dim3(256), 0, call.s(), static_cast<const KcSlot*>(t->slots_dev), t->slots, hist, bins);
  SCFQ_SCRATCH_CHK(g_cerr, hipGetLastError());
  clk.mark(1);
  if ((rc = copy_down(hist_host, hist, bins * 8, call.s()))) return rc;
  if (t->ones) ++hist_host[std::min<uint64_t>(t->ones, bins - 1)];
  g_stage_ms[3] = clk.between(0, 1);
  call.lease.clean = true;
  return SCFQ_OK;
}

int scfq_kcount_dump(const scfq_kcount* t, uint64_t min_count, uint64_t max_count, scfq_kmer_count* out_host, uint64_t cap, uint64_t* total) {
  g_cerr[0] = '\0';
  if (!t || !total || (!out_host && cap)) { std::snprintf(g_cerr, sizeof g_cerr, "a NULL argument"); return SCFQ_EARG; }
  std::lock_guard<std::mutex> lk(t->mu);
  HandleCall call;
  int rc = call.begin();
  if (rc) return rc;
  const KcSlot* table = static_cast<const KcSlot*>(t->slots_dev);
  unsigned long long* cursor = static_cast<unsigned long long*>(t->cursor_dev);
  scfq_kmer_count* rows = static_cast<scfq_kmer_count*>(t->scratch_dev);
  unsigned long long in_table = 0;
  SCFQ_SCRATCH_CHK(g_cerr, hipMemsetAsync(cursor, 0, 8, call.s()));
  hipLaunchKernelGGL(kc_select<false>, dim3(grid_for(t->slots)), dim3(256), 0, call.s(), table, t->slots, min_count, max_count,
                     (scfq_kmer_count*)nullptr, (uint64_t)0, cursor);
  SCFQ_SCRATCH_CHK(g_cerr, hipGetLastError());
  if ((rc = copy_down(&in_table, cursor, 8, call.s()))) return rc;
  const bool ones = t->ones && t->ones >= min_count && (max_count == 0 || t->ones <= max_count);
  *total = in_table + (ones ? 1 : 0);
  if (*total && cap >= *total) {
    // the table in pieces of kDumpPiece slots, whose rows fit the scratch whatever qualifies; the host gathers them behind each other
    uint64_t done = 0;
    for (uint64_t s0 = 0; s0 < t->slots && done < in_table; s0 += kDumpPiece) {
      const uint64_t n = std::min<uint64_t>(kDumpPiece, t->slots - s0);
      unsigned long long got = 0;
      SCFQ_SCRATCH_CHK(g_cerr, hipMemsetAsync(cursor, 0, 8, call.s()));
      hipLaunchKernelGGL(kc_select<true>, dim3(grid_for(n)), dim3(256), 0, call.s(), table + s0, n, min_count, max_count, rows, kDumpPiece, cursor);
      SCFQ_SCRATCH_CHK(g_cerr, hipGetLastError());
      if ((rc = copy_down(&got, cursor, 8, call.s()))) return rc;
      if (got > n || done + got > in_table) {      // (the table does not change between the two passes)
        std::snprintf(g_cerr, sizeof g_cerr, "dump: %llu rows counted, more written", in_table);
        return SCFQ_EHIP;
      }
      if (got && (rc = copy_down(out_host + done, rows, got * sizeof(scfq_kmer_count), call.s()))) return rc;
      done += got;
    }
    if (done != in_table) {
      std::snprintf(g_cerr, sizeof g_cerr, "dump: %llu rows counted, %llu written", in_table, (unsigned long long)done);
      return SCFQ_EHIP;
    }
    std::sort(out_host, out_host + in_table, [](const scfq_kmer_count& a, const scfq_kmer_count& b) { return a.key < b.key; });
    if (ones) out_host[in_table] = scfq_kmer_count{kEmpty, t->ones};      // (the largest key there is)
  }
  call.lease.clean = true;      // (every piece ended with a wait for the stream)
  return SCFQ_OK;
}

int scfq_kcount_query(const scfq_kcount* t, const uint64_t* keys_host, uint64_t n, uint64_t* counts_host) {
  g_cerr[0] = '\0';
  if (!t || ((!keys_host || !counts_host) && n)) { std::snprintf(g_cerr, sizeof g_cerr, "a NULL argument"); return SCFQ_EARG; }
  if (!n) return SCFQ_OK;
  const uint64_t kmask = key_mask(t->k);
  const bool canonical = (t->flags & SCFQ_KCOUNT_CANONICAL) != 0;
  std::vector<uint64_t> keys;
  try { keys.resize(n); } catch (const std::bad_alloc&) { return SCFQ_ENOMEM; }
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t key = keys_host[i];
    if (key & ~kmask) {
      std::snprintf(g_cerr, sizeof g_cerr, "keys[%llu] = %llu is not below 4^%u", (unsigned long long)i, (unsigned long long)key, t->k);
      return SCFQ_EARG;
    }
    keys[i] = canonical ? std::min(key, revcomp(key, t->k)) : key;
  }
  std::lock_guard<std::mutex> lk(t->mu);
  HandleCall call;
  int rc = call.begin();
  if (rc) return rc;
  // kQueryPiece keys at a time: the keys in the first half of the table's scratch, their counts in the second
  uint64_t* d_keys = static_cast<uint64_t*>(t->scratch_dev);
  uint64_t* d_counts = d_keys + kQueryPiece;
  for (uint64_t i0 = 0; i0 < n; i0 += kQueryPiece) {
    const uint64_t m = std::min<uint64_t>(kQueryPiece, n - i0);
    SCFQ_SCRATCH_CHK(g_cerr, hipMemcpyAsync(d_keys, keys.data() + i0, m * 8, hipMemcpyHostToDevice, call.s()));
    hipLaunchKernelGGL(kc_query, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, call.s(), static_cast<const KcSlot*>(t->slots_dev), t->slots - 1,
                       t->max_probe, d_keys, m, d_counts);
    SCFQ_SCRATCH_CHK(g_cerr, hipGetLastError());
    if ((rc = copy_down(counts_host + i0, d_counts, m * 8, call.s()))) return rc;
  }
  for (uint64_t i = 0; i < n; ++i)
    if (keys[i] == kEmpty) counts_host[i] = t->ones;                 // (the key without a slot)
  call.lease.clean = true;      // (every piece ended with a wait for the stream)
  return SCFQ_OK;
}

void scfq_kcount_free(scfq_kcount* t) {
  if (!t) return;
  if (t->slots_dev) (void)hipFree(t->slots_dev);
  delete t;
}

}  // extern "C"

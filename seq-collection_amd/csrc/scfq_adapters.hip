// scfq_adapters.hip — `sc fq-adapters` on the MI355X (gfx950): where in the reads known adapters (or poly-A / poly-G tails) first occur.
// Not in the reference; definitions in include/sc_fqcount.h.
//
// The whole (inflated) input sits in HBM, as for fq-kmers:
//   K5  line index            (scfq_scratch::build_line_index: line_off[0 .. lines], and whether the input holds "\r\n" at all)
//   A0  ad_lens               a pass over line_off: the longest sequence line (the rows of the table, and the 32-bit position check)
//   A1  ad_match              the hot path, partitioned by BYTES exactly as km_count (scfq_kmers.hip): 16-byte chunks on the address grid, a
//                             chunk per lane, a block owns a run of consecutive 8 KiB steps, one binary search in line_off per block, the
//                             line of every byte from the '\n' the block sees.  (The chunk load, the newline prefix and the line phase
//                             repeat km_count's; see DESIGN.md §fq-adapters for why they are not shared yet.)  A lane owns the windows that
//                             START in its chunk.  It makes of its bytes a 2-bit word (first byte on top) and a "not A C G T" mask and tests
//                             its sixteen starts against each probe's word under the probe's length mask; '\n', '\r' and what lies outside
//                             the input are "not A C G T", so no window crosses a line end.  Whether a start lies in a sequence line (4i+1)
//                             comes from the line number.
//                               every probe <= 16 letters:  bytes [o, o + 31), 32-bit compares (the loads are km_count's two chunks)
//                               a probe of 17 .. 32:        bytes [o, o + 47), 64-bit compares
//                             The probes (words, masks, lengths) are a kernel argument: scalar registers for the whole kernel.
//                             first[read][probe] (32-bit, all-ones = none, pool memory) takes an atomicMin per (line, probe) a lane sees in
//                             its chunk; lanes of a wave that continue a line on which a lower lane has an occurrence already leave it to
//                             that lane, and a plain load in front of the atomic skips what cannot lower the word (values only fall: a
//                             stale load is never too small).  hits[j] are per-lane registers, one atomic per wave at the block's end.
//   A2  ad_rows               a thread per read: its words, `any` = their minimum, +1 on rows[min(first, positions)][j]; equal (row, column)
//                             pairs of a wave are added as one (all reads may hold the probe at position 0)
//   A3  ad_finish             the sum of the rows (total); rows, tail and total go to the host
// Everything is integer / byte work; there is no CPU fallback.
#include "../../include/sc_fqcount.h"
#include "../../include/sc_fqcount_debug.h"

#include <hip/hip_runtime.h>

#include "scfq_record_device.hpp"
#include "scfq_scratch.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>

namespace {

thread_local char g_aerr[scfq_scratch::kErrBytes] = "";
thread_local double g_stage_ms[4] = {0, 0, 0, 0};

using scfq_scratch::DevBuf;

constexpr uint32_t kAdThreads = 512;                 // a chunk per lane and step
constexpr uint32_t kAdWaves = kAdThreads / 64;
constexpr uint32_t kAdMaxBlocks = 1024;
constexpr uint32_t kAdNone = 0xffffffffu;            // first[read][probe]: no occurrence
constexpr uint32_t kAdCols = SCFQ_ADAPTERS_MAX_PROBES + 1;      // a row: first[8], any
static_assert(SCFQ_ADAPTERS_MAX_PROBES == 8 && SCFQ_ADAPTERS_MAX_LEN == 32 && sizeof(scfq_adapter_row) == 8 * kAdCols, "a row is nine words");
static_assert(SCFQ_ADAPTERS_MAX_CAP < kAdNone, "a row number fits the 32-bit key of ad_rows");

enum : uint32_t { kStHits = 0, kStMaxLen = 8, kStTotal = 9, kStWords = 18 };      // hits[8], max_seq_len, total[9]

struct AdProbes {
  uint64_t word[SCFQ_ADAPTERS_MAX_PROBES];           // 2-bit codes (A C G T -> 0 1 2 3), the first letter in the top two bits
  uint64_t mask[SCFQ_ADAPTERS_MAX_PROBES];           // the top 2 * len bits
  uint32_t len[SCFQ_ADAPTERS_MAX_PROBES];
  uint32_t n;
};

// OR of x >> 0 .. x >> (k - 1): bit i says whether any of bits i .. i + k - 1 is set
template <typename T> __device__ __forceinline__ T smear_down(T x, uint32_t k) {
  uint32_t done = 1;
  while (done < k) {
    const uint32_t sh = done < k - done ? done : k - done;
    x |= x >> sh;
    done += sh;
  }
  return x;
}

// A0: the longest text of a sequence line
__global__ __launch_bounds__(256) void ad_lens(const uint8_t* base, uint64_t n, const uint64_t* line_off, uint64_t lines, bool has_cr,
                                               unsigned long long* stats) {
  const uint64_t j = 4 * ((uint64_t)blockIdx.x * 256 + threadIdx.x) + 1;
  uint64_t len = 0;
  if (j < lines) {
    uint64_t s, e;
    line_span(base, n, line_off, j, s, e, has_cr);
    len = e - s;
  }
  len = wave_max(len);
  if ((threadIdx.x & 63) == 0 && len) atomicMax(&stats[kStMaxLen], (unsigned long long)len);
}

// A1.  kWide: a probe has more than 16 letters.  chunks: 16-byte chunks of the address grid that hold a byte of the input;
// steps_per_block * kAdThreads of them per block.  shift: address of the input mod 16.
template <bool kWide>
__global__ __launch_bounds__(kAdThreads) void ad_match(const uint8_t* base, uint64_t n, const uint64_t* line_off, uint64_t lines, uint32_t shift,
                                                      AdProbes pr, uint64_t chunks, uint64_t steps_per_block, uint32_t* first,
                                                      unsigned long long* stats) {
  constexpr int kBytes = kWide ? 47 : 31;            // a start in the chunk and the longest probe behind it
  constexpr int kWords = kWide ? 12 : 8;
  __shared__ uint32_t wave_nl[2][kAdWaves];
  __shared__ uint64_t first_line;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;

  const uint64_t step0 = (uint64_t)blockIdx.x * steps_per_block;
  const uint64_t c_first = step0 * kAdThreads;                       // (c_first < chunks: the grid is sized so)
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
  uint32_t n_hits[SCFQ_ADAPTERS_MAX_PROBES] = {0, 0, 0, 0, 0, 0, 0, 0};      // (at most 16 per step: a block's steps fit 32 bits)

  for (uint64_t st = 0; st < steps_per_block; ++st) {
    const uint64_t c0 = c_first + st * kAdThreads;
    if (c0 >= chunks) break;                                         // (block-uniform)
    const uint64_t c = c0 + threadIdx.x;
    const int64_t o = 16 * (int64_t)c - (int64_t)shift;              // offset of this lane's byte 0; bytes [o, o + kBytes) are looked at
    uint32_t w[kWords];
#pragma unroll
    for (int i = 0; i < kWords; ++i) w[i] = 0;                       // (a byte outside the input stays 0: not A C G T, not '\n')
    if (c < chunks) {
      if (o >= 0 && o + 4 * kWords <= (int64_t)n) {
#pragma unroll
        for (int q = 0; q < kWords / 4; ++q) {
          const uint4 v = *reinterpret_cast<const uint4*>(base + o + 16 * q);      // (aligned: shift + o = 0 mod 16)
          w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
        }
      } else {
        // the input's first chunk and its last ones: only its own bytes are read
        for (int i = 0; i < 4 * kWords; ++i) {
          const int64_t p = o + i;
          if (p >= 0 && p < (int64_t)n) w[i >> 2] |= (uint32_t)base[p] << (8 * (i & 3));
        }
      }
    }
    // bytes 0 .. kBytes - 1: the 2-bit words with byte 0 (byte 32) on top, the "not A C G T" mask; the '\n' of the chunk
    uint64_t hi = 0, lo = 0, bad = 0;
    uint32_t nl16 = 0;
#pragma unroll
    for (int i = 0; i < kBytes; ++i) {
      const uint32_t b = (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
      const uint32_t code = ((b >> 1) & 3u) ^ ((b >> 2) & 1u);                       // A C G T -> 0 1 2 3
      const bool ok = ((0x54474341u >> (8 * code)) & 0xffu) == b;
      if (i < 32) hi |= (uint64_t)code << (62 - 2 * i);
      else lo |= (uint64_t)code << (62 - 2 * (i - 32));
      bad |= (uint64_t)(ok ? 0u : 1u) << i;
      if (i < 16) nl16 |= (b == '\n' ? 1u : 0u) << i;
    }

    // the line of this lane's byte 0
    uint32_t incl = (uint32_t)__builtin_popcount(nl16);
    const uint32_t own = incl;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d, 64);
      if (lane >= (uint32_t)d) incl += up;
    }
    if (lane == 63) wave_nl[st & 1][wave] = incl;
    __syncthreads();
    uint32_t before = incl - own, step_nl = 0;
#pragma unroll
    for (uint32_t v = 0; v < kAdWaves; ++v) {
      const uint32_t t = wave_nl[st & 1][v];
      if (v < wave) before += t;
      step_nl += t;
    }
    const uint64_t line0 = line_run + before;
    line_run += step_nl;

    // the bytes of this chunk that lie in a sequence line (4i + 1)
    uint32_t in_seq = 0;
    {
      uint32_t rest = 0xffffu, ph = (uint32_t)line0 & 3u, m = nl16;
      while (m) {
        const uint32_t bit = (uint32_t)__builtin_ctz(m);
        m &= m - 1;
        const uint32_t seg = rest & ((2u << bit) - 1u);
        if (ph == 1) in_seq |= seg;
        rest &= ~seg;
        ph = (ph + 1) & 3u;
      }
      if (ph == 1) in_seq |= rest;
    }
    const uint32_t cand = in_seq & ~(uint32_t)bad & 0xffffu;        // starts: a letter of a sequence line

    // the first occurrence per (line, probe) of this chunk goes to first[][]; called by the whole wave
    auto emit = [&](uint32_t j, uint32_t h) {
      // the leading segment continues the line of the chunk before: when a lower lane of the wave has an occurrence on that line
      // (behind its last '\n', and no '\n' in the lanes between), that one is the smaller position
      const uint32_t lead = nl16 ? (1u << __builtin_ctz(nl16)) - 1u : 0xffffu;
      const uint32_t trail = nl16 ? ~((2u << (31 - __builtin_clz(nl16))) - 1u) & 0xffffu : 0xffffu;
      const uint64_t b_nl = __builtin_amdgcn_ballot_w64(nl16 != 0);
      const uint64_t b_trail = __builtin_amdgcn_ballot_w64((h & trail) != 0);
      const uint64_t lower = (1ull << lane) - 1ull;
      const uint64_t nl_lower = b_nl & lower;
      const uint64_t from = nl_lower ? ~((1ull << (63 - __builtin_clzll(nl_lower))) - 1ull) : ~0ull;
      if (b_trail & lower & from) h &= ~lead;
      while (h) {
        const uint32_t bit = (uint32_t)__builtin_ctz(h);
        const uint64_t ln = line0 + (uint32_t)__builtin_popcount(nl16 & ((1u << bit) - 1u));      // (a sequence line: ln = 4i + 1)
        const uint64_t pos = ln < lines ? (uint64_t)(o + (int64_t)bit) - line_off[ln] : ~0ull;
        if (pos < kAdNone) {                                         // (longer lines are refused by the host: nothing wraps)
          uint32_t* wd = &first[(ln >> 2) * pr.n + j];
          if (*wd > (uint32_t)pos) atomicMin(wd, (uint32_t)pos);
        }
        const uint32_t next_nl = nl16 & ~((2u << bit) - 1u);         // later occurrences on this line are not the first
        h = next_nl ? h & ~((1u << __builtin_ctz(next_nl)) - 1u) : 0u;
      }
    };

#pragma unroll
    for (uint32_t j = 0; j < SCFQ_ADAPTERS_MAX_PROBES; ++j) {
      if (j < pr.n) {                                                // (kernel-uniform)
        uint32_t h = 0;
        if (cand) {
          const uint32_t ok = cand & ~(kWide ? (uint32_t)smear_down<uint64_t>(bad, pr.len[j]) : smear_down<uint32_t>((uint32_t)bad, pr.len[j]));
          if (ok) {
            if (kWide) {
              const uint64_t pw = pr.word[j], pm = pr.mask[j];
#pragma unroll
              for (int i = 0; i < 16; ++i) {
                const uint64_t win = i ? (hi << (2 * i)) | (lo >> (64 - 2 * i)) : hi;
                h |= (((win ^ pw) & pm) == 0 ? 1u : 0u) << i;
              }
            } else {
              const uint32_t pw = (uint32_t)(pr.word[j] >> 32), pm = (uint32_t)(pr.mask[j] >> 32);
#pragma unroll
              for (int i = 0; i < 16; ++i) {
                const uint32_t win = (uint32_t)((hi << (2 * i)) >> 32);
                h |= (((win ^ pw) & pm) == 0 ? 1u : 0u) << i;
              }
            }
            h &= ok;
          }
        }
        n_hits[j] += (uint32_t)__builtin_popcount(h);
        if (__builtin_amdgcn_ballot_w64(h != 0)) emit(j, h);         // (wave-uniform; rare on real data)
      }
    }
  }
#pragma unroll
  for (uint32_t j = 0; j < SCFQ_ADAPTERS_MAX_PROBES; ++j) {
    if (j < pr.n) {
      const uint64_t s = wave_sum((uint64_t)n_hits[j]);
      if (lane == 0 && s) atomicAdd(&stats[kStHits + j], (unsigned long long)s);
    }
  }
}

// A2: a thread per read.  table: rows [0, positions] of nine words, the last one the tail.
__global__ __launch_bounds__(256) void ad_rows(const uint32_t* first, uint64_t reads, uint32_t np, uint64_t positions, unsigned long long* table) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  // +1 on table[min(f, positions)][col] for every lane with an occurrence; lanes of the wave with the same row add once
  auto add = [&](uint32_t f, uint32_t col) {
    const bool has = f != kAdNone;
    const uint32_t key = (uint64_t)f < positions ? f : (uint32_t)positions;
    uint64_t active = __builtin_amdgcn_ballot_w64(has);
    while (active) {                                                 // (wave-uniform)
      const int leader = __builtin_ctzll(active);
      const uint32_t k = (uint32_t)__shfl((int)key, leader, 64);
      const uint64_t same = __builtin_amdgcn_ballot_w64(has && key == k);
      if ((int)lane == leader) atomicAdd(&table[(uint64_t)k * kAdCols + col], (unsigned long long)__builtin_popcountll(same));
      active &= ~same;
    }
  };
  uint32_t any = kAdNone;
#pragma unroll
  for (uint32_t j = 0; j < SCFQ_ADAPTERS_MAX_PROBES; ++j) {
    if (j < np) {                                                    // (kernel-uniform)
      const uint32_t f = r < reads ? first[r * np + j] : kAdNone;
      any = f < any ? f : any;
      add(f, j);
    }
  }
  add(any, SCFQ_ADAPTERS_MAX_PROBES);
}

// A3: the sum of the rows, the tail among them
__global__ __launch_bounds__(256) void ad_finish(const unsigned long long* table, uint64_t rows, unsigned long long* stats) {
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
#pragma unroll
  for (uint32_t k = 0; k < kAdCols; ++k) {
    const uint64_t s = wave_sum(p < rows ? (uint64_t)table[p * kAdCols + k] : 0);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(&stats[kStTotal + k], (unsigned long long)s);
  }
}

// the checks of both entry points; the probes as the kernel takes them
bool args_ok(const char* const* probes, uint32_t n_probes, const scfq_adapter_row* rows_host, uint64_t cap, const scfq_adapter_summary* out,
             AdProbes* pr) {
  if (!out || out->struct_size != sizeof(scfq_adapter_summary) || (!rows_host && cap) || !probes) return false;
  if (n_probes < 1 || n_probes > SCFQ_ADAPTERS_MAX_PROBES) {
    std::snprintf(g_aerr, sizeof g_aerr, "%u probes: 1 .. %u are allowed", n_probes, (unsigned)SCFQ_ADAPTERS_MAX_PROBES);
    return false;
  }
  std::memset(pr, 0, sizeof *pr);
  pr->n = n_probes;
  for (uint32_t j = 0; j < n_probes; ++j) {
    const char* p = probes[j];
    if (!p || !*p) {
      std::snprintf(g_aerr, sizeof g_aerr, "probe %u is %s", j, p ? "empty" : "NULL");
      return false;
    }
    uint32_t len = 0;
    uint64_t word = 0;
    for (; p[len]; ++len) {
      if (len >= SCFQ_ADAPTERS_MAX_LEN) {
        std::snprintf(g_aerr, sizeof g_aerr, "probe %u is longer than %u letters", j, (unsigned)SCFQ_ADAPTERS_MAX_LEN);
        return false;
      }
      const unsigned char b = (unsigned char)p[len];
      const uint64_t code = b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : 4;
      if (code > 3) {
        std::snprintf(g_aerr, sizeof g_aerr, "probe %u holds the byte 0x%02x at %u: only A C G T are allowed", j, (unsigned)b, len);
        return false;
      }
      word |= code << (62 - 2 * len);
    }
    pr->word[j] = word;
    pr->mask[j] = ~0ull << (64 - 2 * len);
    pr->len[j] = len;
  }
  if (cap > SCFQ_ADAPTERS_MAX_CAP) {
    std::snprintf(g_aerr, sizeof g_aerr, "cap %llu is above %llu rows", (unsigned long long)cap, (unsigned long long)SCFQ_ADAPTERS_MAX_CAP);
    return false;
  }
  return true;
}

// d_in: the whole input, resident; rows_host / cap: the caller's rows
int adapters_device(const uint8_t* d_in, uint64_t n, const AdProbes& pr, scfq_adapter_row* rows_host, uint64_t cap, scfq_adapter_summary* out,
                    hipStream_t stream) {
  for (double& m : g_stage_ms) m = 0;
  out->input_bytes = n;
  out->n_probes = pr.n;
  bool wide = false;
  for (uint32_t j = 0; j < pr.n; ++j) { out->probe_len[j] = pr.len[j]; wide = wide || pr.len[j] > 16; }
  uint64_t lines = 0;
  DevBuf line_off, first, stats, table;
  int rc = SCFQ_OK;
  bool has_cr = true;
  {
    const auto t_a = std::chrono::steady_clock::now();
    if ((rc = scfq_scratch::build_line_index(d_in, n, stream, g_aerr, line_off, &lines, &has_cr))) return rc;
    g_stage_ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_a).count();
  }
  const uint64_t reads = (lines + 3) / 4;
  out->lines = lines;
  out->reads = reads;
  if (reads >= (1ull << 31)) { std::snprintf(g_aerr, sizeof g_aerr, "more than 2^31 records in one input"); return SCFQ_EARG; }
  const uint64_t first_bytes = reads * pr.n * 4;
  if ((rc = first.alloc(first_bytes, stream, g_aerr)) || (rc = stats.alloc(kStWords * 8, stream, g_aerr))) return rc;
  static const bool timing = scfq_scratch::env_switch("SCFQ_ADAPTERS_TIMING");
  scfq_scratch::StageClock clk(stream, timing);
  if (first_bytes) SCFQ_SCRATCH_CHK(g_aerr, hipMemsetAsync(first.p, 0xff, first_bytes, stream));
  SCFQ_SCRATCH_CHK(g_aerr, hipMemsetAsync(stats.p, 0, kStWords * 8, stream));
  if (reads) {
    hipLaunchKernelGGL(ad_lens, dim3((unsigned)((reads + 255) / 256)), dim3(256), 0, stream, d_in, n, line_off.as<uint64_t>(), lines, has_cr,
                       stats.as<unsigned long long>());
    SCFQ_SCRATCH_CHK(g_aerr, hipGetLastError());
  }
  clk.mark(0);
  if (lines) {
    const uint32_t shift = (uint32_t)((uintptr_t)d_in & 15u);
    const uint64_t chunks = (shift + n + 15) / 16;
    const uint64_t steps = (chunks + kAdThreads - 1) / kAdThreads;
    const uint64_t spb = (steps + kAdMaxBlocks - 1) / kAdMaxBlocks;
    const unsigned blocks = (unsigned)((steps + spb - 1) / spb);
    if (wide)
      hipLaunchKernelGGL(ad_match<true>, dim3(blocks), dim3(kAdThreads), 0, stream, d_in, n, line_off.as<uint64_t>(), lines, shift, pr, chunks,
                         spb, first.as<uint32_t>(), stats.as<unsigned long long>());
    else
      hipLaunchKernelGGL(ad_match<false>, dim3(blocks), dim3(kAdThreads), 0, stream, d_in, n, line_off.as<uint64_t>(), lines, shift, pr, chunks,
                         spb, first.as<uint32_t>(), stats.as<unsigned long long>());
    SCFQ_SCRATCH_CHK(g_aerr, hipGetLastError());
  }
  clk.mark(1);
  uint64_t max_len = 0;
  SCFQ_SCRATCH_CHK(g_aerr, hipMemcpyAsync(&max_len, stats.as<uint64_t>() + kStMaxLen, 8, hipMemcpyDeviceToHost, stream));
  SCFQ_SCRATCH_CHK(g_aerr, hipStreamSynchronize(stream));
  out->max_seq_len = max_len;
  if (max_len >= kAdNone) {
    std::snprintf(g_aerr, sizeof g_aerr, "a sequence line of %llu bytes: positions are kept in 32 bits", (unsigned long long)max_len);
    return SCFQ_EARG;
  }
  const uint64_t positions = std::min(cap, max_len);
  out->positions = positions;
  const uint64_t rows = positions + 1;            // the last one is the tail
  if ((rc = table.alloc(rows * sizeof(scfq_adapter_row), stream, g_aerr))) return rc;
  SCFQ_SCRATCH_CHK(g_aerr, hipMemsetAsync(table.p, 0, rows * sizeof(scfq_adapter_row), stream));
  clk.mark(2);
  if (reads) {
    hipLaunchKernelGGL(ad_rows, dim3((unsigned)((reads + 255) / 256)), dim3(256), 0, stream, first.as<uint32_t>(), reads, pr.n, positions,
                       table.as<unsigned long long>());
    SCFQ_SCRATCH_CHK(g_aerr, hipGetLastError());
  }
  clk.mark(3);
  hipLaunchKernelGGL(ad_finish, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, table.as<unsigned long long>(), rows,
                     stats.as<unsigned long long>());
  SCFQ_SCRATCH_CHK(g_aerr, hipGetLastError());
  clk.mark(4);
  uint64_t h[kStWords];
  if (positions) SCFQ_SCRATCH_CHK(g_aerr, hipMemcpyAsync(rows_host, table.p, positions * sizeof(scfq_adapter_row), hipMemcpyDeviceToHost, stream));
  SCFQ_SCRATCH_CHK(g_aerr, hipMemcpyAsync(&out->tail, table.as<scfq_adapter_row>() + positions, sizeof(scfq_adapter_row), hipMemcpyDeviceToHost, stream));
  SCFQ_SCRATCH_CHK(g_aerr, hipMemcpyAsync(h, stats.p, sizeof h, hipMemcpyDeviceToHost, stream));
  SCFQ_SCRATCH_CHK(g_aerr, hipStreamSynchronize(stream));
  for (uint32_t j = 0; j < SCFQ_ADAPTERS_MAX_PROBES; ++j) {
    out->hits[j] = h[kStHits + j];
    out->total.first[j] = h[kStTotal + j];
  }
  out->total.any = h[kStTotal + SCFQ_ADAPTERS_MAX_PROBES];
  g_stage_ms[1] = clk.between(0, 1);
  g_stage_ms[2] = clk.between(2, 3);
  g_stage_ms[3] = clk.between(3, 4);
  return SCFQ_OK;
}

}  // namespace

extern "C" {

const char* scfq_adapters_error_detail(void) { return g_aerr; }

int scfq_debug_adapters_stages(double* ms, uint32_t cap) { return scfq_scratch::copy_stage_ms(g_stage_ms, ms, cap); }

int scfq_adapters_buffer(const void* ptr, uint64_t n, int is_device, const char* const* probes, uint32_t n_probes, scfq_adapter_row* rows_host,
                         uint64_t cap, scfq_adapter_summary* out) {
  g_aerr[0] = '\0';
  AdProbes pr;
  if (!args_ok(probes, n_probes, rows_host, cap, out, &pr) || (!ptr && n)) return SCFQ_EARG;
  scfq_scratch::clear_keep_size(out);
  scfq_scratch::ResidentInput in;
  int rc = in.from_buffer(ptr, n, is_device != 0, is_device != 0, g_aerr);
  if (rc) return rc;
  rc = adapters_device(in.d_in, n, pr, rows_host, cap, out, in.stream);
  if (rc == SCFQ_OK) in.mark_clean();      // (its last act was to wait for the stream)
  return rc;
}

int scfq_adapters_file(const char* path, const scfq_opts* opts, const char* const* probes, uint32_t n_probes, scfq_adapter_row* rows_host,
                       uint64_t cap, scfq_adapter_summary* out) {
  g_aerr[0] = '\0';
  AdProbes pr;
  if (!path || !args_ok(probes, n_probes, rows_host, cap, out, &pr)) return SCFQ_EARG;
  scfq_scratch::clear_keep_size(out);
  scfq_scratch::ResidentInput in;
  int rc = in.from_file(path, opts, g_aerr);
  if (rc) return rc;
  rc = adapters_device(in.d_in, in.n, pr, rows_host, cap, out, in.stream);
  if (rc == SCFQ_OK) in.mark_clean();      // (its last act was to wait for the stream)
  return rc;
}

}  // extern "C"

// scfq_kmers.hip — `sc fq-kmers` on the MI355X (gfx950): the k-mer spectrum (1 <= k <= 12) of the sequence lines.
// Not in the reference; definitions in include/sc_fqcount.h.
//
// The whole (inflated) input sits in HBM, as for fq-readstats and fq-cycles:
//   K5  line index            (scfq_scratch::build_line_index: line_off[0 .. lines], and whether the input holds "\r\n" at all)
//   M1  km_count              the hot path, partitioned by BYTES.  The input is cut into 16-byte chunks where its ADDRESS is a multiple
//                             of 16; a STEP is 512 chunks (8 KiB, a chunk per lane) and a block owns a run of consecutive steps, the
//                             same number for every block: a 3 MB line and 300 eight-base reads cost the same per byte, and no lane
//                             walks a line.  The block looks up the line of its first byte once (a binary search in line_off); from
//                             there the line of every byte follows from the '\n' the block sees: a wave prefix count per chunk, carried
//                             across the waves through LDS and across the steps in a register.  A lane loads its chunk and the next one
//                             (k - 1 <= 11 bytes of window, one more for the "\r\n" rule) and makes of the first 28 bytes a 2-bit word
//                             (and its reverse complement), a "not ACGT" mask and a "no text" mask ('\n', the '\r' before a real '\n',
//                             what lies outside the input); the windows that START in its chunk follow from shifts of those.  Equal
//                             indices of consecutive windows are added as one (a lane's run, and a run of lanes whose sixteen windows
//                             are all the same k-mer): poly-A and poly-G would put a thousand adds on one address per wave otherwise.
//                               k <= 7:  32-bit counters in LDS (16 K words: 4^k entries in 16384 / 4^k, at most 64, copies by lane, so
//                                        that the four counters of k = 1 are not one address for 64 lanes), flushed to the 64-bit table
//                                        at the block's end (and every kKmFlushSteps steps, so that no counter wraps)
//                               k >= 8:  a no-return 64-bit atomic add on the table in HBM (512 KiB .. 128 MiB)
//                             windows, skipped and short_lines are per-lane registers, one atomic per wave at the block's end;
//                             short_lines is counted by the lane that holds a sequence line's (real or implied) '\n'.
//   M2  km_finish             one pass over the table: distinct, max_count and the sum of the entries (= kmers)
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

thread_local char g_kerr[scfq_scratch::kErrBytes] = "";
thread_local double g_stage_ms[4] = {0, 0, 0, 0};

using scfq_scratch::DevBuf;

constexpr uint32_t kKmThreads = 512;                 // a chunk per lane and step
constexpr uint32_t kKmWaves = kKmThreads / 64;
constexpr uint32_t kKmStepBytes = kKmThreads * 16;
constexpr uint32_t kKmMaxBlocks = 1024;
constexpr uint32_t kKmLdsWords = 1u << 14;           // tier A: 4^7 counters, or fewer in copies
constexpr uint32_t kKmFlushSteps = 1u << 16;         // tier A: steps of a block between two flushes of its LDS counters
static_assert((uint64_t)kKmFlushSteps * kKmStepBytes < (1ull << 32), "a 32-bit LDS counter holds every window a block sees between two flushes");
static_assert(SCFQ_KMERS_MAX_K == 12 && 2 * SCFQ_KMERS_MAX_K <= 32 && 16 + SCFQ_KMERS_MAX_K <= 28, "28 bytes per lane, a 32-bit index");

enum : uint32_t { kStWindows = 0, kStSkipped = 1, kStShort = 2, kStDistinct = 3, kStMax = 4, kStSum = 5, kStWords = 8 };

// OR of x >> 0 .. x >> (k - 1): bit i says whether any of bits i .. i + k - 1 is set
__device__ __forceinline__ uint32_t smear_down(uint32_t x, uint32_t k) {
  uint32_t done = 1;
  while (done < k) {
    const uint32_t sh = done < k - done ? done : k - done;
    x |= x >> sh;
    done += sh;
  }
  return x;
}

// M1.  kLds: the counters of the block are in LDS (k <= 7).  chunks: 16-byte chunks of the address grid that hold a byte of the input or the
// position behind its last byte; steps_per_block * kKmThreads of them per block.  shift: address of the input mod 16.
template <bool kLds>
__global__ __launch_bounds__(kKmThreads) void km_count(const uint8_t* base, uint64_t n, const uint64_t* line_off, uint64_t lines, uint32_t shift,
                                                      bool has_cr, uint32_t k, bool canonical, bool merge, uint64_t chunks,
                                                      uint64_t steps_per_block, unsigned long long* table, unsigned long long* stats) {
  __shared__ uint32_t cnt[kLds ? kKmLdsWords : 1];
  __shared__ uint32_t wave_nl[2][kKmWaves];
  __shared__ uint64_t first_line;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t kmask = (uint32_t)((1ull << (2 * k)) - 1u);
  // tier A: entry e, copy r -> cnt[(e << rsh) + r]
  uint32_t rsh = 0;
  if (kLds) { while (rsh < 6 && ((2u << (2 * k)) << rsh) <= kKmLdsWords) ++rsh; }      // copies = min(64, 16384 / 4^k)
  const uint32_t entries = 1u << (2 * k), rmask = (1u << rsh) - 1u;
  auto flush = [&]() {
    for (uint32_t e = threadIdx.x; e < entries; e += kKmThreads) {
      uint64_t sum = 0;
      for (uint32_t r = 0; r <= rmask; ++r) {
        const uint32_t at = (e << rsh) + ((r + e) & rmask);
        sum += cnt[at];
        cnt[at] = 0;
      }
      if (sum) atomicAdd(&table[e], (unsigned long long)sum);
    }
  };
  if (kLds) for (uint32_t i = threadIdx.x; i < (entries << rsh); i += kKmThreads) cnt[i] = 0;

  const uint64_t step0 = (uint64_t)blockIdx.x * steps_per_block;
  const uint64_t c_first = step0 * kKmThreads;                       // (c_first < chunks: the grid is sized so)
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
  uint64_t n_windows = 0, n_skipped = 0, n_short = 0;

  for (uint64_t st = 0; st < steps_per_block; ++st) {
    const uint64_t c0 = c_first + st * kKmThreads;
    if (c0 >= chunks) break;                                         // (block-uniform)
    const uint64_t c = c0 + threadIdx.x;
    const int64_t o = 16 * (int64_t)c - (int64_t)shift;              // offset of this lane's byte 0; bytes [o, o + 28) are looked at
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t outside = 0xffffffffu;                                  // bytes that are not the input's
    if (c < chunks) {
      if (o >= 0 && o + 32 <= (int64_t)n) {
        const uint4 q0 = *reinterpret_cast<const uint4*>(base + o);  // (aligned: shift + o = 0 mod 16)
        const uint4 q1 = *reinterpret_cast<const uint4*>(base + o + 16);
        w[0] = q0.x; w[1] = q0.y; w[2] = q0.z; w[3] = q0.w; w[4] = q1.x; w[5] = q1.y; w[6] = q1.z; w[7] = q1.w;
        outside = 0;
      } else {
        // the input's first chunk and its last ones: only its own bytes are read
        for (int i = 0; i < 32; ++i) {
          const int64_t p = o + i;
          if (p >= 0 && p < (int64_t)n) {
            w[i >> 2] |= (uint32_t)base[p] << (8 * (i & 3));
            outside &= ~(1u << i);
          }
        }
      }
    }
    // bytes 0 .. 27: the 2-bit word with byte 0 on top, its reverse complement with byte 0 at the bottom, and the masks
    uint64_t fw = 0, rv = 0;
    uint32_t bad = 0, nl = 0, cr = 0;
#pragma unroll
    for (int i = 0; i < 28; ++i) {
      const uint32_t b = (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
      const uint32_t code = ((b >> 1) & 3u) ^ ((b >> 2) & 1u);                       // A C G T -> 0 1 2 3
      const bool ok = ((0x54474341u >> (8 * code)) & 0xffu) == b;
      if (i < 27) {
        fw |= (uint64_t)code << (2 * (26 - i));
        rv |= (uint64_t)(3u - code) << (2 * i);
      }
      bad |= (ok ? 0u : 1u) << i;
      nl |= (b == '\n' ? 1u : 0u) << i;
      cr |= (b == '\r' ? 1u : 0u) << i;
    }
    nl &= ~outside;
    uint32_t no_text = nl | outside;
    if (has_cr) no_text |= cr & (nl >> 1);                           // the '\r' directly before a real '\n'

    // the line of this lane's byte 0
    const uint32_t nl16 = nl & 0xffffu;
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
    for (uint32_t v = 0; v < kKmWaves; ++v) {
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
    const uint32_t win = in_seq & ~smear_down(no_text, k) & 0xffffu;
    const uint32_t masked = smear_down(bad, k);
    const uint32_t km = win & ~masked;
    n_windows += (uint32_t)__builtin_popcount(win);
    n_skipped += (uint32_t)__builtin_popcount(win & masked);

    auto emit = [&](uint32_t idx, uint32_t times) {
      if (kLds) atomicAdd(&cnt[(idx << rsh) + (lane & rmask)], times);
      else atomicAdd(&table[idx], (unsigned long long)times);       // (the value is not used: no return)
    };
    uint32_t run_idx = 0, run_cnt = 0;
    if (km) {
      const uint32_t top = 2 * (27 - k);                             // window i: fw >> (top - 2 i)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        if (km & (1u << i)) {
          uint32_t idx = (uint32_t)(fw >> (top - 2 * i)) & kmask;
          if (canonical) {
            const uint32_t rc = (uint32_t)(rv >> (2 * i)) & kmask;
            idx = rc < idx ? rc : idx;
          }
          if (run_cnt && idx == run_idx) ++run_cnt;
          else {
            if (run_cnt) emit(run_idx, run_cnt);
            run_idx = idx;
            run_cnt = 1;
          }
        }
      }
    }
    if (merge) {
      // lanes whose sixteen windows are one k-mer, the same as the lane's before them, leave their adds to the first of the run
      const bool full = run_cnt == 16;
      const uint32_t prev_idx = __shfl_up(run_idx, 1, 64);
      const int prev_full = __shfl_up((int)full, 1, 64);
      const bool follows = full && lane > 0 && prev_full && prev_idx == run_idx;
      const uint64_t fm = __builtin_amdgcn_ballot_w64(follows);
      if (follows) run_cnt = 0;
      else if (full && lane < 63) run_cnt += 16u * (uint32_t)__builtin_ctzll(~(fm >> (lane + 1)));
    }
    if (run_cnt) emit(run_idx, run_cnt);

    if (kLds && (st + 1) % kKmFlushSteps == 0) {                     // (block-uniform)
      __syncthreads();
      flush();
      __syncthreads();
    }
  }
  if (kLds) {
    __syncthreads();
    flush();
  }
  n_windows = wave_sum(n_windows);
  n_skipped = wave_sum(n_skipped);
  n_short = wave_sum(n_short);
  if (lane == 0) {
    if (n_windows) atomicAdd(&stats[kStWindows], (unsigned long long)n_windows);
    if (n_skipped) atomicAdd(&stats[kStSkipped], (unsigned long long)n_skipped);
    if (n_short) atomicAdd(&stats[kStShort], (unsigned long long)n_short);
  }
}

// M2: distinct, max_count and the sum of the table
__global__ __launch_bounds__(256) void km_finish(const unsigned long long* table, uint64_t entries, unsigned long long* stats) {
  uint64_t distinct = 0, mx = 0, sum = 0;
  for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < entries; e += (uint64_t)gridDim.x * 256) {
    const uint64_t v = table[e];
    distinct += v != 0;
    mx = v > mx ? v : mx;
    sum += v;
  }
  distinct = wave_sum(distinct);
  sum = wave_sum(sum);
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0 && sum) {
    atomicAdd(&stats[kStDistinct], (unsigned long long)distinct);
    atomicAdd(&stats[kStSum], (unsigned long long)sum);
    atomicMax(&stats[kStMax], (unsigned long long)mx);
  }
}

bool args_ok(uint32_t k, uint32_t flags, const uint64_t* table_host, uint64_t cap, const scfq_kmer_summary* out) {
  if (!out || out->struct_size != sizeof(scfq_kmer_summary) || (!table_host && cap)) return false;
  if (k < 1 || k > SCFQ_KMERS_MAX_K) {
    std::snprintf(g_kerr, sizeof g_kerr, "k = %u is outside 1 .. %u", k, (unsigned)SCFQ_KMERS_MAX_K);
    return false;
  }
  if (flags & ~(uint32_t)SCFQ_KMERS_CANONICAL) {
    std::snprintf(g_kerr, sizeof g_kerr, "unknown flag bits 0x%x", flags & ~(uint32_t)SCFQ_KMERS_CANONICAL);
    return false;
  }
  const uint64_t entries = 1ull << (2 * k);
  if (cap && cap < entries) {
    std::snprintf(g_kerr, sizeof g_kerr, "cap %llu is below the %llu entries of k = %u (0 sizes)", (unsigned long long)cap, (unsigned long long)entries, k);
    return false;
  }
  return true;
}

// d_in: the whole input, resident; table_host / cap: the caller's table
int kmers_device(const uint8_t* d_in, uint64_t n, uint32_t k, uint32_t flags, uint64_t* table_host, uint64_t cap, scfq_kmer_summary* out,
                 hipStream_t stream) {
  for (double& m : g_stage_ms) m = 0;
  const uint64_t entries = 1ull << (2 * k);
  out->input_bytes = n;
  out->k = k;
  out->flags = flags;
  out->table_entries = entries;
  uint64_t lines = 0;
  DevBuf line_off, table, stats;
  int rc = SCFQ_OK;
  bool has_cr = true;
  {
    const auto t_a = std::chrono::steady_clock::now();
    if ((rc = scfq_scratch::build_line_index(d_in, n, stream, g_kerr, line_off, &lines, &has_cr))) return rc;
    g_stage_ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_a).count();
  }
  out->lines = lines;
  out->reads = (lines + 3) / 4;
  if (out->reads >= (1ull << 31)) { std::snprintf(g_kerr, sizeof g_kerr, "more than 2^31 records in one input"); return SCFQ_EARG; }
  if ((rc = table.alloc(entries * 8, stream, g_kerr)) || (rc = stats.alloc(kStWords * 8, stream, g_kerr))) return rc;
  static const bool timing = scfq_scratch::env_switch("SCFQ_KMERS_TIMING");
  static const bool merge = [] { const char* e = std::getenv("SCFQ_KMERS_MERGE"); return !e || std::atoi(e) != 0; }();
  scfq_scratch::StageClock clk(stream, timing);
  SCFQ_SCRATCH_CHK(g_kerr, hipMemsetAsync(table.p, 0, entries * 8, stream));
  SCFQ_SCRATCH_CHK(g_kerr, hipMemsetAsync(stats.p, 0, kStWords * 8, stream));
  clk.mark(0);
  if (lines) {
    const uint32_t shift = (uint32_t)((uintptr_t)d_in & 15u);
    const uint64_t chunks = (shift + n) / 16 + 1;      // the last one holds the position behind the input
    const uint64_t steps = (chunks + kKmThreads - 1) / kKmThreads;
    const uint64_t spb = (steps + kKmMaxBlocks - 1) / kKmMaxBlocks;
    const unsigned blocks = (unsigned)((steps + spb - 1) / spb);
    const bool canonical = (flags & SCFQ_KMERS_CANONICAL) != 0;
    if (k <= 7)
      hipLaunchKernelGGL(km_count<true>, dim3(blocks), dim3(kKmThreads), 0, stream, d_in, n, line_off.as<uint64_t>(), lines, shift, has_cr, k,
                         canonical, merge, chunks, spb, table.as<unsigned long long>(), stats.as<unsigned long long>());
    else
      hipLaunchKernelGGL(km_count<false>, dim3(blocks), dim3(kKmThreads), 0, stream, d_in, n, line_off.as<uint64_t>(), lines, shift, has_cr, k,
                         canonical, merge, chunks, spb, table.as<unsigned long long>(), stats.as<unsigned long long>());
    SCFQ_SCRATCH_CHK(g_kerr, hipGetLastError());
  }
  clk.mark(1);
  hipLaunchKernelGGL(km_finish, dim3((unsigned)std::min<uint64_t>((entries + 255) / 256, 2048)), dim3(256), 0, stream,
                     table.as<unsigned long long>(), entries, stats.as<unsigned long long>());
  SCFQ_SCRATCH_CHK(g_kerr, hipGetLastError());
  clk.mark(2);
  uint64_t h[kStWords] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (cap) SCFQ_SCRATCH_CHK(g_kerr, hipMemcpyAsync(table_host, table.p, entries * 8, hipMemcpyDeviceToHost, stream));
  SCFQ_SCRATCH_CHK(g_kerr, hipMemcpyAsync(h, stats.p, sizeof h, hipMemcpyDeviceToHost, stream));
  clk.mark(3);
  SCFQ_SCRATCH_CHK(g_kerr, hipStreamSynchronize(stream));
  out->windows = h[kStWindows];
  out->kmers = h[kStSum];
  out->skipped = h[kStSkipped];
  out->short_lines = h[kStShort];
  out->distinct = h[kStDistinct];
  out->max_count = h[kStMax];
  g_stage_ms[1] = clk.between(0, 1);
  g_stage_ms[2] = clk.between(1, 2);
  g_stage_ms[3] = clk.between(2, 3);
  return SCFQ_OK;
}

}  // namespace

extern "C" {

const char* scfq_kmers_error_detail(void) { return g_kerr; }

int scfq_debug_kmers_stages(double* ms, uint32_t cap) { return scfq_scratch::copy_stage_ms(g_stage_ms, ms, cap); }

int scfq_kmers_buffer(const void* ptr, uint64_t n, int is_device, uint32_t k, uint32_t flags, uint64_t* table_host, uint64_t cap,
                      scfq_kmer_summary* out) {
  g_kerr[0] = '\0';
  if (!args_ok(k, flags, table_host, cap, out) || (!ptr && n)) return SCFQ_EARG;
  scfq_scratch::clear_keep_size(out);
  scfq_scratch::ResidentInput in;
  int rc = in.from_buffer(ptr, n, is_device != 0, is_device != 0, g_kerr);
  if (rc) return rc;
  rc = kmers_device(in.d_in, n, k, flags, table_host, cap, out, in.stream);
  if (rc == SCFQ_OK) in.mark_clean();      // (its last act was to wait for the stream)
  return rc;
}

int scfq_kmers_file(const char* path, const scfq_opts* opts, uint32_t k, uint32_t flags, uint64_t* table_host, uint64_t cap,
                    scfq_kmer_summary* out) {
  g_kerr[0] = '\0';
  if (!path || !args_ok(k, flags, table_host, cap, out)) return SCFQ_EARG;
  scfq_scratch::clear_keep_size(out);
  scfq_scratch::ResidentInput in;
  int rc = in.from_file(path, opts, g_kerr);
  if (rc) return rc;
  rc = kmers_device(in.d_in, in.n, k, flags, table_host, cap, out, in.stream);
  if (rc == SCFQ_OK) in.mark_clean();      // (its last act was to wait for the stream)
  return rc;
}

}  // extern "C"

// scfq_cycles.hip — `sc fq-cycles` on the MI355X (gfx950): base composition and quality position by position.
// Not in the reference; definitions in include/sc_fqcount.h.
//
// The whole (inflated) input sits in HBM, as for fq-readstats:
//   K5  line index            (scfq_scratch::build_line_index: line_off[0 .. lines], and whether the input holds "\r\n" at all)
//   C0  cy_lines              a pass over line_off.  Only the odd lines count (4i+1 sequence, 4i+3 quality): odd line k is line 2k+1,
//                             a sequence line when k is even.  A block per GROUP of 2048 odd lines: the longest text of either kind
//                             (global maxima) and the group's longest line, which says how many position WINDOWS of 1024 the group needs.
//       exclusive scan        (rocprim) of the windows per group: block b of C1 -> (group, window)
//   C1  cy_count              the hot path.  A block owns one window of one group: at most 2048 x 1 KiB of input, whatever the line
//                             lengths are, and every line of it at the SAME positions — the counters of those positions are 7 x 32 bit in
//                             LDS (8 arrays, numbered by the letter's bits; one is unused).  A line is cut into 16-byte chunks where its ADDRESS is a multiple of 16 (one aligned load per lane
//                             for any pointer); window w of a line is its chunks [64w, 64w + 64).  L = 4 .. 64 lanes work on a line, as
//                             many as the group's longest line has chunks in the window, so short reads fill the wave four or sixteen
//                             at a time.  The position of a byte is its address minus line_off: nothing is searched and nothing crosses
//                             blocks.  One LDS add per text byte: counter[letter (A C G T N other)][position] += 1, or for a quality byte
//                             the quality counter[position] += 1 << 20 | byte (2048 lines x 255 < 2^20, 1024 quality lines < 2^12).  A block adds
//                             every non-zero counter to the 64-bit table once; positions >= cap are summed in the block first.
//   C2  cy_finish             counters -> rows (bases = the six letter counters), and their sum
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

thread_local char g_cerr[scfq_scratch::kErrBytes] = "";
thread_local double g_stage_ms[4] = {0, 0, 0, 0};

using scfq_scratch::DevBuf;

constexpr uint32_t kCyThreads = 256;
constexpr uint32_t kCyGroup = 2048;                  // odd lines of a group (even: the parity of k inside a group is that of k)
constexpr uint32_t kCyWin = 1024;                    // positions of a window = 64 chunks
constexpr uint32_t kCyRel = kCyWin + 16;             // a line's chunks start up to 15 bytes before the line: slots per counter
constexpr uint32_t kCyPad = kCyRel + kCyRel / 16;    // one word of padding per 16: lanes 16 positions apart hit different banks
constexpr uint32_t kCyArr = 8;                       // counter arrays: A C T G other quality (count << 20 | sum) - N, see letter_of
constexpr uint32_t kQualShift = 20;
static_assert(kCyGroup % 2 == 0 && (uint64_t)kCyGroup * 255 < (1u << kQualShift) && kCyGroup / 2 < (1u << (32 - kQualShift)), "the packed quality counter");

// C0: a block per group.  nwin[g]: windows the group's longest line needs (its chunk grid starts up to 15 bytes before the line)
__global__ __launch_bounds__(kCyThreads) void cy_lines(const uint8_t* base, uint64_t n, const uint64_t* line_off, uint64_t odd, bool has_cr,
                                                      uint64_t groups, uint64_t* gmax, uint64_t* nwin, unsigned long long* mx) {
  __shared__ uint64_t red[2][kCyThreads / 64];
  const uint64_t g = blockIdx.x;
  uint64_t ms = 0, mq = 0;
  for (uint32_t i = threadIdx.x; i < kCyGroup; i += kCyThreads) {
    const uint64_t k = g * kCyGroup + i;
    if (k >= odd) break;
    uint64_t s, e;
    line_span(base, n, line_off, 2 * k + 1, s, e, has_cr);      // (2k + 2 <= lines)
    const uint64_t len = e - s;
    if (i & 1) mq = len > mq ? len : mq; else ms = len > ms ? len : ms;
  }
  ms = wave_max(ms);
  mq = wave_max(mq);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = ms; red[1][threadIdx.x >> 6] = mq; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t k = 1; k < kCyThreads / 64; ++k) { ms = red[0][k] > ms ? red[0][k] : ms; mq = red[1][k] > mq ? red[1][k] : mq; }
    const uint64_t m = ms > mq ? ms : mq;
    gmax[g] = m;
    nwin[g] = m ? (m + 15 + kCyWin - 1) / kCyWin : 0;
    if (ms) atomicMax(&mx[0], (unsigned long long)ms);
    if (mq) atomicMax(&mx[1], (unsigned long long)mq);
    if (g == 0) nwin[groups] = 0;      // (the scan's last entry is the number of blocks)
  }
}

// the counter array of a sequence byte: bits 1 .. 3 tell A C T G N apart (0 1 2 3 7); any other byte that lands on one of their
// numbers, or on 4 5 6, is not the letter that belongs there and counts as "other"
constexpr uint32_t kArrA = 0, kArrC = 1, kArrT = 2, kArrG = 3, kArrOther = 4, kArrQual = 5, kArrN = 7;
__device__ __forceinline__ uint32_t letter_of(uint32_t b) {
  const uint32_t h = (b >> 1) & 7u;
  const uint32_t expect = (uint32_t)(0x4e00000047544341ull >> (8 * h)) & 0xffu;      // 'A' 'C' 'T' 'G' 0 0 0 'N'
  return expect == b ? h : kArrOther;
}

struct CyItem {      // what a lane holds of its chunk
  uint32_t w[4];
  int lo, hi;        // its text bytes: [lo, hi) of 16
  uint32_t slot;     // a quality line << 16 | slot of byte 0
};

// C1
__global__ __launch_bounds__(kCyThreads) void cy_count(const uint8_t* base, uint64_t n, const uint64_t* line_off, uint64_t odd, uint32_t shift,
                                                      bool has_cr, const uint64_t* gbase, uint64_t groups, const uint64_t* gmax, uint64_t cycles,
                                                      unsigned long long* table) {
  __shared__ uint32_t cnt[kCyArr * kCyPad];
  // block -> (group, window): the first entry of gbase above the block number ends the group's run (gbase[groups] = blocks)
  const uint64_t b = blockIdx.x;
  uint64_t a = 0, h = groups;
  while (a < h) {
    const uint64_t m = a + (h - a) / 2;
    if (gbase[m] > b) h = m; else a = m + 1;
  }
  const uint64_t g = a - 1, w = b - gbase[g], gm = gmax[g];
  const uint64_t wlo = w * kCyWin;                                           // (wlo < gm + 15)
  const uint32_t ext = (uint32_t)std::min<uint64_t>(kCyWin, gm + 15 - wlo);  // bytes of the longest line's chunk grid in this window
  const uint32_t chunks = (ext + 15) / 16;
  uint32_t lsh = 2;
  while ((1u << lsh) < chunks) ++lsh;                                        // lanes per line: 4 .. 64
  const uint32_t rel_end = gm + 16 > wlo ? (uint32_t)std::min<uint64_t>(kCyRel, gm + 16 - wlo) : 0u;      // slots in use: position - wlo + 16
  for (uint32_t r = threadIdx.x; r < rel_end; r += kCyThreads) {
    const uint32_t idx = r + (r >> 4);
#pragma unroll
    for (uint32_t k = 0; k < kCyArr; ++k) cnt[k * kCyPad + idx] = 0;
  }
  __syncthreads();

  const uint32_t per_step = kCyThreads >> lsh, sub = threadIdx.x >> lsh, cl = threadIdx.x & ((1u << lsh) - 1);
  const uint64_t k0 = g * kCyGroup, kend = std::min<uint64_t>(odd, k0 + kCyGroup);
  const int64_t chunk0 = 16 * (int64_t)(w * (kCyWin / 16) + cl);             // this lane's chunk, in bytes behind the line's grid start
  // this lane's chunk of the line [s, e) (e: its real or implied '\n')
  auto fetch_line = [&](int64_t s, int64_t e, bool qual_line) -> CyItem {
    CyItem it;
    it.w[0] = it.w[1] = it.w[2] = it.w[3] = 0;
    it.lo = it.hi = 0;
    it.slot = 0;
    const uint32_t d = (shift + (uint32_t)s) & 15u;                           // the line starts d bytes into its first chunk
    const int64_t o = s - (int64_t)d + chunk0;
    if (o >= e) return it;
    const int64_t v0 = o > s ? o : s;
    int64_t v1 = o + 16 < e ? o + 16 : e;
    if (o >= 0 && o + 16 <= (int64_t)n) {
      const uint4 q = *reinterpret_cast<const uint4*>(base + o);             // (aligned: shift + o = 0 mod 16)
      it.w[0] = q.x; it.w[1] = q.y; it.w[2] = q.z; it.w[3] = q.w;
    } else {
      // the input's first or last chunk: only its own bytes are read
      for (int64_t p = v0; p < v1; ++p) {
        const uint32_t i = (uint32_t)(p - o);
        it.w[i >> 2] |= (uint32_t)base[p] << (8 * (i & 3));
      }
    }
    if (has_cr && e < (int64_t)n && v1 == e && e - 1 >= v0) {                 // the byte before a real '\n' is text of this chunk
      const uint32_t i = (uint32_t)(e - 1 - o);
      if (((it.w[i >> 2] >> (8 * (i & 3))) & 0xffu) == '\r') v1 = e - 1;
    }
    it.lo = (int)(v0 - o);
    it.hi = (int)(v1 - o);
    it.slot = (qual_line ? 1u << 16 : 0u) | (16 * cl + 16 - d);                 // byte i: position - wlo + 16 = 16 cl + 16 - d + i
    return it;
  };
  auto fetch = [&](uint64_t k) -> CyItem {
    if (k >= kend) { CyItem it; it.w[0] = it.w[1] = it.w[2] = it.w[3] = 0; it.lo = it.hi = 0; it.slot = 0; return it; }
    return fetch_line((int64_t)line_off[2 * k + 1], (int64_t)line_off[2 * k + 2] - 1, (k & 1) != 0);
  };
  auto count = [&](const CyItem& it) {
    if (it.lo >= it.hi) return;
    const bool qual = (it.slot >> 16) != 0;
    const uint32_t r0 = it.slot & 0xffffu;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if (i >= it.lo && i < it.hi) {
        const uint32_t c = (it.w[i >> 2] >> (8 * (i & 3))) & 0xffu;
        const uint32_t r = r0 + (uint32_t)i;
        const uint32_t arr = qual ? kArrQual : letter_of(c);
        atomicAdd(&cnt[arr * kCyPad + r + (r >> 4)], qual ? ((1u << kQualShift) | c) : 1u);
      }
    }
  };
  // the next step's loads are in flight while this step's bytes are counted
  if (lsh == 6) {
    // a wave per line.  Far into long reads most lines of the group have ended before this window: a wave looks at 64 lines at once
    // (a lane each) and visits only those that reach it
    const uint32_t lane = threadIdx.x & 63u;
    CyItem cur = fetch(kend);
    for (uint64_t kb = k0 + 64 * (uint64_t)sub; kb < kend; kb += 64 * per_step) {
      const uint64_t k = kb + lane;
      int64_t s = 0, e = 0;
      if (k < kend) { s = (int64_t)line_off[2 * k + 1]; e = (int64_t)line_off[2 * k + 2] - 1; }
      uint64_t reach = __builtin_amdgcn_ballot_w64(s - (int64_t)((shift + (uint32_t)s) & 15u) + 16 * (int64_t)(w * (kCyWin / 16)) < e);
      while (reach) {
        const int src = __builtin_ctzll(reach);
        reach &= reach - 1;
        const CyItem nxt = fetch_line(__shfl((long long)s, src, 64), __shfl((long long)e, src, 64), ((kb + (uint64_t)src) & 1) != 0);
        count(cur);
        cur = nxt;
      }
    }
    count(cur);
  } else {
    CyItem cur = fetch(k0 + sub);
    for (uint64_t kb = k0; kb < kend; kb += per_step) {
      const CyItem nxt = fetch(kb + per_step + sub);
      count(cur);
      cur = nxt;
    }
  }
  __syncthreads();

  // every non-zero counter once; what lies at or behind `cycles` is summed here first
  uint64_t tl[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (uint32_t r = threadIdx.x; r < rel_end; r += kCyThreads) {
    if (wlo + r < 16) continue;                       // (before the line: never counted)
    const uint64_t p = wlo + r - 16;
    const uint32_t idx = r + (r >> 4);
    uint32_t v[8];
    v[0] = cnt[kArrA * kCyPad + idx]; v[1] = cnt[kArrC * kCyPad + idx]; v[2] = cnt[kArrG * kCyPad + idx]; v[3] = cnt[kArrT * kCyPad + idx];
    v[4] = cnt[kArrN * kCyPad + idx]; v[5] = cnt[kArrOther * kCyPad + idx];
    const uint32_t q = cnt[kArrQual * kCyPad + idx];
    v[6] = q >> kQualShift;
    v[7] = q & ((1u << kQualShift) - 1u);
    if (p < cycles) {
#pragma unroll
      for (uint32_t k = 0; k < 8; ++k) if (v[k]) atomicAdd(&table[8 * p + k], (unsigned long long)v[k]);
    } else {
#pragma unroll
      for (uint32_t k = 0; k < 8; ++k) tl[k] += v[k];
    }
  }
  if (wlo + kCyWin > cycles) {                        // (the same for the whole block)
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) {
      const uint64_t s = wave_sum(tl[k]);
      if ((threadIdx.x & 63) == 0 && s) atomicAdd(&table[8 * cycles + k], (unsigned long long)s);
    }
  }
}

// C2: table rows [0, cycles] hold A C G T N other quals qual_sum; they become scfq_cycle_row, and tot their sum (row `cycles` is the tail)
__global__ __launch_bounds__(256) void cy_finish(unsigned long long* table, uint64_t rows, unsigned long long* tot) {
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint64_t r[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (p < rows) {
    const uint64_t a = table[8 * p], c = table[8 * p + 1], g = table[8 * p + 2], t = table[8 * p + 3], nn = table[8 * p + 4], o = table[8 * p + 5];
    r[0] = a + c + g + t + nn + o; r[1] = a; r[2] = c; r[3] = g; r[4] = t; r[5] = nn; r[6] = table[8 * p + 6]; r[7] = table[8 * p + 7];
#pragma unroll
    for (uint32_t k = 0; k < 6; ++k) table[8 * p + k] = r[k];
  }
#pragma unroll
  for (uint32_t k = 0; k < 8; ++k) {
    const uint64_t s = wave_sum(r[k]);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(&tot[k], (unsigned long long)s);
  }
}

bool args_ok(const scfq_cycle_row* rows_host, uint64_t cap, const scfq_cycle_summary* out) {
  if (!out || out->struct_size != sizeof(scfq_cycle_summary) || (!rows_host && cap)) return false;
  if (cap > SCFQ_CYCLES_MAX_CAP) {
    std::snprintf(g_cerr, sizeof g_cerr, "cap %llu is above %llu rows", (unsigned long long)cap, (unsigned long long)SCFQ_CYCLES_MAX_CAP);
    return false;
  }
  return true;
}

// d_in: the whole input, resident; rows_host / cap: the caller's rows
int cycles_device(const uint8_t* d_in, uint64_t n, scfq_cycle_row* rows_host, uint64_t cap, scfq_cycle_summary* out, hipStream_t stream) {
  for (double& m : g_stage_ms) m = 0;
  out->input_bytes = n;
  uint64_t lines = 0;
  DevBuf line_off, gmax, nwin, gbase, mx, table, tot, tmp;
  int rc = SCFQ_OK;
  bool has_cr = true;
  {
    const auto t_a = std::chrono::steady_clock::now();
    if ((rc = scfq_scratch::build_line_index(d_in, n, stream, g_cerr, line_off, &lines, &has_cr))) return rc;
    g_stage_ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_a).count();
  }
  const uint64_t reads = (lines + 3) / 4;
  out->lines = lines;
  out->reads = reads;
  if (reads >= (1ull << 31)) { std::snprintf(g_cerr, sizeof g_cerr, "more than 2^31 records in one input"); return SCFQ_EARG; }
  const uint64_t odd = lines / 2;               // lines 1, 3, 5, ...: the sequence and quality lines
  if (odd == 0) return SCFQ_OK;
  const uint64_t groups = (odd + kCyGroup - 1) / kCyGroup;
  if ((rc = gmax.alloc(groups * 8, stream, g_cerr)) || (rc = nwin.alloc((groups + 1) * 8, stream, g_cerr)) || (rc = gbase.alloc((groups + 1) * 8, stream, g_cerr)) ||
      (rc = mx.alloc(16, stream, g_cerr)) || (rc = tot.alloc(64, stream, g_cerr)))
    return rc;
  static const bool timing = scfq_scratch::env_switch("SCFQ_CYCLES_TIMING");
  scfq_scratch::StageClock clk(stream, timing);
  clk.mark(0);
  SCFQ_SCRATCH_CHK(g_cerr, hipMemsetAsync(mx.p, 0, 16, stream));
  SCFQ_SCRATCH_CHK(g_cerr, hipMemsetAsync(tot.p, 0, 64, stream));
  hipLaunchKernelGGL(cy_lines, dim3((unsigned)groups), dim3(kCyThreads), 0, stream, d_in, n, line_off.as<uint64_t>(), odd, has_cr, groups,
                     gmax.as<uint64_t>(), nwin.as<uint64_t>(), mx.as<unsigned long long>());
  SCFQ_SCRATCH_CHK(g_cerr, hipGetLastError());
  size_t scan_bytes = 0;
  SCFQ_SCRATCH_CHK(g_cerr, rocprim::exclusive_scan(nullptr, scan_bytes, nwin.as<uint64_t>(), gbase.as<uint64_t>(), (uint64_t)0, (size_t)(groups + 1), rocprim::plus<uint64_t>(), stream));
  if ((rc = tmp.alloc(std::max<size_t>(scan_bytes, 16), stream, g_cerr))) return rc;
  SCFQ_SCRATCH_CHK(g_cerr, rocprim::exclusive_scan(tmp.p, scan_bytes, nwin.as<uint64_t>(), gbase.as<uint64_t>(), (uint64_t)0, (size_t)(groups + 1), rocprim::plus<uint64_t>(), stream));
  clk.mark(1);
  uint64_t h_mx[2] = {0, 0}, blocks = 0;
  SCFQ_SCRATCH_CHK(g_cerr, hipMemcpyAsync(h_mx, mx.p, 16, hipMemcpyDeviceToHost, stream));
  SCFQ_SCRATCH_CHK(g_cerr, hipMemcpyAsync(&blocks, gbase.as<uint64_t>() + groups, 8, hipMemcpyDeviceToHost, stream));
  SCFQ_SCRATCH_CHK(g_cerr, hipStreamSynchronize(stream));
  out->max_seq_len = h_mx[0];
  out->max_qual_len = h_mx[1];
  const uint64_t cycles = std::min(cap, std::max(h_mx[0], h_mx[1]));
  out->cycles = cycles;
  if (blocks >= (1ull << 31)) { std::snprintf(g_cerr, sizeof g_cerr, "input too large for one launch"); return SCFQ_EARG; }
  const uint64_t rows = cycles + 1;             // the last one is the tail
  if ((rc = table.alloc(rows * sizeof(scfq_cycle_row), stream, g_cerr))) return rc;
  SCFQ_SCRATCH_CHK(g_cerr, hipMemsetAsync(table.p, 0, rows * sizeof(scfq_cycle_row), stream));
  clk.mark(2);
  if (blocks) {
    const uint32_t shift = (uint32_t)((uintptr_t)d_in & 15u);
    hipLaunchKernelGGL(cy_count, dim3((unsigned)blocks), dim3(kCyThreads), 0, stream, d_in, n, line_off.as<uint64_t>(), odd, shift, has_cr,
                       gbase.as<uint64_t>(), groups, gmax.as<uint64_t>(), cycles, table.as<unsigned long long>());
    SCFQ_SCRATCH_CHK(g_cerr, hipGetLastError());
  }
  clk.mark(3);
  hipLaunchKernelGGL(cy_finish, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, table.as<unsigned long long>(), rows,
                     tot.as<unsigned long long>());
  SCFQ_SCRATCH_CHK(g_cerr, hipGetLastError());
  clk.mark(4);
  if (cycles) SCFQ_SCRATCH_CHK(g_cerr, hipMemcpyAsync(rows_host, table.p, cycles * sizeof(scfq_cycle_row), hipMemcpyDeviceToHost, stream));
  SCFQ_SCRATCH_CHK(g_cerr, hipMemcpyAsync(&out->tail, table.as<scfq_cycle_row>() + cycles, sizeof(scfq_cycle_row), hipMemcpyDeviceToHost, stream));
  SCFQ_SCRATCH_CHK(g_cerr, hipMemcpyAsync(&out->total, tot.p, sizeof(scfq_cycle_row), hipMemcpyDeviceToHost, stream));
  SCFQ_SCRATCH_CHK(g_cerr, hipStreamSynchronize(stream));
  g_stage_ms[1] = clk.between(0, 1);
  g_stage_ms[2] = clk.between(2, 3);
  g_stage_ms[3] = clk.between(3, 4);
  return SCFQ_OK;
}

}  // namespace

extern "C" {

const char* scfq_cycles_error_detail(void) { return g_cerr; }

int scfq_debug_cycles_stages(double* ms, uint32_t cap) { return scfq_scratch::copy_stage_ms(g_stage_ms, ms, cap); }

int scfq_cycles_buffer(const void* ptr, uint64_t n, int is_device, scfq_cycle_row* rows_host, uint64_t cap, scfq_cycle_summary* out) {
  g_cerr[0] = '\0';
  if (!args_ok(rows_host, cap, out) || (!ptr && n)) return SCFQ_EARG;
  scfq_scratch::clear_keep_size(out);
  scfq_scratch::ResidentInput in;
  int rc = in.from_buffer(ptr, n, is_device != 0, is_device != 0, g_cerr);
  if (rc) return rc;
  rc = cycles_device(in.d_in, n, rows_host, cap, out, in.stream);
  if (rc == SCFQ_OK) in.mark_clean();      // (its last act was to wait for the stream)
  return rc;
}

int scfq_cycles_file(const char* path, const scfq_opts* opts, scfq_cycle_row* rows_host, uint64_t cap, scfq_cycle_summary* out) {
  g_cerr[0] = '\0';
  if (!path || !args_ok(rows_host, cap, out)) return SCFQ_EARG;
  scfq_scratch::clear_keep_size(out);
  scfq_scratch::ResidentInput in;
  int rc = in.from_file(path, opts, g_cerr);
  if (rc) return rc;
  rc = cycles_device(in.d_in, in.n, rows_host, cap, out, in.stream);
  if (rc == SCFQ_OK) in.mark_clean();      // (its last act was to wait for the stream)
  return rc;
}

}  // extern "C"

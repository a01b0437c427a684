// scfq_fagc.hip — `sc fa-gc` on the MI355X (gfx950): GC content of windows around positions of a FASTA.
// Reference: src/fa_gc.nim, which reloads a chromosome and re-counts 2w + 1 bases for every (position, window) pair.  Here the
// input is read once into per-tile prefix tables, and an interval costs two tile reads whatever its length.  Definitions in
// include/sc_fqcount.h.
//
// The whole (inflated) input sits in HBM, cut into tiles of kFaTileBytes on the address grid (fa_tile_device.hpp):
//   F1  fa_tile_scan      the hot path, one read of the input, a wave per tile.  A tile is classified without knowing the line
//                         it starts in: its HEAD (the bytes before its first line start) is counted as if it were sequence, its
//                         REST needs nothing from outside, because every line in it shows its own first byte.  The record of a
//                         tile: (gc, acgt, bases) of head and rest, the header-line starts, whether it holds a line start, and
//                         whether the line open at its end is a header line.
//   F2  fa_tile_resolve   a scan (rocprim) over the records: a tile starts in the line kind the nearest earlier tile with a line
//                         start ends in, its head counts when that is a sequence line.  Out come the exclusive prefixes of
//                         (gc, acgt, bases) and of the header starts, and the start kind per tile.
//   F3  fa_contigs        tiles with a header start are read again: offset, global base rank and 256 bytes of text per contig
//   F4  fa_rank_count     the query kernel, a wave per endpoint g: (gc, acgt) among the bases of global rank < g, from a binary
//                         search in the base prefix, one tile read and a wave prefix sum.  [a, b) of contig c is
//                         F(rank_c + b) - F(rank_c + a).
// Everything is integer / byte work; there is no CPU fallback.
#include "../../include/sc_fqcount.h"
#include "../../include/sc_fqcount_debug.h"

#include <hip/hip_runtime.h>

#include <cstring>        // (rocprim's texture iterator calls memset from host code)

#include <rocprim/rocprim.hpp>

#include "fa_tile_device.hpp"
#include "scfq_record_device.hpp"
#include "scfq_scratch.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

namespace {

thread_local char g_ferr[scfq_scratch::kErrBytes] = "";
thread_local double g_stage_ms[4] = {0, 0, 0, 0};

using scfq_scratch::DevBuf;

constexpr uint32_t kFaThreads = 256;                  // four waves, a tile (an endpoint) each
constexpr uint32_t kFaWaves = kFaThreads / 64;
constexpr uint32_t kFaNameBytes = 256;                // header text kept per contig: a name of 255 bytes and its end
constexpr uint64_t kFaQueryChunk = 1ull << 22;        // endpoints per launch of F4

struct FaTileRec {
  uint32_t head_gc, head_acgt, head_bases;            // as if the tile started in a sequence line
  uint32_t rest_gc, rest_acgt, rest_bases;
  uint32_t hdr_starts;
  uint32_t flags;                                     // bit 0: holds a line start; bit 1: the line open at its end is a header line
};

// the scan's element: a run of tiles.  pend: counts that hold only when the run starts in a sequence line.
struct FaElem {
  uint64_t known[3], pend[3];
  uint64_t hdrs;
  uint64_t flags;                                     // as FaTileRec::flags
};
struct FaToElem {
  __host__ __device__ FaElem operator()(const FaTileRec& r) const {
    return FaElem{{r.rest_gc, r.rest_acgt, r.rest_bases}, {r.head_gc, r.head_acgt, r.head_bases}, r.hdr_starts, r.flags};
  }
};
struct FaCombine {      // a, then b: associative, not commutative
  __host__ __device__ FaElem operator()(const FaElem& a, const FaElem& b) const {
    FaElem o;
    const bool a_has = a.flags & 1u, b_counts = a_has && !(a.flags & 2u);
    for (int k = 0; k < 3; ++k) {
      o.known[k] = a.known[k] + b.known[k] + (b_counts ? b.pend[k] : 0);
      o.pend[k] = a.pend[k] + (a_has ? 0 : b.pend[k]);
    }
    o.hdrs = a.hdrs + b.hdrs;
    o.flags = (b.flags & 1u) ? b.flags : a.flags;
    return o;
  }
};

__device__ __forceinline__ int64_t lane_offset(uint64_t t, uint32_t step, uint32_t lane, uint32_t shift) {
  return (int64_t)(t * kFaTileBytes + step * kFaStepBytes + lane * 16u) - (int64_t)shift;
}

// F1.  shift: address of the input mod kFaTileBytes; tile t holds the input's bytes [t * kFaTileBytes - shift, ... + kFaTileBytes).
__global__ __launch_bounds__(kFaThreads) void fa_tile_scan(const uint8_t* base, uint64_t n, uint32_t shift, uint64_t tiles, FaTileRec* rec) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t t = (uint64_t)blockIdx.x * kFaWaves + (threadIdx.x >> 6);
  if (t >= tiles) return;                                            // (wave-uniform)
  FaCarry c = {false, false, false};
  // 16-bit fields (a tile has 4096 bytes): head gc / acgt / bases, and rest gc / acgt / bases / header starts
  uint64_t head = 0, rest = 0;
#pragma unroll
  for (uint32_t step = 0; step < kFaSteps; ++step) {
    const FaStep s = fa_step(base, n, lane_offset(t, step, lane, shift), lane, step == 0, c);
    const uint32_t in_rest = ~s.hdr & ~s.head;
    head += (uint64_t)__builtin_popcount(s.m.gc & s.head) | (uint64_t)__builtin_popcount(s.m.acgt & s.head) << 16 |
            (uint64_t)__builtin_popcount(s.m.base & s.head) << 32;
    rest += (uint64_t)__builtin_popcount(s.m.gc & in_rest) | (uint64_t)__builtin_popcount(s.m.acgt & in_rest) << 16 |
            (uint64_t)__builtin_popcount(s.m.base & in_rest) << 32 | (uint64_t)__builtin_popcount(s.hs) << 48;
  }
  head = wave_sum(head);
  rest = wave_sum(rest);
  if (lane == 0) {
    FaTileRec r;
    r.head_gc = (uint32_t)head & 0xffffu; r.head_acgt = (uint32_t)(head >> 16) & 0xffffu; r.head_bases = (uint32_t)(head >> 32) & 0xffffu;
    r.rest_gc = (uint32_t)rest & 0xffffu; r.rest_acgt = (uint32_t)(rest >> 16) & 0xffffu; r.rest_bases = (uint32_t)(rest >> 32) & 0xffffu;
    r.hdr_starts = (uint32_t)(rest >> 48);
    r.flags = (c.known ? 1u : 0u) | (c.known && c.hdr ? 2u : 0u);
    rec[t] = r;
  }
}

// F2, behind the scan: entry t of `scanned` is the run of tiles [0, t); entry `tiles` is the whole input
__global__ __launch_bounds__(256) void fa_tile_resolve(const FaElem* scanned, uint64_t entries, uint64_t* gc_pre, uint64_t* acgt_pre,
                                                       uint64_t* base_pre, uint64_t* hdr_pre, uint8_t* start_hdr) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= entries) return;
  const FaElem e = scanned[t];
  gc_pre[t] = e.known[0] + e.pend[0];                                // (the input starts in a sequence line, or at a line start)
  acgt_pre[t] = e.known[1] + e.pend[1];
  base_pre[t] = e.known[2] + e.pend[2];
  hdr_pre[t] = e.hdrs;
  start_hdr[t] = (e.flags & 3u) == 3u;
}

// F3.  text: kFaNameBytes per contig, the bytes behind its '>' (as many as the input has)
__global__ __launch_bounds__(kFaThreads) void fa_contigs(const uint8_t* base, uint64_t n, uint32_t shift, uint64_t tiles, const FaTileRec* rec,
                                                       const uint64_t* base_pre, const uint64_t* hdr_pre, const uint8_t* start_hdr,
                                                       uint64_t contigs, uint64_t* c_off, uint64_t* c_rank, uint8_t* text) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t t = (uint64_t)blockIdx.x * kFaWaves + (threadIdx.x >> 6);
  if (t >= tiles || rec[t].hdr_starts == 0) return;                  // (wave-uniform)
  FaCarry c = {false, true, start_hdr[t] != 0};
  uint64_t run_bases = base_pre[t], run_hdr = hdr_pre[t];
  for (uint32_t step = 0; step < kFaSteps; ++step) {
    const int64_t o = lane_offset(t, step, lane, shift);
    const FaStep s = fa_step(base, n, o, lane, step == 0, c);
    const uint32_t counted = s.m.base & ~s.hdr;
    const uint64_t own = (uint64_t)__builtin_popcount(counted) | (uint64_t)__builtin_popcount(s.hs) << 32;
    uint64_t incl = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint64_t up = __shfl_up((unsigned long long)incl, d, 64);
      if (lane >= (uint32_t)d) incl += up;
    }
    const uint64_t total = __shfl((unsigned long long)incl, 63, 64);
    const uint64_t before = incl - own;
    for (uint32_t m = s.hs; m;) {
      const uint32_t b = (uint32_t)__builtin_ctz(m);
      m &= m - 1;
      const uint32_t below = (1u << b) - 1u;
      const uint64_t idx = run_hdr + (before >> 32) + (uint32_t)__builtin_popcount(s.hs & below);
      if (idx >= contigs) continue;                                  // (never: contigs is the sum of the records)
      const uint64_t off = (uint64_t)(o + (int64_t)b);
      c_off[idx] = off;
      c_rank[idx] = run_bases + (before & 0xffffffffu) + (uint32_t)__builtin_popcount(counted & below);
      for (uint32_t i = 0; i < kFaNameBytes && off + 1 + i < n; ++i) text[idx * kFaNameBytes + i] = base[off + 1 + i];
    }
    run_bases += total & 0xffffffffu;
    run_hdr += total >> 32;
  }
}

// F4.  out[2 e], out[2 e + 1]: gc and acgt among the bases of global rank < g[e] (g[e] <= base_pre[tiles])
__global__ __launch_bounds__(kFaThreads) void fa_rank_count(const uint8_t* base, uint64_t n, uint32_t shift, uint64_t tiles, const uint64_t* gc_pre,
                                                          const uint64_t* acgt_pre, const uint64_t* base_pre, const uint8_t* start_hdr,
                                                          const uint64_t* g, uint64_t endpoints, uint64_t* out) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t e = (uint64_t)blockIdx.x * kFaWaves + (threadIdx.x >> 6);
  if (e >= endpoints) return;                                        // (wave-uniform)
  const uint64_t rank = g[e];
  // the last t in [0, tiles] with base_pre[t] <= rank (base_pre[0] = 0): entry `tiles` when rank is the total
  uint64_t lo = 0, hi = tiles + 1;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (base_pre[mid] <= rank) lo = mid; else hi = mid;
  }
  const uint64_t t = lo;
  uint64_t r = rank - base_pre[t];                                   // bases of tile t below the cut
  uint64_t part = 0;                                                 // gc, acgt << 32
  if (r != 0 && t < tiles) {                                         // (r > 0 puts the cut inside tile t, which then has more than r bases)
    FaCarry c = {false, true, start_hdr[t] != 0};
    for (uint32_t step = 0; step < kFaSteps; ++step) {
      const FaStep s = fa_step(base, n, lane_offset(t, step, lane, shift), lane, step == 0, c);
      const uint32_t counted = s.m.base & ~s.hdr;
      const uint32_t own = (uint32_t)__builtin_popcount(counted);
      uint32_t incl = own;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if (lane >= (uint32_t)d) incl += up;
      }
      const uint32_t total = __shfl(incl, 63, 64);
      const uint32_t before = incl - own;
      // this lane's bases below the cut: its first k
      const uint32_t k = r > before ? (uint32_t)std::min<uint64_t>(r - before, own) : 0u;
      uint32_t above = counted;
      for (uint32_t i = 0; i < k; ++i) above &= above - 1;
      const uint32_t take = counted ^ above;
      part += (uint64_t)__builtin_popcount(s.m.gc & take) | (uint64_t)__builtin_popcount(s.m.acgt & take) << 32;
      if (r <= total) break;                                         // (wave-uniform)
      r -= total;
    }
    part = wave_sum(part);
  }
  if (lane == 0) {
    out[2 * e] = gc_pre[t] + (part & 0xffffffffu);
    out[2 * e + 1] = acgt_pre[t] + (part >> 32);
  }
}

struct Contig {
  std::string name;
  uint64_t header_offset = 0, rank = 0, length = 0;
};

}  // namespace

struct scfq_fa_index {
  scfq_scratch::ResidentInput in;          // the stream of the index, and the staged copy when the index owns one
  // (pool memory of in.stream: declared behind `in`, so returned before the stream is)
  DevBuf gc_pre, acgt_pre, base_pre, start_hdr;
  int device = 0;
  uint32_t shift = 0;
  uint64_t tiles = 0, total_bases = 0;
  std::vector<Contig> contigs;
  std::unordered_map<std::string, uint64_t> by_name;       // the first contig of a name
};

namespace {

// the device the index lives on is made current for a call and the caller's put back
struct DeviceScope {
  int prev = -1;
  bool switched = false;
  int enter(int dev, char* errbuf) {
    SCFQ_SCRATCH_CHK(errbuf, hipGetDevice(&prev));
    if (prev != dev) {
      SCFQ_SCRATCH_CHK(errbuf, hipSetDevice(dev));
      switched = true;
    }
    return SCFQ_OK;
  }
  ~DeviceScope() { if (switched) (void)hipSetDevice(prev); }
};

bool summary_ok(const scfq_fa_summary* sum) { return !sum || sum->struct_size == sizeof(scfq_fa_summary); }

// ix->in holds the input.  On success nothing is pending on the stream.
int index_device(scfq_fa_index* ix, scfq_fa_summary* sum) {
  for (double& m : g_stage_ms) m = 0;
  const uint8_t* d_in = ix->in.d_in;
  const uint64_t n = ix->in.n;
  hipStream_t stream = ix->in.stream;
  SCFQ_SCRATCH_CHK(g_ferr, hipGetDevice(&ix->device));
  ix->shift = n ? (uint32_t)((uintptr_t)d_in & (kFaTileBytes - 1)) : 0u;
  ix->tiles = n ? (ix->shift + n + kFaTileBytes - 1) / kFaTileBytes : 0;
  const uint64_t tiles = ix->tiles, entries = tiles + 1;
  static const bool timing = scfq_scratch::env_switch("SCFQ_FA_TIMING");
  scfq_scratch::StageClock clk(stream, timing);
  int rc = SCFQ_OK;
  DevBuf rec, scanned, hdr_pre, tmp;
  if ((rc = rec.alloc(entries * sizeof(FaTileRec), stream, g_ferr))) return rc;
  clk.mark(0);
  SCFQ_SCRATCH_CHK(g_ferr, hipMemsetAsync(rec.as<FaTileRec>() + tiles, 0, sizeof(FaTileRec), stream));   // (the scan's last input: nothing)
  if (tiles) {
    hipLaunchKernelGGL(fa_tile_scan, dim3((unsigned)((tiles + kFaWaves - 1) / kFaWaves)), dim3(kFaThreads), 0, stream, d_in, n, ix->shift, tiles,
                       rec.as<FaTileRec>());
    SCFQ_SCRATCH_CHK(g_ferr, hipGetLastError());
  }
  clk.mark(1);
  if ((rc = scanned.alloc(entries * sizeof(FaElem), stream, g_ferr)) || (rc = ix->gc_pre.alloc(entries * 8, stream, g_ferr)) ||
      (rc = ix->acgt_pre.alloc(entries * 8, stream, g_ferr)) || (rc = ix->base_pre.alloc(entries * 8, stream, g_ferr)) ||
      (rc = hdr_pre.alloc(entries * 8, stream, g_ferr)) || (rc = ix->start_hdr.alloc(entries, stream, g_ferr)))
    return rc;
  {
    auto first = rocprim::make_transform_iterator(rec.as<const FaTileRec>(), FaToElem());
    const FaElem nothing = {{0, 0, 0}, {0, 0, 0}, 0, 0};
    size_t scan_bytes = 0;
    SCFQ_SCRATCH_CHK(g_ferr, rocprim::exclusive_scan(nullptr, scan_bytes, first, scanned.as<FaElem>(), nothing, (size_t)entries, FaCombine(), stream));
    if ((rc = tmp.alloc(scan_bytes, stream, g_ferr))) return rc;
    SCFQ_SCRATCH_CHK(g_ferr, rocprim::exclusive_scan(tmp.p, scan_bytes, first, scanned.as<FaElem>(), nothing, (size_t)entries, FaCombine(), stream));
  }
  hipLaunchKernelGGL(fa_tile_resolve, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, stream, scanned.as<const FaElem>(), entries,
                     ix->gc_pre.as<uint64_t>(), ix->acgt_pre.as<uint64_t>(), ix->base_pre.as<uint64_t>(), hdr_pre.as<uint64_t>(),
                     ix->start_hdr.as<uint8_t>());
  SCFQ_SCRATCH_CHK(g_ferr, hipGetLastError());
  clk.mark(2);
  uint64_t totals[4] = {0, 0, 0, 0};      // gc, acgt, bases, contigs
  SCFQ_SCRATCH_CHK(g_ferr, hipMemcpyAsync(&totals[0], ix->gc_pre.as<uint64_t>() + tiles, 8, hipMemcpyDeviceToHost, stream));
  SCFQ_SCRATCH_CHK(g_ferr, hipMemcpyAsync(&totals[1], ix->acgt_pre.as<uint64_t>() + tiles, 8, hipMemcpyDeviceToHost, stream));
  SCFQ_SCRATCH_CHK(g_ferr, hipMemcpyAsync(&totals[2], ix->base_pre.as<uint64_t>() + tiles, 8, hipMemcpyDeviceToHost, stream));
  SCFQ_SCRATCH_CHK(g_ferr, hipMemcpyAsync(&totals[3], hdr_pre.as<uint64_t>() + tiles, 8, hipMemcpyDeviceToHost, stream));
  SCFQ_SCRATCH_CHK(g_ferr, hipStreamSynchronize(stream));
  const uint64_t contigs = totals[3];
  ix->total_bases = totals[2];
  std::vector<uint64_t> off(contigs), rank(contigs);
  std::vector<uint8_t> text(contigs * kFaNameBytes);
  if (contigs) {
    DevBuf c_off, c_rank, c_text;
    if ((rc = c_off.alloc(contigs * 8, stream, g_ferr)) || (rc = c_rank.alloc(contigs * 8, stream, g_ferr)) ||
        (rc = c_text.alloc(contigs * kFaNameBytes, stream, g_ferr)))
      return rc;
    clk.mark(3);
    hipLaunchKernelGGL(fa_contigs, dim3((unsigned)((tiles + kFaWaves - 1) / kFaWaves)), dim3(kFaThreads), 0, stream, d_in, n, ix->shift, tiles,
                       rec.as<const FaTileRec>(), ix->base_pre.as<const uint64_t>(), hdr_pre.as<const uint64_t>(), ix->start_hdr.as<const uint8_t>(),
                       contigs, c_off.as<uint64_t>(), c_rank.as<uint64_t>(), c_text.as<uint8_t>());
    SCFQ_SCRATCH_CHK(g_ferr, hipGetLastError());
    clk.mark(4);
    SCFQ_SCRATCH_CHK(g_ferr, hipMemcpyAsync(off.data(), c_off.p, contigs * 8, hipMemcpyDeviceToHost, stream));
    SCFQ_SCRATCH_CHK(g_ferr, hipMemcpyAsync(rank.data(), c_rank.p, contigs * 8, hipMemcpyDeviceToHost, stream));
    SCFQ_SCRATCH_CHK(g_ferr, hipMemcpyAsync(text.data(), c_text.p, contigs * kFaNameBytes, hipMemcpyDeviceToHost, stream));
    SCFQ_SCRATCH_CHK(g_ferr, hipStreamSynchronize(stream));
  }
  g_stage_ms[0] = clk.between(0, 1);
  g_stage_ms[1] = clk.between(1, 2);
  g_stage_ms[2] = clk.between(3, 4);
  ix->contigs.resize(contigs);
  for (uint64_t i = 0; i < contigs; ++i) {
    Contig& c = ix->contigs[i];
    const uint64_t have = std::min<uint64_t>(kFaNameBytes, n - off[i] - 1);
    const uint8_t* t = text.data() + i * kFaNameBytes;
    uint64_t len = 0;
    while (len < have && t[len] > 0x20) ++len;
    if (len == kFaNameBytes) {
      std::snprintf(g_ferr, sizeof g_ferr, "the name of contig %llu (header at byte %llu) is longer than %u bytes", (unsigned long long)i,
                    (unsigned long long)off[i], kFaNameBytes - 1);
      return SCFQ_EARG;
    }
    c.name.assign(reinterpret_cast<const char*>(t), len);
    c.header_offset = off[i];
    c.rank = rank[i];
    c.length = (i + 1 < contigs ? rank[i + 1] : ix->total_bases) - rank[i];
    ix->by_name.emplace(c.name, i);                     // (the first of a name stays)
  }
  if (sum) {
    sum->input_bytes = n;
    sum->tiles = tiles;
    sum->contigs = contigs;
    sum->bases = totals[2];
    sum->gc_bases = totals[0];
    sum->acgt_bases = totals[1];
    sum->orphan_bases = contigs ? rank[0] : totals[2];
  }
  return SCFQ_OK;
}

int finish_index(scfq_fa_index* ix, int rc, scfq_fa_index** out) {
  if (rc != SCFQ_OK) { delete ix; return rc; }
  ix->in.mark_clean();            // (the last act of index_device was to wait for the stream)
  *out = ix;
  return SCFQ_OK;
}

bool all_digits(const std::string& s) { return !s.empty() && s.find_first_not_of("0123456789") == std::string::npos; }

}  // namespace

extern "C" {

const char* scfq_fa_error_detail(void) { return g_ferr; }

int scfq_debug_fa_stages(double* ms, uint32_t cap) { return scfq_scratch::copy_stage_ms(g_stage_ms, ms, cap); }

int scfq_fa_index_buffer(const void* ptr, uint64_t n, int is_device, scfq_fa_index** out, scfq_fa_summary* sum) {
  g_ferr[0] = '\0';
  if (!out || !summary_ok(sum) || (!ptr && n)) return SCFQ_EARG;
  *out = nullptr;
  if (sum) scfq_scratch::clear_keep_size(sum);
  scfq_fa_index* ix = new (std::nothrow) scfq_fa_index;
  if (!ix) return SCFQ_ENOMEM;
  int rc = ix->in.from_buffer(ptr, n, is_device != 0, is_device != 0, g_ferr);
  if (rc == SCFQ_OK) rc = index_device(ix, sum);
  return finish_index(ix, rc, out);
}

int scfq_fa_index_file(const char* path, const scfq_opts* opts, scfq_fa_index** out, scfq_fa_summary* sum) {
  g_ferr[0] = '\0';
  if (!path || !out || !summary_ok(sum)) return SCFQ_EARG;
  *out = nullptr;
  if (sum) scfq_scratch::clear_keep_size(sum);
  scfq_fa_index* ix = new (std::nothrow) scfq_fa_index;
  if (!ix) return SCFQ_ENOMEM;
  int rc = ix->in.from_file(path, opts, g_ferr);
  if (rc == SCFQ_OK) rc = index_device(ix, sum);
  return finish_index(ix, rc, out);
}

void scfq_fa_index_free(scfq_fa_index* ix) { delete ix; }

int scfq_fa_contig_at(const scfq_fa_index* ix, uint64_t i, scfq_fa_contig* out) {
  g_ferr[0] = '\0';
  if (!ix || !out) return SCFQ_EARG;
  if (i >= ix->contigs.size()) {
    std::snprintf(g_ferr, sizeof g_ferr, "contig %llu of %llu", (unsigned long long)i, (unsigned long long)ix->contigs.size());
    return SCFQ_EARG;
  }
  const Contig& c = ix->contigs[i];
  out->name = c.name.c_str();
  out->name_len = c.name.size();
  out->header_offset = c.header_offset;
  out->length = c.length;
  return SCFQ_OK;
}

int scfq_fa_contig_find(const scfq_fa_index* ix, const char* name, uint64_t* i_out) {
  g_ferr[0] = '\0';
  if (!ix || !name || !i_out) return SCFQ_EARG;
  const auto it = ix->by_name.find(name);
  if (it == ix->by_name.end()) {
    std::snprintf(g_ferr, sizeof g_ferr, "no contig named \"%.200s\"", name);
    return SCFQ_EARG;
  }
  *i_out = it->second;
  return SCFQ_OK;
}

int scfq_fa_count_intervals(scfq_fa_index* ix, const scfq_fa_interval* q, uint64_t nq, scfq_fa_counts* out) {
  g_ferr[0] = '\0';
  if (!ix || (nq && (!q || !out))) return SCFQ_EARG;
  for (uint64_t i = 0; i < nq; ++i) {
    const bool known = q[i].contig < ix->contigs.size();
    if (!known || q[i].begin > q[i].end || q[i].end > ix->contigs[q[i].contig].length) {
      std::snprintf(g_ferr, sizeof g_ferr, "interval %llu: %s (contig %llu, [%llu, %llu))", (unsigned long long)i,
                    !known ? "no such contig" : q[i].begin > q[i].end ? "begin > end" : "end > length", (unsigned long long)q[i].contig,
                    (unsigned long long)q[i].begin, (unsigned long long)q[i].end);
      return SCFQ_EARG;
    }
  }
  if (nq == 0) return SCFQ_OK;
  DeviceScope dev;
  int rc = dev.enter(ix->device, g_ferr);
  if (rc) return rc;
  hipStream_t stream = ix->in.stream;
  const uint64_t per_launch = std::min<uint64_t>(2 * nq, kFaQueryChunk);      // (even)
  DevBuf d_g, d_f;
  if ((rc = d_g.alloc(per_launch * 8, stream, g_ferr)) || (rc = d_f.alloc(per_launch * 16, stream, g_ferr))) return rc;
  std::vector<uint64_t> g(per_launch), f(2 * per_launch);
  for (uint64_t i0 = 0; i0 < nq; i0 += per_launch / 2) {
    const uint64_t cells = std::min<uint64_t>(per_launch / 2, nq - i0), endpoints = 2 * cells;
    for (uint64_t i = 0; i < cells; ++i) {
      const uint64_t rank = ix->contigs[q[i0 + i].contig].rank;
      g[2 * i] = rank + q[i0 + i].begin;
      g[2 * i + 1] = rank + q[i0 + i].end;
    }
    SCFQ_SCRATCH_CHK(g_ferr, hipMemcpyAsync(d_g.p, g.data(), endpoints * 8, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(fa_rank_count, dim3((unsigned)((endpoints + kFaWaves - 1) / kFaWaves)), dim3(kFaThreads), 0, stream, ix->in.d_in, ix->in.n,
                       ix->shift, ix->tiles, ix->gc_pre.as<const uint64_t>(), ix->acgt_pre.as<const uint64_t>(), ix->base_pre.as<const uint64_t>(),
                       ix->start_hdr.as<const uint8_t>(), d_g.as<const uint64_t>(), endpoints, d_f.as<uint64_t>());
    SCFQ_SCRATCH_CHK(g_ferr, hipGetLastError());
    SCFQ_SCRATCH_CHK(g_ferr, hipMemcpyAsync(f.data(), d_f.p, endpoints * 16, hipMemcpyDeviceToHost, stream));
    SCFQ_SCRATCH_CHK(g_ferr, hipStreamSynchronize(stream));
    for (uint64_t i = 0; i < cells; ++i) {
      out[i0 + i].gc = f[4 * i + 2] - f[4 * i];
      out[i0 + i].acgt = f[4 * i + 3] - f[4 * i + 1];
      out[i0 + i].bases = q[i0 + i].end - q[i0 + i].begin;
    }
  }
  return SCFQ_OK;
}

// ---- host-only helpers -------------------------------------------------------------------------------------------------

// sci_parse_int, helpers.nim:230-237, and the ">= 1" rule of fa_gc.nim:69-71
int scfq_fa_parse_window(const char* text, uint64_t* window_out) {
  g_ferr[0] = '\0';
  if (!text || !window_out) return SCFQ_EARG;
  const std::string s(text);
  double value = 0;
  const size_t e = s.find('e');
  if (e != std::string::npos) {
    const std::string co = s.substr(0, e), ex = s.substr(e + 1);
    char* end = nullptr;
    const double coeff = std::strtod(co.c_str(), &end);
    const bool sign = !ex.empty() && (ex[0] == '-' || ex[0] == '+');
    if (co.empty() || co[0] == ' ' || *end || !all_digits(ex.substr(sign ? 1 : 0)) || ex.size() > 9) {
      std::snprintf(g_ferr, sizeof g_ferr, "invalid window: %.200s", text);
      return SCFQ_EARG;
    }
    value = std::trunc(std::pow(coeff * 10.0, (double)std::atol(ex.c_str())));
  } else {
    std::string d;
    for (const char ch : s) if (ch != ',') d += ch;
    const bool sign = !d.empty() && (d[0] == '-' || d[0] == '+');
    if (!all_digits(d.substr(sign ? 1 : 0)) || d.size() > 18) {
      std::snprintf(g_ferr, sizeof g_ferr, "invalid window: %.200s", text);
      return SCFQ_EARG;
    }
    value = (double)std::atoll(d.c_str());
  }
  if (!(value >= 1.0)) {
    std::snprintf(g_ferr, sizeof g_ferr, "Window lengths must be >= 1");
    return SCFQ_EARG;
  }
  if (!(value < 9.0e18)) {
    std::snprintf(g_ferr, sizeof g_ferr, "window out of range: %.200s", text);
    return SCFQ_EARG;
  }
  *window_out = (uint64_t)value;
  return SCFQ_OK;
}

// sub_seq, fa_gc.nim:29-37, and the range rule
int scfq_fa_gc_interval(int64_t pos, uint64_t window, uint64_t length, uint64_t* begin, uint64_t* end, int* out_of_range) {
  if (!begin || !end || !out_of_range) return SCFQ_EARG;
  *begin = *end = 0;
  *out_of_range = pos < 1 || (uint64_t)(pos - 1) >= length;
  if (*out_of_range) return SCFQ_OK;
  const uint64_t pos0 = (uint64_t)(pos - 1);
  *begin = pos0 > window ? pos0 - window : 0;
  *end = window >= length - pos0 - 1 ? length : pos0 + window + 1;       // min(length, pos0 + w + 1) without overflow
  return SCFQ_OK;
}

int scfq_format_fa_gc_value(uint64_t gc, uint64_t acgt, uint64_t window, char* buf, uint64_t cap) {
  if (!buf && cap) return SCFQ_EARG;
  std::string text = "nan";
  if (acgt) {
    int digits = 2;
    for (uint64_t w = window; ; w /= 10) { ++digits; if (w < 10) break; }
    const double scale = std::pow(10.0, digits);
    const double x = std::round((double)gc / (double)acgt * scale) / scale;
    // the shortest digits that read back as x, laid out as Python's repr(float)
    char sci[40];
    for (int p = 0; p <= 16; ++p) {
      std::snprintf(sci, sizeof sci, "%.*e", p, x);
      if (std::strtod(sci, nullptr) == x) break;
    }
    std::string mant;
    const char* ep = std::strchr(sci, 'e');
    for (const char* c = sci; c < ep; ++c) if (*c >= '0' && *c <= '9') mant += *c;
    const int exp10 = std::atoi(ep + 1);
    if (x == 0) text = "0.0";
    else if (exp10 < -4 || exp10 >= 16) {
      char tail[16];
      std::snprintf(tail, sizeof tail, "e%c%02d", exp10 < 0 ? '-' : '+', std::abs(exp10));
      text = mant.substr(0, 1) + (mant.size() > 1 ? "." + mant.substr(1) : "") + tail;
    } else if (exp10 < 0) text = "0." + std::string((size_t)(-exp10 - 1), '0') + mant;
    else {
      if ((int)mant.size() <= exp10) mant.append((size_t)(exp10 + 1 - (int)mant.size()), '0');
      text = mant.substr(0, (size_t)exp10 + 1) + "." + ((int)mant.size() > exp10 + 1 ? mant.substr((size_t)exp10 + 1) : "0");
    }
  }
  if (cap) std::snprintf(buf, (size_t)cap, "%s", text.c_str());
  return (int)text.size();
}

}  // extern "C"

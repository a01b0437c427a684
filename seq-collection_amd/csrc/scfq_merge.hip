// scfq_merge.hip — `sc fq-merge` on the MI355X (gfx950): overlapping read pairs become single reads, the rest stay pairs.
// Not in the reference; definitions in include/sc_fqcount.h.
//
// Both inputs sit in HBM whole (or the one interleaved input):
//   K5  line index            (scfq_scratch::build_line_index) of each input      } scfq_overlap.hpp: fq-insert-size's own code,
//   P1  is_overlap            d*, ov and mm of every pair into a table in pool memory } compiled once, in scfq_insert.hip
//   M1  mg_lengths            a thread per pair: the bytes the pair adds to each of the three outputs, summed per group of kMgGroup
//                             pairs (the scans run over groups, as fq-dedup's does), and the statistics that follow from the table
//                             alone, one atomic per block and counter
//       exclusive scans       one per output over the groups (rocprim), each with a last entry that is the output's size
//   M2  mg_write              the hot path: a wave per group.  Lanes 0 .. 31 look their pair up once (spans, lengths), a prefix over
//                             the lengths inside the wave gives every pair its place, then the pairs are written one after another by
//                             the whole wave: an unmerged record is a copy (wave_copy, or line by line where "\r\n" or a missing final
//                             newline makes the echo differ from the input), a merged one is built kMgRun positions per lane.
// M2 compares the three totals with the capacities before it stores anything: a result that does not fit leaves every output alone.
// It still walks the merged pairs then (and for outputs that are not asked for): took_mate1, took_mate2 and neither_valid are counted
// where the consensus is formed, so the statistics do not depend on what is written.
// Everything is integer / byte work; there is no CPU fallback.
#include "../../include/sc_fqcount.h"
#include "../../include/sc_fqcount_debug.h"

#include <cstring>        // (rocprim's texture iterator calls memset from host code)
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "scfq_reads_host.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

namespace {

thread_local char g_merr[scfq_scratch::kErrBytes] = "";
thread_local double g_stage_ms[4] = {0, 0, 0, 0};

using scfq_reads::Dest;
using scfq_reads::DevBuf;
using scfq_reads::finish;
using scfq_reads::Mode;

constexpr uint32_t kMgGroup = kRecGroup;      // pairs of a group: one wave of M2, one entry of the scans
constexpr uint32_t kMgWaves = 4;       // waves (groups) of a block of M2
constexpr uint32_t kMgRun = 4;         // consecutive positions of a merged read a lane builds and stores at a time: one 32-bit word
static_assert(kMgRun == 4, "a run is one 32-bit word");
// the counters: M1's six, then M2's three
enum { kMerged = 0, kNotOverlapped, kTooLong, kMergedBases, kOverlapBases, kMismatches, kTook1, kTook2, kNeither, kCounters };

// what a pair adds to the outputs and, for a merged pair, where its texts lie.  M1 and M2 both get it from here, so the lengths the
// scans saw are the lengths M2 writes
struct MgPair {
  uint64_t len_m, len_u1, len_u2;      // bytes for merged, unmerged 1, unmerged 2
  uint64_t len_first;                  // of len_u1, mate 1's record (interleaved input: mate 2's follows it)
  uint64_t hs, hl;                     // mate 1's header text
  uint64_t sa, qa, sb, qb;             // starts of A, QA, B, QB
  int32_t la, lb, qla, qlb, d;         // lengths (the quality texts cut to their sequence's), d*
  uint32_t kind;                       // 0 merged, 1 not overlapped, 2 too long
  uint32_t ov, mm;
};

__device__ __forceinline__ MgPair look_up(const RecInput& a, const RecInput& b, uint64_t stride, uint64_t second, uint64_t p, const scfq_overlap_rec* recs) {
  MgPair r = {};
  const scfq_overlap_rec rec = recs[p];
  const uint64_t i1 = p * stride, i2 = p * stride + second;
  if (rec.overlap == 0) {
    r.kind = rec.mismatches == 0xFFFFu ? 2u : 1u;
    r.len_first = echo_len(a, i1);
    const uint64_t l2 = echo_len(b, i2);
    r.len_u1 = second ? r.len_first + l2 : r.len_first;
    r.len_u2 = second ? 0 : l2;
    return r;
  }
  uint64_t e;
  text_span(a, 4 * i1, r.hs, e);
  r.hl = e - r.hs;
  text_span(a, 4 * i1 + 1, r.sa, e);
  r.la = (int32_t)(e - r.sa);                        // (a merged pair's reads are at most SCFQ_INSERT_MAX_LEN long)
  text_span(a, 4 * i1 + 3, r.qa, e);
  r.qla = (int32_t)std::min<uint64_t>(e - r.qa, (uint64_t)r.la);
  text_span(b, 4 * i2 + 1, r.sb, e);
  r.lb = (int32_t)(e - r.sb);
  text_span(b, 4 * i2 + 3, r.qb, e);
  r.qlb = (int32_t)std::min<uint64_t>(e - r.qb, (uint64_t)r.lb);
  r.d = rec.offset;
  r.ov = rec.overlap;
  r.mm = rec.mismatches;
  r.len_m = r.hl + 2ull * (uint64_t)(r.d + r.lb) + 5;
  return r;
}

// M1.  group_len: three arrays of n_groups + 1 entries, one after another (the last entry of each stays 0: the scan's total)
__global__ __launch_bounds__(256) void mg_lengths(RecInput a, RecInput b, uint64_t stride, uint64_t second, uint64_t pairs, const scfq_overlap_rec* recs,
                                                 uint64_t n_groups, uint64_t* group_len, unsigned long long* counters) {
  __shared__ uint64_t sum_sh[6][4];
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint64_t len[3] = {0, 0, 0}, c[6] = {0, 0, 0, 0, 0, 0};
  if (p < pairs) {
    const MgPair r = look_up(a, b, stride, second, p, recs);
    len[0] = r.len_m; len[1] = r.len_u1; len[2] = r.len_u2;
    c[kMerged] = r.kind == 0; c[kNotOverlapped] = r.kind == 1; c[kTooLong] = r.kind == 2;
    c[kMergedBases] = r.kind == 0 ? (uint64_t)(r.d + r.lb) : 0;
    c[kOverlapBases] = r.ov; c[kMismatches] = r.mm;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) store_group_len(len[k], k, p, pairs, n_groups, group_len);
  // the statistics: ONE atomic per block and counter (dd_count_marks: an atomic per wave on one address costs more than the kernel)
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const uint64_t s = wave_sum(c[k]);
    if ((threadIdx.x & 63) == 0) sum_sh[k][threadIdx.x >> 6] = s;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const uint64_t t = sum_sh[threadIdx.x][0] + sum_sh[threadIdx.x][1] + sum_sh[threadIdx.x][2] + sum_sh[threadIdx.x][3];
    if (t) atomicAdd(&counters[threadIdx.x], (unsigned long long)t);
  }
}

// the four bytes at base[pos .. pos + 4), byte k in bits 8k ..; a byte outside [0, n) reads as 0 and nothing outside is touched
__device__ __forceinline__ uint32_t load4(const uint8_t* base, uint64_t n, int64_t pos) {
  uint32_t v = 0;
  if (pos >= 0 && (uint64_t)pos + 4 <= n) {
    __builtin_memcpy(&v, base + pos, 4);             // arbitrarily aligned
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (pos + k >= 0 && (uint64_t)(pos + k) < n) v |= (uint32_t)base[pos + k] << (8 * k);
  }
  return v;
}

// valid(b) and comp(b): bits 1 and 2 of 'A' 'C' 'T' 'G' are 0 1 2 3
__device__ __forceinline__ bool is_acgt(uint32_t b) { return ((0x47544341u >> (8 * ((b >> 1) & 3u))) & 0xffu) == b; }
__device__ __forceinline__ uint32_t comp_of(uint32_t b) { return is_acgt(b) ? (0x43414754u >> (8 * ((b >> 1) & 3u))) & 0xffu : b; }

// the merged record of one pair, by the whole wave.  dst = nullptr: nothing is stored, the positions are only counted.
// Run k covers the positions [4k - ph, 4k - ph + 4) of the merged read, ph being the low two bits of the sequence's destination: the
// words of the sequence are stored aligned.  The quality text begins s + 3 bytes further on, so its words are aligned for one s in
// four; they are stored as words all the same (an unaligned 32-bit store is one instruction here), the first and last run of either
// text byte by byte.
__device__ __forceinline__ void write_merged(const RecInput& a, const RecInput& b, const MgPair& r, uint8_t* dst, uint32_t q0, uint32_t lane,
                                             uint32_t& took1, uint32_t& took2, uint32_t& neither) {
  const int s = r.d + r.lb;
  uint8_t* seq = dst + r.hl + 1;
  uint8_t* qual = seq + s + 3;
  if (dst) {
    for (uint64_t k = lane; k < r.hl; k += 64) dst[k] = a.base[r.hs + k];
    if (lane == 0) dst[r.hl] = '\n';
    if (lane == 1) seq[s] = '\n';
    if (lane == 2) seq[s + 1] = '+';
    if (lane == 3) seq[s + 2] = '\n';
    if (lane == 4) qual[s] = '\n';
  }
  const int ph = dst ? (int)((uintptr_t)seq & 3u) : 0;
  const int runs = (s + ph + (int)kMgRun - 1) / (int)kMgRun;
  for (int k = (int)lane; k < runs; k += 64) {
    const int x0 = (int)kMgRun * k - ph;                                   // (>= -3)
    // A and QA forward; B and QB backward: position x faces B[lb - 1 - (x - d)], so the word is loaded at the run's last position
    const int yb = r.lb - 1 - (x0 + 3 - r.d);
    const uint32_t wa = load4(a.base, a.n, (int64_t)r.sa + x0), wqa = load4(a.base, a.n, (int64_t)r.qa + x0);
    const uint32_t wb = __builtin_bswap32(load4(b.base, b.n, (int64_t)r.sb + yb)), wqb = __builtin_bswap32(load4(b.base, b.n, (int64_t)r.qb + yb));
    uint32_t out_b = 0, out_q = 0;
#pragma unroll
    for (int j = 0; j < (int)kMgRun; ++j) {
      const int x = x0 + j, y = r.lb - 1 - (x - r.d);                      // y: the index into B and QB
      const bool in = x >= 0 && x < s, cov_a = in && x < r.la, cov_c = in && x >= r.d, both = cov_a && cov_c;
      const uint32_t ba = (wa >> (8 * j)) & 0xffu, bc = comp_of((wb >> (8 * j)) & 0xffu);
      const uint32_t qa = x < r.qla ? (wqa >> (8 * j)) & 0xffu : q0, qc = y < r.qlb ? (wqb >> (8 * j)) & 0xffu : q0;
      const bool va = is_acgt(ba), vc = is_acgt(bc), differ = both && va && vc && ba != bc, none = both && !va && !vc;
      const bool a_wins = qa >= qc;                                        // mate 1 on a tie
      const uint32_t gap = qa > qc ? qa - qc : qc - qa;
      // the base: A's unless only C covers, or C is the valid one of the two, or both are valid, differ and C's quality is larger
      const bool take_c = !cov_a || (both && vc && (!va || (ba != bc && !a_wins)));
      uint32_t q = take_c ? qc : qa;                                       // one covers; exactly one valid
      q = (both && va && vc) ? (qa > qc ? qa : qc) : q;                    // both valid, equal
      q = differ ? std::min(q0 + std::max(2u, gap), 126u) : q;
      q = none ? (qa < qc ? qa : qc) : q;
      out_b |= (take_c ? bc : ba) << (8 * j);
      out_q |= q << (8 * j);
      took1 += differ && a_wins;
      took2 += differ && !a_wins;
      neither += none;
    }
    if (!dst) continue;
    if (x0 >= 0 && x0 + (int)kMgRun <= s) {
      *reinterpret_cast<uint32_t*>(seq + x0) = out_b;                      // aligned: seq + x0 = seq - ph + 4k
      __builtin_memcpy(qual + x0, &out_q, 4);
    } else {
#pragma unroll
      for (int j = 0; j < (int)kMgRun; ++j)
        if (x0 + j >= 0 && x0 + j < s) { seq[x0 + j] = (uint8_t)(out_b >> (8 * j)); qual[x0 + j] = (uint8_t)(out_q >> (8 * j)); }
    }
  }
}

// M2.  group_off: the three scanned arrays of M1's layout
__global__ __launch_bounds__(64 * kMgWaves) void mg_write(RecInput a, RecInput b, uint64_t stride, uint64_t second, uint64_t pairs, const scfq_overlap_rec* recs,
                                                         uint64_t n_groups, const uint64_t* group_off, RecOut om, RecOut o1, RecOut o2, uint32_t q0,
                                                         unsigned long long* counters) {
  __shared__ uint32_t sum_sh[3][kMgWaves];
  const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // (when one result is more than its output holds, nothing is written to any; the mates' votes are counted all the same)
  const bool fits = output_fits(om, 0, n_groups, group_off) && output_fits(o1, 1, n_groups, group_off) && output_fits(o2, 2, n_groups, group_off);
  uint8_t* const out_m = fits ? om.p : nullptr;
  uint8_t* const out_1 = fits ? o1.p : nullptr;
  uint8_t* const out_2 = fits ? o2.p : nullptr;
  const uint64_t g = (uint64_t)blockIdx.x * kMgWaves + wave;
  uint32_t took1 = 0, took2 = 0, neither = 0;
  if (g < n_groups) {
    const uint64_t p0 = g * kMgGroup;
    const uint32_t count = (uint32_t)std::min<uint64_t>(kMgGroup, pairs - p0);
    MgPair mine = {};
    mine.kind = 3;
    if (lane < count) mine = look_up(a, b, stride, second, p0 + lane, recs);
    const uint64_t len[3] = {mine.len_m, mine.len_u1, mine.len_u2};
    uint64_t at[3];
    place_units(len, g, n_groups, group_off, lane, at);
    for (uint32_t q = 0; q < count; ++q) {
      const uint32_t kind = (uint32_t)__shfl((int)mine.kind, (int)q, 64);
      if (kind == 0) {
        MgPair r;
        r.hs = bcast(mine.hs, q); r.hl = bcast(mine.hl, q);
        r.sa = bcast(mine.sa, q); r.qa = bcast(mine.qa, q); r.sb = bcast(mine.sb, q); r.qb = bcast(mine.qb, q);
        r.la = __shfl(mine.la, (int)q, 64); r.lb = __shfl(mine.lb, (int)q, 64); r.qla = __shfl(mine.qla, (int)q, 64);
        r.qlb = __shfl(mine.qlb, (int)q, 64); r.d = __shfl(mine.d, (int)q, 64);
        const uint64_t w = bcast(at[0], q);
        write_merged(a, b, r, out_m ? out_m + w : nullptr, q0, lane, took1, took2, neither);
      } else {
        const uint64_t p = p0 + q, first = bcast(mine.len_first, q), l1 = bcast(mine.len_u1, q), l2 = bcast(mine.len_u2, q);
        const uint64_t w1 = bcast(at[1], q), w2 = bcast(at[2], q);
        if (out_1) {
          echo_record(a, p * stride, out_1 + w1, first, lane);
          if (second) echo_record(b, p * stride + second, out_1 + w1 + first, l1 - first, lane);
        }
        if (out_2 && !second) echo_record(b, p * stride, out_2 + w2, l2, lane);
      }
    }
  }
  const uint32_t t1 = (uint32_t)wave_sum(took1), t2 = (uint32_t)wave_sum(took2), nv = (uint32_t)wave_sum(neither);
  if (lane == 0) { sum_sh[0][wave] = t1; sum_sh[1][wave] = t2; sum_sh[2][wave] = nv; }
  __syncthreads();
  if (threadIdx.x < 3) {
    uint32_t t = 0;
    for (uint32_t w = 0; w < kMgWaves; ++w) t += sum_sh[threadIdx.x][w];
    if (t) atomicAdd(&counters[kTook1 + threadIdx.x], (unsigned long long)t);
  }
}

struct Params { scfq_overlap::Params ov; uint32_t q0; };

bool args_ok(const scfq_merge_opts* opts, const scfq_merge_stats* st, Params& p) {
  if (!st || st->struct_size != sizeof(scfq_merge_stats)) return false;
  p.ov.flags = 0; p.ov.min_overlap = 30; p.ov.max_mm = 5; p.ov.max_pct = 20; p.q0 = 33;
  if (!opts) return true;
  if (opts->struct_size != sizeof(scfq_merge_opts)) return false;
  p.ov.flags = opts->flags; p.ov.min_overlap = opts->min_overlap; p.ov.max_mm = opts->max_mismatches; p.ov.max_pct = opts->max_mismatch_pct;
  p.q0 = opts->phred_offset;
  if (p.ov.flags & ~(uint32_t)SCFQ_MERGE_INTERLEAVED) { std::snprintf(g_merr, sizeof g_merr, "unknown flag bits 0x%x", p.ov.flags & ~(uint32_t)SCFQ_MERGE_INTERLEAVED); return false; }
  if (!scfq_overlap::params_in_range(p.ov, g_merr)) return false;
  if (p.q0 != 33 && p.q0 != 64) { std::snprintf(g_merr, sizeof g_merr, "phred_offset %u is not 33 or 64", p.q0); return false; }
  if (opts->reserved) { std::snprintf(g_merr, sizeof g_merr, "the reserved word is %u, not 0", opts->reserved); return false; }
  return true;
}

const char* const kDestName[3] = {"merged", "unmerged1", "unmerged2"};

int merge_device(const uint8_t* d1, uint64_t n1, const uint8_t* d2, uint64_t n2, bool interleaved, const Params& prm, bool own_outputs, Dest dst[3],
                 DevBuf own[3], bool check_caps, scfq_merge_stats* st, hipStream_t stream) {
  for (double& m : g_stage_ms) m = 0;
  st->input_bytes1 = n1;
  st->input_bytes2 = n2;
  st->min_overlap = prm.ov.min_overlap;
  st->max_mismatches = prm.ov.max_mm;
  st->max_mismatch_pct = prm.ov.max_pct;
  st->phred_offset = prm.q0;
  scfq_overlap::Indexed ix;
  int rc = SCFQ_OK;
  uint64_t pairs = 0;
  if ((rc = scfq_reads::index_units(d1, n1, d2, n2, interleaved ? Mode::interleaved : Mode::two, stream, g_merr, ix, &g_stage_ms[0], st, &pairs, nullptr))) return rc;
  if (pairs == 0) return SCFQ_OK;           // (three empty outputs: they fit into anything)
  const uint64_t n_groups = (pairs + kMgGroup - 1) / kMgGroup;
  DevBuf recs, acc, group_len, group_off, counters, tmp;
  scfq_reads::GroupScan gs(3, n_groups, group_len, group_off, stream, g_merr);
  if ((rc = recs.alloc(pairs * sizeof(scfq_overlap_rec), stream, g_merr)) || (rc = acc.alloc(scfq_overlap::kAccWords * 8, stream, g_merr)) || (rc = gs.alloc()) ||
      (rc = counters.alloc(kCounters * 8, stream, g_merr)))
    return rc;
  size_t scan_bytes = 0;
  if ((rc = gs.scratch_bytes(&scan_bytes)) || (rc = tmp.alloc(scan_bytes, stream, g_merr))) return rc;
  static const bool timing = scfq_scratch::env_switch("SCFQ_MERGE_TIMING");
  scfq_scratch::StageClock clk(stream, timing);
  SCFQ_SCRATCH_CHK(g_merr, hipMemsetAsync(acc.p, 0, scfq_overlap::kAccWords * 8, stream));
  SCFQ_SCRATCH_CHK(g_merr, hipMemsetAsync(counters.p, 0, kCounters * 8, stream));
  if ((rc = gs.zero())) return rc;
  clk.mark(0);
  if ((rc = scfq_overlap::queue_overlap(d1, n1, d2, n2, interleaved, ix, prm.ov, recs.as<scfq_overlap_rec>(), acc.as<unsigned long long>(), stream, g_merr))) return rc;
  clk.mark(1);
  const RecInput a = {d1, n1, ix.off1.as<uint64_t>(), ix.lines1, ix.cr1};
  const RecInput b = interleaved ? a : RecInput{d2, n2, ix.off2.as<uint64_t>(), ix.lines2, ix.cr2};
  const uint64_t stride = interleaved ? 2 : 1, second = interleaved ? 1 : 0;
  hipLaunchKernelGGL(mg_lengths, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, stream, a, b, stride, second, pairs, recs.as<scfq_overlap_rec>(), n_groups,
                     gs.len(), counters.as<unsigned long long>());
  SCFQ_SCRATCH_CHK(g_merr, hipGetLastError());
  if ((rc = gs.scan(tmp.p, scan_bytes))) return rc;
  clk.mark(2);
  // the sizes come back first: pool memory for the outputs is taken to fit, and a caller's buffer that is too small is known here
  if ((rc = gs.read_totals())) return rc;
  SCFQ_SCRATCH_CHK(g_merr, hipStreamSynchronize(stream));
  st->merged_bytes = gs.total[0]; st->unmerged1_bytes = gs.total[1]; st->unmerged2_bytes = gs.total[2];
  const scfq_reads::Placement put = scfq_reads::place_outputs(gs, kDestName, dst, own_outputs, check_caps, false, own, stream, g_merr);
  if (put.rc) return put.rc;
  hipLaunchKernelGGL(mg_write, dim3((unsigned)((n_groups + kMgWaves - 1) / kMgWaves)), dim3(64 * kMgWaves), 0, stream, a, b, stride, second, pairs,
                     recs.as<scfq_overlap_rec>(), n_groups, gs.off(), put.out[0], put.out[1], put.out[2], prm.q0, counters.as<unsigned long long>());
  SCFQ_SCRATCH_CHK(g_merr, hipGetLastError());
  clk.mark(3);
  uint64_t h[kCounters];
  SCFQ_SCRATCH_CHK(g_merr, hipMemcpyAsync(h, counters.p, kCounters * 8, hipMemcpyDeviceToHost, stream));
  SCFQ_SCRATCH_CHK(g_merr, hipStreamSynchronize(stream));
  st->merged = h[kMerged]; st->not_overlapped = h[kNotOverlapped]; st->too_long = h[kTooLong];
  st->merged_bases = h[kMergedBases]; st->overlap_bases = h[kOverlapBases]; st->mismatches = h[kMismatches];
  st->took_mate1 = h[kTook1]; st->took_mate2 = h[kTook2]; st->neither_valid = h[kNeither];
  g_stage_ms[1] = clk.between(0, 1);
  g_stage_ms[2] = clk.between(1, 2);
  g_stage_ms[3] = clk.between(2, 3);
  return put.verdict;      // (SCFQ_EARG for an output that is too small: place_outputs has left the text)
}

}  // namespace

extern "C" {

const char* scfq_merge_error_detail(void) { return g_merr; }

int scfq_debug_merge_stages(double* ms, uint32_t cap) { return scfq_scratch::copy_stage_ms(g_stage_ms, ms, cap); }

int scfq_merge_buffers(const void* r1, uint64_t n1, const void* r2, uint64_t n2, int is_device, const scfq_merge_opts* opts, void* merged, uint64_t merged_cap,
                       void* un1, uint64_t un1_cap, void* un2, uint64_t un2_cap, int out_is_device, scfq_merge_stats* stats) {
  g_merr[0] = '\0';
  Params prm;
  if (!args_ok(opts, stats, prm) || (!r1 && n1) || (!r2 && n2) || (!merged && merged_cap) || (!un1 && un1_cap) || (!un2 && un2_cap)) return SCFQ_EARG;
  const bool interleaved = (prm.ov.flags & SCFQ_MERGE_INTERLEAVED) != 0;
  if (interleaved && (r2 || n2)) { std::snprintf(g_merr, sizeof g_merr, "interleaved input takes no second buffer"); return SCFQ_EARG; }
  if (interleaved && un2) { std::snprintf(g_merr, sizeof g_merr, "interleaved input has no second unmerged output (unmerged2)"); return SCFQ_EARG; }
  scfq_scratch::clear_keep_size(stats);
  Dest dst[3] = {{static_cast<uint8_t*>(merged), merged_cap, merged != nullptr}, {static_cast<uint8_t*>(un1), un1_cap, un1 != nullptr},
                 {static_cast<uint8_t*>(un2), un2_cap, un2 != nullptr}};
  const bool any_out = merged || un1 || un2, direct = any_out && out_is_device;
  scfq_scratch::ResidentInput in1, in2;
  int rc = in1.from_buffer(r1, n1, is_device != 0, is_device || direct, g_merr);
  if (rc) return rc;
  // (a host buffer's copy is waited for inside; device memory of the caller is ordered before in1's stream above)
  if (!interleaved && (rc = in2.from_buffer(r2, n2, is_device != 0, false, g_merr))) return rc;
  DevBuf own[3];
  rc = merge_device(in1.d_in, in1.n, in2.d_in, in2.n, interleaved, prm, /*own_outputs=*/!direct, dst, own, /*check_caps=*/true, stats, in1.stream);
  if (rc) return finish(in1, rc);
  if (!direct) {
    const uint64_t bytes[3] = {stats->merged_bytes, stats->unmerged1_bytes, stats->unmerged2_bytes};
    if ((rc = scfq_reads::outputs_to_host(3, dst, own, bytes, in1.stream, g_merr))) return rc;
    SCFQ_SCRATCH_CHK(g_merr, hipStreamSynchronize(in1.stream));
  }
  for (DevBuf& o : own) o.drop();
  in1.mark_clean();      // (the last act was to wait for the stream; behind it lie returns of pool memory only)
  return SCFQ_OK;
}

int scfq_merge_files(const char* path1, const char* path2, const scfq_opts* opts, const scfq_merge_opts* mopts, int merged_fd, int un1_fd, int un2_fd,
                     scfq_merge_stats* stats) {
  g_merr[0] = '\0';
  Params prm;
  if (!path1 || !args_ok(mopts, stats, prm)) return SCFQ_EARG;
  const bool interleaved = path2 == nullptr;
  if ((prm.ov.flags & SCFQ_MERGE_INTERLEAVED) && path2) { std::snprintf(g_merr, sizeof g_merr, "interleaved input takes no second file"); return SCFQ_EARG; }
  if (interleaved && un2_fd >= 0) { std::snprintf(g_merr, sizeof g_merr, "interleaved input has no second unmerged output (unmerged2)"); return SCFQ_EARG; }
  scfq_scratch::clear_keep_size(stats);
  scfq_scratch::ResidentInput in1, in2;
  int rc = in1.from_file(path1, opts, g_merr);
  if (rc) return rc;
  if (!interleaved && (rc = in2.from_file(path2, opts, g_merr))) return rc;      // (staged when this returns)
  const int fd[3] = {merged_fd, un1_fd, un2_fd};
  Dest dst[3] = {{nullptr, 0, merged_fd >= 0}, {nullptr, 0, un1_fd >= 0}, {nullptr, 0, un2_fd >= 0}};
  DevBuf own[3];
  rc = merge_device(in1.d_in, in1.n, in2.d_in, in2.n, interleaved, prm, /*own_outputs=*/true, dst, own, /*check_caps=*/false, stats, in1.stream);
  if (rc) return finish(in1, rc);
  const uint64_t bytes[3] = {stats->merged_bytes, stats->unmerged1_bytes, stats->unmerged2_bytes};
  return scfq_reads::outputs_to_fds(3, own, bytes, fd, in1, g_merr);
}

}  // extern "C"

// scfq_insert.hip — `sc fq-insert-size` on the MI355X (gfx950): insert sizes from the overlap of the two mates of a read pair.
// Not in the reference (its insert-size command reads an aligned BAM); definitions in include/sc_fqcount.h.
//
// Both inputs sit in HBM whole (or the one interleaved input):
//   K5  line index            (scfq_scratch::build_line_index) of each input
//   P1  is_overlap            the hot path: a wave per pair, kIsWaves waves per block, the blocks stride over the pairs.  The lanes load
//                             mate 1 front to back and mate 2 back to front, a byte each, and turn a byte into a 2-bit code (bits 1 and 2
//                             of the letter: A 0, C 1, T 2, G 3, so the complement is code ^ 2) and a valid bit (the byte IS that letter).
//                             Three ballots pack 64 bases into three bit planes; a read of 512 bases is 8 words per plane.  The planes
//                             of A go to LDS between zero words, those of C = revcomp(B) next to them.  Lane l then takes the offsets
//                             d0 + l, d0 + l + 64, ...: it reads A's planes shifted by d (two words and a funnel shift per word) and
//                             counts the positions where both are valid and the codes agree.  Outside either read the valid bits are
//                             0, so no overlap mask is needed: mm = ov - agreeing positions.  Only offsets with ov >= min_overlap are
//                             looked at, and an offset is left as soon as the words still to come cannot bring the agreeing positions
//                             it needs any more (exact: such an offset is never accepted): of 64 offsets at most a few are near the
//                             truth, so most rounds end after one word (measured: 11 % of P1 at 2 x 250, nothing at 2 x 150).  The wave picks d* with ONE minimum of a packed 64-bit key (1023 - ov, mm, 1024 - d); lane 0
//                             writes the record and adds 1 to the block's 32-bit LDS bin of the insert; the sums stay in lane 0's
//                             registers.  A block adds its non-zero bins and its sums to the 64-bit global counters once.
//   P2  is_finish             one block over the 1024 bins: min, max, mode, median
// Everything is integer / bit work; there is no CPU fallback.
#include "../../include/sc_fqcount.h"
#include "../../include/sc_fqcount_debug.h"

#include <hip/hip_runtime.h>

#include "scfq_overlap.hpp"
#include "scfq_reads_device.hpp"
#include "scfq_scratch.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>

namespace {

thread_local char g_ierr[scfq_scratch::kErrBytes] = "";
thread_local double g_stage_ms[4] = {0, 0, 0, 0};

using scfq_scratch::DevBuf;

constexpr uint32_t kIsWaves = 4;                         // pairs a block works on at a time
constexpr uint32_t kIsThreads = 64 * kIsWaves;
constexpr uint32_t kIsWords = SCFQ_INSERT_MAX_LEN / 64;  // words of a plane
constexpr uint32_t kIsSlots = 3 * kIsWords;              // A's plane in LDS: kIsWords zero words, the plane, kIsWords zero words
constexpr uint32_t kIsMaxBlocks = 4096;
static_assert(SCFQ_INSERT_MAX_LEN % 64 == 0 && 2 * SCFQ_INSERT_MAX_LEN <= SCFQ_INSERT_HIST_BINS, "an insert is below La + Lb");
// the counters behind the bins
enum { kOverlapped = 0, kNotOverlapped, kTooLong, kReadThrough, kOverlapBases, kMismatches, kInsertSum, kInsertSqSum, kMin, kMax, kMode, kMedian, kSums };
constexpr uint32_t kIsAcc = SCFQ_INSERT_HIST_BINS + kSums;

// the text of the sequence line of record r (a line the input does not have is empty)
__device__ __forceinline__ void seq_span(const RecInput& in, uint64_t r, uint64_t& s, uint64_t& e) {
  text_span(in, 4 * r + 1, s, e);
}

// code (bit 0, bit 1) and valid bit of a byte: bits 1 and 2 of 'A' 'C' 'T' 'G' are 0 1 2 3
__device__ __forceinline__ void classify(uint32_t b, bool& c0, bool& c1, bool& v) {
  const uint32_t h = (b >> 1) & 3u;
  v = ((0x47544341u >> (8 * h)) & 0xffu) == b;
  c0 = (h & 1u) != 0;
  c1 = (h & 2u) != 0;
}

// P1.  a, b: the inputs of mate 1 and mate 2 (the same one twice for interleaved input); pair p is record p * stride of a and
// record p * stride + second of b
__global__ __launch_bounds__(kIsThreads) void is_overlap(RecInput a, RecInput b, uint64_t stride, uint64_t second, uint64_t pairs, uint32_t min_overlap,
                                                        uint32_t max_mm, uint32_t max_pct, scfq_overlap_rec* recs, unsigned long long* acc) {
  __shared__ uint32_t bins[SCFQ_INSERT_HIST_BINS];
  __shared__ uint64_t pa[kIsWaves][3][kIsSlots];
  __shared__ uint64_t pc[kIsWaves][3][kIsWords];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint32_t k = threadIdx.x; k < SCFQ_INSERT_HIST_BINS; k += kIsThreads) bins[k] = 0;
  uint64_t sums[8] = {0, 0, 0, 0, 0, 0, 0, 0};          // (lane 0's count)
  // every wave of the block makes the same number of rounds: the barrier inside is reached by all of them
  for (uint64_t p0 = (uint64_t)blockIdx.x * kIsWaves; p0 < pairs; p0 += (uint64_t)gridDim.x * kIsWaves) {
    const uint64_t p = p0 + wave;
    const bool have = p < pairs;
    uint64_t sa = 0, ea = 0, sb = 0, eb = 0;
    if (have) {
      seq_span(a, p * stride, sa, ea);
      seq_span(b, p * stride + second, sb, eb);
    }
    const uint64_t la64 = ea - sa, lb64 = eb - sb;
    const bool too_long = la64 > SCFQ_INSERT_MAX_LEN || lb64 > SCFQ_INSERT_MAX_LEN;
    const int la = too_long ? 0 : (int)la64, lb = too_long ? 0 : (int)lb64;      // (a pair that is not looked at has no bytes)
    // the planes: word w of a plane is with lane w
    uint64_t ra[3] = {0, 0, 0}, rc[3] = {0, 0, 0};
#pragma unroll
    for (uint32_t w = 0; w < kIsWords; ++w) {
      const int y = (int)(64 * w + lane);
      if (64 * (int)w < la) {
        bool c0, c1, v;
        classify(y < la ? a.base[sa + (uint64_t)y] : 0u, c0, c1, v);
        const uint64_t b0 = __builtin_amdgcn_ballot_w64(c0), b1 = __builtin_amdgcn_ballot_w64(c1), bv = __builtin_amdgcn_ballot_w64(v);
        if (lane == w) { ra[0] = b0; ra[1] = b1; ra[2] = bv; }
      }
      if (64 * (int)w < lb) {
        bool c0, c1, v;
        classify(y < lb ? b.base[sb + (uint64_t)(lb - 1 - y)] : 0u, c0, c1, v);
        const uint64_t b0 = __builtin_amdgcn_ballot_w64(c0), b1 = __builtin_amdgcn_ballot_w64(!c1), bv = __builtin_amdgcn_ballot_w64(v);
        if (lane == w) { rc[0] = b0; rc[1] = b1; rc[2] = bv; }      // (the complement: code ^ 2; where v is 0 the code is never looked at)
      }
    }
    if (lane < kIsSlots) {
      // lanes 0 .. 7 hold the words and write the middle, lanes 8 .. 23 write the zero words below and above (their r is 0)
      const uint32_t slot = lane < kIsWords ? lane + kIsWords : (lane < 2 * kIsWords ? lane - kIsWords : lane);
#pragma unroll
      for (uint32_t k = 0; k < 3; ++k) pa[wave][k][slot] = ra[k];
      if (lane < kIsWords) {
#pragma unroll
        for (uint32_t k = 0; k < 3; ++k) pc[wave][k][lane] = rc[k];
      }
    }
    __syncthreads();
    // offsets with ov >= min_overlap: d in [min_overlap - lb, la - min_overlap], none when a read is shorter than that
    uint64_t best = ~0ull;
    const int mo = (int)min_overlap;
    if (la >= mo && lb >= mo) {
      const int d1 = la - mo, nwc = (lb + 63) >> 6;
      for (int d = mo - lb + (int)lane; d <= d1; d += 64) {
        const int q = d >> 6, r = d & 63;                  // (floor: d = 64 q + r); bit y of A shifted = bit y + d of A
        const uint64_t* w0 = &pa[wave][0][(int)kIsWords + q];
        const uint64_t* w1 = &pa[wave][1][(int)kIsWords + q];
        const uint64_t* wv = &pa[wave][2][(int)kIsWords + q];
        uint64_t l0 = w0[0], l1 = w1[0], lv = wv[0];
        const int lo = std::max(0, -d), hi = std::min(lb, la - d), ov = hi - lo;      // (ov >= mo: d is inside the range above)
        // agreeing positions the offset needs to be accepted; a word is only looked at while the words still to come can supply them
        // (what is left of the overlap behind word k is an upper bound of what they add), so most offsets end after their first word
        const int need = ov - (int)std::min<uint32_t>(max_mm, max_pct * (uint32_t)ov / 100u);
        int agree = 0;
        for (int k = 0; k < nwc && agree + std::max(0, hi - std::max(lo, 64 * k)) >= need; ++k) {
          const uint64_t h0 = w0[k + 1], h1 = w1[k + 1], hv = wv[k + 1];
          const uint64_t a0 = r ? (l0 >> r) | (h0 << (64 - r)) : l0;
          const uint64_t a1 = r ? (l1 >> r) | (h1 << (64 - r)) : l1;
          const uint64_t av = r ? (lv >> r) | (hv << (64 - r)) : lv;
          agree += __popcll(av & pc[wave][2][k] & ~((a0 ^ pc[wave][0][k]) | (a1 ^ pc[wave][1][k])));
          l0 = h0; l1 = h1; lv = hv;
        }
        const uint32_t mm = (uint32_t)(ov - agree);
        if (agree >= need) {                                  // mm <= max_mm and 100 mm <= max_pct ov
          const uint64_t key = ((uint64_t)(1023 - ov) << 48) | ((uint64_t)mm << 32) | (uint32_t)(1024 - d);
          best = key < best ? key : best;
        }
      }
    }
    best = wave_min(best);
    if (have && lane == 0) {
      scfq_overlap_rec rec;
      rec.offset = 0; rec.overlap = 0; rec.mismatches = 0;
      if (too_long) {
        rec.mismatches = 0xFFFFu;
        ++sums[kTooLong];
      } else if (best == ~0ull) {
        ++sums[kNotOverlapped];
      } else {
        const int ov = 1023 - (int)(best >> 48), d = 1024 - (int)(uint32_t)best;
        const uint32_t mm = (uint32_t)(best >> 32) & 0xFFFFu;
        const uint64_t ins = (uint64_t)(d + lb);
        rec.offset = d; rec.overlap = (uint16_t)ov; rec.mismatches = (uint16_t)mm;
        ++sums[kOverlapped];
        sums[kReadThrough] += ins < (uint64_t)std::max(la, lb);
        sums[kOverlapBases] += (uint64_t)ov;
        sums[kMismatches] += mm;
        sums[kInsertSum] += ins;
        sums[kInsertSqSum] += ins * ins;
        atomicAdd(&bins[ins], 1u);                          // (1 <= ins <= la + lb - 1 < 1024)
      }
      if (recs) recs[p] = rec;
    }
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < SCFQ_INSERT_HIST_BINS; k += kIsThreads)
    if (bins[k]) atomicAdd(&acc[k], (unsigned long long)bins[k]);
  if (lane == 0) {
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k)
      if (sums[k]) atomicAdd(&acc[SCFQ_INSERT_HIST_BINS + k], (unsigned long long)sums[k]);
  }
}

// P2: a thread per bin.  cum: the inclusive prefix sums of the bins
__global__ __launch_bounds__(SCFQ_INSERT_HIST_BINS) void is_finish(unsigned long long* acc) {
  __shared__ uint64_t cum[2][SCFQ_INSERT_HIST_BINS];
  __shared__ unsigned long long mode;
  const uint32_t s = threadIdx.x;
  const uint64_t c = acc[s];
  cum[0][s] = c;
  if (s == 0) mode = 0;
  __syncthreads();
  uint32_t cur = 0;
  for (uint32_t step = 1; step < SCFQ_INSERT_HIST_BINS; step <<= 1) {
    cum[cur ^ 1][s] = cum[cur][s] + (s >= step ? cum[cur][s - step] : 0);
    cur ^= 1;
    __syncthreads();
  }
  const uint64_t total = cum[cur][SCFQ_INSERT_HIST_BINS - 1], mine = cum[cur][s], before = mine - c;
  // the largest count, the smallest bin among equals (a count is below 2^31)
  if (c) atomicMax(&mode, ((unsigned long long)c << 10) | (SCFQ_INSERT_HIST_BINS - 1 - s));
  __syncthreads();
  unsigned long long* out = acc + SCFQ_INSERT_HIST_BINS;
  if (c && before == 0) out[kMin] = s;
  if (c && mine == total) out[kMax] = s;
  if (total && 2 * mine >= total && 2 * before < total) out[kMedian] = s;
  if (s == 0) out[kMode] = mode ? SCFQ_INSERT_HIST_BINS - 1 - (mode & (SCFQ_INSERT_HIST_BINS - 1)) : 0;
}

using scfq_overlap::Params;

bool args_ok(const scfq_insert_opts* opts, const scfq_overlap_rec* recs, uint64_t rec_cap, const scfq_insert_summary* out, Params& p) {
  if (!out || out->struct_size != sizeof(scfq_insert_summary) || (!recs && rec_cap)) return false;
  p.flags = 0; p.min_overlap = 30; p.max_mm = 5; p.max_pct = 20;
  if (!opts) return true;
  if (opts->struct_size != sizeof(scfq_insert_opts)) return false;
  p.flags = opts->flags; p.min_overlap = opts->min_overlap; p.max_mm = opts->max_mismatches; p.max_pct = opts->max_mismatch_pct;
  if (p.flags & ~(uint32_t)SCFQ_INSERT_INTERLEAVED) { std::snprintf(g_ierr, sizeof g_ierr, "unknown flag bits 0x%x", p.flags & ~(uint32_t)SCFQ_INSERT_INTERLEAVED); return false; }
  return scfq_overlap::params_in_range(p, g_ierr);
}

// in1, in2: the inputs, resident (in2 = nullptr: in1 is interleaved); everything runs on `stream`
int insert_device(const uint8_t* d1, uint64_t n1, const uint8_t* d2, uint64_t n2, bool interleaved, const Params& prm, scfq_overlap_rec* recs,
                  uint64_t rec_cap, uint64_t* hist_host, scfq_insert_summary* out, hipStream_t stream) {
  for (double& m : g_stage_ms) m = 0;
  out->input_bytes1 = n1;
  out->input_bytes2 = n2;
  out->min_overlap = prm.min_overlap;
  out->max_mismatches = prm.max_mm;
  out->max_mismatch_pct = prm.max_pct;
  scfq_overlap::Indexed ix;
  DevBuf acc;
  int rc = scfq_overlap::index_inputs(d1, n1, d2, n2, interleaved, stream, g_ierr, ix, &g_stage_ms[0]);
  out->lines1 = ix.lines1; out->lines2 = ix.lines2;
  out->reads1 = ix.reads1; out->reads2 = ix.reads2;
  if (rc) return rc;
  const uint64_t pairs = ix.pairs;
  out->pairs = pairs;
  out->unpaired = ix.unpaired;
  if (recs && rec_cap < pairs) { std::snprintf(g_ierr, sizeof g_ierr, "the record table holds %llu pairs, the input has %llu", (unsigned long long)rec_cap, (unsigned long long)pairs); return SCFQ_EARG; }
  if (hist_host) std::memset(hist_host, 0, SCFQ_INSERT_HIST_BINS * sizeof(uint64_t));
  if (pairs == 0) return SCFQ_OK;
  if ((rc = acc.alloc(kIsAcc * 8, stream, g_ierr))) return rc;
  static const bool timing = scfq_scratch::env_switch("SCFQ_INSERT_TIMING");
  scfq_scratch::StageClock clk(stream, timing);
  SCFQ_SCRATCH_CHK(g_ierr, hipMemsetAsync(acc.p, 0, kIsAcc * 8, stream));
  clk.mark(0);
  if ((rc = scfq_overlap::queue_overlap(d1, n1, d2, n2, interleaved, ix, prm, recs, acc.as<unsigned long long>(), stream, g_ierr))) return rc;
  clk.mark(1);
  hipLaunchKernelGGL(is_finish, dim3(1), dim3(SCFQ_INSERT_HIST_BINS), 0, stream, acc.as<unsigned long long>());
  SCFQ_SCRATCH_CHK(g_ierr, hipGetLastError());
  clk.mark(2);
  static thread_local uint64_t h[kIsAcc];
  SCFQ_SCRATCH_CHK(g_ierr, hipMemcpyAsync(h, acc.p, kIsAcc * 8, hipMemcpyDeviceToHost, stream));
  clk.mark(3);
  SCFQ_SCRATCH_CHK(g_ierr, hipStreamSynchronize(stream));
  if (hist_host) std::memcpy(hist_host, h, SCFQ_INSERT_HIST_BINS * sizeof(uint64_t));
  const uint64_t* s = h + SCFQ_INSERT_HIST_BINS;
  out->overlapped = s[kOverlapped]; out->not_overlapped = s[kNotOverlapped]; out->too_long = s[kTooLong];
  out->read_through = s[kReadThrough]; out->overlap_bases = s[kOverlapBases]; out->mismatches = s[kMismatches];
  out->insert_sum = s[kInsertSum]; out->insert_sq_sum = s[kInsertSqSum];
  out->min_insert = s[kMin]; out->max_insert = s[kMax]; out->mode_insert = s[kMode]; out->median_insert = s[kMedian];
  g_stage_ms[1] = clk.between(0, 1);
  g_stage_ms[2] = clk.between(1, 2);
  g_stage_ms[3] = clk.between(2, 3);
  return SCFQ_OK;
}

// the call on two resident inputs (in2 unused for interleaved input).  After a failure kernels that read the second input may
// still be queued on the first one's stream: they are waited for before the second input's memory goes back
int run(scfq_scratch::ResidentInput& in1, scfq_scratch::ResidentInput& in2, bool interleaved, const Params& prm, scfq_overlap_rec* recs, uint64_t rec_cap,
        uint64_t* hist_host, scfq_insert_summary* out) {
  const int rc = insert_device(in1.d_in, in1.n, in2.d_in, in2.n, interleaved, prm, recs, rec_cap, hist_host, out, in1.stream);
  if (rc == SCFQ_OK) in1.mark_clean();      // (its last act was to wait for the stream)
  else (void)hipStreamSynchronize(in1.stream);
  return rc;
}

}  // namespace

// ---- scfq_overlap.hpp: the part fq-merge runs as well ----
namespace scfq_overlap {

static_assert(kAccWords == kIsAcc, "scfq_overlap.hpp sizes P1's counters");

bool params_in_range(const Params& p, char* errbuf) {
  const size_t cap = scfq_scratch::kErrBytes;
  if (p.min_overlap < 1 || p.min_overlap > SCFQ_INSERT_MAX_LEN) { std::snprintf(errbuf, cap, "min_overlap %u is not in 1 .. %d", p.min_overlap, SCFQ_INSERT_MAX_LEN); return false; }
  if (p.max_mm > 65535) { std::snprintf(errbuf, cap, "max_mismatches %u is not in 0 .. 65535", p.max_mm); return false; }
  if (p.max_pct > 100) { std::snprintf(errbuf, cap, "max_mismatch_pct %u is not in 0 .. 100", p.max_pct); return false; }
  return true;
}

int index_inputs(const uint8_t* d1, uint64_t n1, const uint8_t* d2, uint64_t n2, bool interleaved, hipStream_t stream, char* errbuf, Indexed& ix,
                 double* index_ms) {
  int rc = SCFQ_OK;
  const auto t_a = std::chrono::steady_clock::now();
  if ((rc = scfq_scratch::build_line_index(d1, n1, stream, errbuf, ix.off1, &ix.lines1, &ix.cr1))) return rc;
  if (!interleaved && (rc = scfq_scratch::build_line_index(d2, n2, stream, errbuf, ix.off2, &ix.lines2, &ix.cr2))) return rc;
  *index_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_a).count();
  ix.reads1 = (ix.lines1 + 3) / 4;
  ix.reads2 = (ix.lines2 + 3) / 4;
  if (ix.reads1 >= (1ull << 31) || ix.reads2 >= (1ull << 31)) { std::snprintf(errbuf, scfq_scratch::kErrBytes, "more than 2^31 records in one input"); return SCFQ_EARG; }
  ix.pairs = interleaved ? ix.reads1 / 2 : std::min(ix.reads1, ix.reads2);
  ix.unpaired = interleaved ? (ix.reads1 & 1) : std::max(ix.reads1, ix.reads2) - ix.pairs;
  return SCFQ_OK;
}

int queue_overlap(const uint8_t* d1, uint64_t n1, const uint8_t* d2, uint64_t n2, bool interleaved, const Indexed& ix, const Params& prm,
                  scfq_overlap_rec* recs, unsigned long long* acc, hipStream_t stream, char* errbuf) {
  const RecInput a = {d1, n1, static_cast<const uint64_t*>(ix.off1.p), ix.lines1, ix.cr1};
  const RecInput b = interleaved ? a : RecInput{d2, n2, static_cast<const uint64_t*>(ix.off2.p), ix.lines2, ix.cr2};
  const unsigned blocks = (unsigned)std::min<uint64_t>((ix.pairs + kIsWaves - 1) / kIsWaves, kIsMaxBlocks);
  hipLaunchKernelGGL(is_overlap, dim3(blocks), dim3(kIsThreads), 0, stream, a, b, interleaved ? 2ull : 1ull, interleaved ? 1ull : 0ull, ix.pairs,
                     prm.min_overlap, prm.max_mm, prm.max_pct, recs, acc);
  SCFQ_SCRATCH_CHK(errbuf, hipGetLastError());
  return SCFQ_OK;
}

}  // namespace scfq_overlap

extern "C" {

const char* scfq_insert_size_error_detail(void) { return g_ierr; }

int scfq_debug_insert_size_stages(double* ms, uint32_t cap) { return scfq_scratch::copy_stage_ms(g_stage_ms, ms, cap); }

int scfq_insert_size_buffers(const void* r1, uint64_t n1, const void* r2, uint64_t n2, int is_device, const scfq_insert_opts* opts,
                             scfq_overlap_rec* recs_device, uint64_t rec_cap, uint64_t* hist_host, scfq_insert_summary* out) {
  g_ierr[0] = '\0';
  Params prm;
  if (!args_ok(opts, recs_device, rec_cap, out, prm) || (!r1 && n1) || (!r2 && n2)) return SCFQ_EARG;
  const bool interleaved = (prm.flags & SCFQ_INSERT_INTERLEAVED) != 0;
  if (interleaved && (r2 || n2)) { std::snprintf(g_ierr, sizeof g_ierr, "interleaved input takes no second buffer"); return SCFQ_EARG; }
  scfq_scratch::clear_keep_size(out);
  scfq_scratch::ResidentInput in1, in2;
  int rc = in1.from_buffer(r1, n1, is_device != 0, is_device || recs_device, g_ierr);
  if (rc) return rc;
  // (a host buffer's copy is waited for inside; device memory of the caller is ordered before in1's stream above)
  if (!interleaved && (rc = in2.from_buffer(r2, n2, is_device != 0, false, g_ierr))) return rc;
  return run(in1, in2, interleaved, prm, recs_device, rec_cap, hist_host, out);
}

int scfq_insert_size_files(const char* path1, const char* path2, const scfq_opts* opts, const scfq_insert_opts* iopts, scfq_overlap_rec* recs_device,
                           uint64_t rec_cap, uint64_t* hist_host, scfq_insert_summary* out) {
  g_ierr[0] = '\0';
  Params prm;
  if (!path1 || !args_ok(iopts, recs_device, rec_cap, out, prm)) return SCFQ_EARG;
  const bool interleaved = path2 == nullptr;
  if ((prm.flags & SCFQ_INSERT_INTERLEAVED) && path2) { std::snprintf(g_ierr, sizeof g_ierr, "interleaved input takes no second file"); return SCFQ_EARG; }
  scfq_scratch::clear_keep_size(out);
  scfq_scratch::ResidentInput in1, in2;
  int rc = in1.from_file(path1, opts, g_ierr);
  if (rc) return rc;
  if (recs_device && (rc = scfq_scratch::order_after_caller(in1.stream, g_ierr))) return rc;
  if (!interleaved && (rc = in2.from_file(path2, opts, g_ierr))) return rc;      // (staged when this returns)
  return run(in1, in2, interleaved, prm, recs_device, rec_cap, hist_host, out);
}

}  // extern "C"

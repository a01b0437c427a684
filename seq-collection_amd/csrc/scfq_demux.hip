// scfq_demux.hip — `sc fq-demux` on the MI355X (gfx950): the reads of a pooled run split by sample barcode, every sample's records
// one behind the other in one buffer per mate.  Not in the reference; definitions in include/sc_fqcount.h.
//
// A call, the inputs in HBM whole (one FASTQ, two, or one interleaved):
//   X0  the sheet               host (scfq_demux_host.hpp): names and barcodes checked, a barcode as a 64-bit word of 2-bit codes
//   K5  line index              (scfq_scratch::build_line_index) of each input
//   X1  dx_assign               a lane per unit: the candidates' first 32 bytes as a word of 2-bit codes and a word that marks the
//                               bytes that are not A C G T, then all N samples one after the other, without an early exit: XOR, fold
//                               of the bit pairs, the marks ORed in, the mask of the barcode's length, population count.  The
//                               sample index is the same in every lane, so the sheet's words are read by scalar loads and cost
//                               no vector instruction and no LDS.  8 bytes, a 16-bit sort key (N: undetermined) and the unit's
//                               number per unit; the five kinds counted per block
//       radix sort              (key, unit) pairs over the key's ceil(log2(N + 1)) bits, rocprim::radix_sort_pairs: stable, so every
//                               destination keeps its input order
//   X2  dx_lengths              a thread per sorted position: the bytes its unit adds to each output, summed per group of kDxGroup,
//                               and the rows — summed over the wave first where the wave has one destination, which is the rule
//       exclusive scans         one per output over the groups (rocprim), each with a last entry that is the output's size
//   X3  dx_write                the hot path: a wave per group of sorted positions, kDxWaves per block.  The records lie wherever
//                               the input has them and go out one behind the other: a record whose output is its own bytes is one
//                               wave_copy, a clipped one three (what lies in front of, between and behind the two clips), one that
//                               needs '\n' put right its four pieces
// Guards: a unit number read from the sorted array is compared with `units` before it is used, a sample number read from the
// per-unit table with N; every loop runs over a line's span, a barcode's 32 bytes or the N samples; nothing waits for another
// wave.  X3 compares the scanned totals with the capacities before it stores anything.  No CPU fallback.
#include "../../include/sc_fqcount.h"
#include "../../include/sc_fqcount_debug.h"

#include <cstring>        // (rocprim's texture iterator calls memset from host code)
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "scfq_demux_host.hpp"
#include "scfq_reads_host.hpp"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <string>
#include <vector>

static_assert(sizeof(scfq_demux_rec) == 8 && sizeof(scfq_demux_row) == 64 && sizeof(scfq_demux_stats) == 29 * 8 && sizeof(scfq_demux_opts) == 24, "the ABI's sizes");
static_assert(scfq_demux_host::kErrBytes == scfq_scratch::kErrBytes, "one error buffer for both");
static_assert(SCFQ_DEMUX_MAX_SAMPLES < 0xFFFF && SCFQ_DEMUX_MAX_BARCODE == 32, "a 16-bit key; a barcode is one 64-bit word");

struct scfq_demux_sheet { scfq_demux_host::Sheet sh; };

namespace {

thread_local char g_xerr[scfq_scratch::kErrBytes] = "";
thread_local double g_stage_ms[4] = {0, 0, 0, 0};

using scfq_reads::Dest;
using scfq_reads::DevBuf;
using scfq_reads::finish;
using scfq_reads::Mode;

constexpr uint32_t kDxGroup = kRecGroup;                 // sorted positions of a group: one wave of X3, one entry of the scans
constexpr uint32_t kDxWaves = 4;                         // groups of a block of X3
constexpr uint64_t kPairMask = 0x5555555555555555ull;

struct DxSheet {          // the sheet on the device
  const uint64_t* codes;  // 2 words per sample
  const uint32_t* lens;   // m1 | m2 << 8
  uint32_t n;
};

// the first min(32, e - s) bytes of [s, e): byte i's code at bits 2i and 2i + 1 of `code`, bit 2i of `bad` set iff the byte is not
// exactly A, C, G or T (the plane of such bytes, spread to where the folded XOR has its bits)
__device__ __forceinline__ void pack_byte(uint32_t b, uint32_t i, uint64_t& code, uint64_t& bad) {
  const bool valid = b == 'A' || b == 'C' || b == 'G' || b == 'T';
  code |= (uint64_t)((b >> 1) & 3u) << (2 * i);
  bad |= (uint64_t)(valid ? 0u : 1u) << (2 * i);
}
__device__ __forceinline__ void pack_candidate(const uint8_t* base, uint64_t s, uint64_t e, uint64_t& code, uint64_t& bad, uint32_t& len) {
  len = (uint32_t)std::min<uint64_t>(e - s, SCFQ_DEMUX_MAX_BARCODE);
  code = bad = 0;
  uint32_t i = 0;
  for (; i + 8 <= len; i += 8) {                         // eight bytes by one load, all of them inside [s, s + len)
    uint64_t w;
    __builtin_memcpy(&w, base + s + i, 8);               // (arbitrarily aligned)
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) pack_byte((uint32_t)(w >> (8 * k)) & 0xFFu, i + k, code, bad);
  }
  for (; i < len; ++i) pack_byte(base[s + i], i, code, bad);
}

// mismatches of the candidate against a barcode of m letters (mask: the low 2m bits)
__device__ __forceinline__ uint32_t mismatches(uint64_t code, uint64_t bad, uint64_t barcode, uint64_t mask) {
  const uint64_t x = code ^ barcode;
  return (uint32_t)__builtin_popcountll((((x | (x >> 1)) & kPairMask) | bad) & mask);
}

// the counters of X1
enum { kPerfect = 0, kMismatched, kUnmatched, kAmbiguous, kNoBarcode, kKinds };

// X1.  Unit u is record u of `a` (single-end: paired = 0) or the pair of record u * stride of a and record u * stride + second of b.
// header = 1: the candidates come from a's header line.  max_mm: M
__global__ __launch_bounds__(256) void dx_assign(RecInput a, RecInput b, uint64_t stride, uint64_t second, uint32_t paired, uint32_t header, uint64_t units,
                                                const uint64_t* __restrict__ codes, const uint32_t* __restrict__ lens, uint32_t n_samples, uint32_t max_mm,
                                                scfq_demux_rec* __restrict__ recs, uint16_t* __restrict__ keys, uint32_t* __restrict__ idx,
                                                unsigned long long* __restrict__ counters) {
  __shared__ uint32_t kind_sh[kKinds];
  if (threadIdx.x < kKinds) kind_sh[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = u < units;
  uint64_t c1 = 0, bad1 = 0, c2 = 0, bad2 = 0;
  uint32_t len1 = 0, len2 = 0;
  if (live) {
    const uint64_t i1 = paired ? u * stride : u;
    uint64_t s, e;
    if (header) {
      text_span(a, 4 * i1, s, e);
      uint64_t p = e;
      while (p > s && a.base[p - 1] != ':') --p;         // behind the last ':', or s without one
      if (p > s) {
        uint64_t q = p;
        while (q < e && a.base[q] != '+') ++q;           // the first '+' of the tail, or e
        pack_candidate(a.base, p, q, c1, bad1, len1);
        if (q < e) pack_candidate(a.base, q + 1, e, c2, bad2, len2);
      }
    } else {
      text_span(a, 4 * i1 + 1, s, e);
      pack_candidate(a.base, s, e, c1, bad1, len1);
      if (paired) {
        text_span(b, 4 * (u * stride + second) + 1, s, e);
        pack_candidate(b.base, s, e, c2, bad2, len2);
      }
    }
  }
  // all samples, always: s is the same in every lane, the sheet's words come by scalar loads.  The best so far is ONE word, smaller is
  // better: t above, 64 - (m1 + m2) below
  uint32_t best = ~0u, best_s = 0, best_mm = 0;
  bool tie = false, any = false;
  for (uint32_t s = 0; s < n_samples; ++s) {
    const uint64_t b1 = codes[2 * s], b2 = codes[2 * s + 1];
    const uint32_t ml = lens[s], m1 = ml & 0xFFu, m2 = ml >> 8;
    const uint64_t k1 = ~0ull >> (64 - 2 * m1), k2 = m2 ? ~0ull >> (64 - 2 * m2) : 0ull;      // (m1 >= 1: never a shift by 64)
    const uint32_t mm1 = mismatches(c1, bad1, b1, k1), mm2 = mismatches(c2, bad2, b2, k2);
    const bool eligible = len1 >= m1 && len2 >= m2;
    const bool match = eligible && mm1 <= max_mm && mm2 <= max_mm;
    const uint32_t w = ((mm1 + mm2) << 8) | (64u - m1 - m2);
    any = any || eligible;
    tie = match ? (w == best ? true : (w < best ? false : tie)) : tie;
    if (match && w < best) { best = w; best_s = s; best_mm = mm1 | (mm2 << 8); }
  }
  const bool matched = best != ~0u;
  const uint32_t state = matched ? (tie ? SCFQ_DEMUX_AMBIGUOUS : SCFQ_DEMUX_ASSIGNED) : (any ? SCFQ_DEMUX_UNMATCHED : SCFQ_DEMUX_NO_BARCODE);
  const bool assigned = state == SCFQ_DEMUX_ASSIGNED;
  if (live) {
    scfq_demux_rec r = {};
    r.sample = assigned ? (uint16_t)best_s : (uint16_t)0xFFFF;
    r.mm1 = assigned ? (uint8_t)(best_mm & 0xFFu) : (uint8_t)0xFF;
    r.mm2 = assigned ? (uint8_t)(best_mm >> 8) : (uint8_t)0xFF;
    r.state = (uint8_t)state;
    recs[u] = r;
    keys[u] = (uint16_t)(assigned ? best_s : n_samples);
    idx[u] = (uint32_t)u;
  }
  // the kinds: a ballot per kind, one LDS add per wave, ONE global atomic per block and kind
  const bool first_lane = (threadIdx.x & 63) == 0;
  const uint32_t kind = !live ? (uint32_t)kKinds : assigned ? ((best >> 8) ? kMismatched : kPerfect) : state == SCFQ_DEMUX_UNMATCHED ? kUnmatched
                                                            : state == SCFQ_DEMUX_AMBIGUOUS ? kAmbiguous : kNoBarcode;
#pragma unroll
  for (uint32_t k = 0; k < kKinds; ++k) {
    const uint32_t c = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(kind == k));
    if (first_lane && c) atomicAdd(&kind_sh[k], c);
  }
  __syncthreads();
  if (threadIdx.x < kKinds && kind_sh[threadIdx.x]) atomicAdd(&counters[threadIdx.x], (unsigned long long)kind_sh[threadIdx.x]);
}

// what a read adds to its output and where its pieces lie.  X2 and X3 both get it from here, so the lengths the scans saw are the
// lengths X3 writes
struct DxRead {
  uint64_t len;                        // bytes of the output record
  uint64_t hs, ss, ps, qs;             // starts of the header, sequence, separator and quality texts as they are written
  uint64_t hl, sl, pl, ql;             // their lengths
  uint32_t kind;                       // kPieces, kWhole or kRuns
};
// kWhole: the record is len bytes from hs on.  kRuns: the record's own bytes but for the clipped bases and qualities, three runs: the
// header and its '\n' from hs, the sequence's rest, '\n', the separator and its '\n' from ss, the quality's rest and its '\n' from qs
enum : uint32_t { kPieces = 0, kWhole, kRuns };

// record i of `in` with the first `clip` bases and qualities left out; seq_len: L
__device__ __forceinline__ DxRead read_of(const RecInput& in, uint64_t i, uint64_t clip, uint64_t& seq_len) {
  DxRead r = {};
  uint64_t e;
  text_span(in, 4 * i + 1, r.ss, e);
  seq_len = e - r.ss;
  const uint64_t cs = std::min(clip, seq_len);           // (an assigned unit has L >= m: the sample was eligible)
  r.ss += cs;
  r.sl = seq_len - cs;
  text_span(in, 4 * i, r.hs, e);
  r.hl = e - r.hs;
  text_span(in, 4 * i + 2, r.ps, e);
  r.pl = e - r.ps;
  text_span(in, 4 * i + 3, r.qs, e);
  const uint64_t cq = std::min(clip, e - r.qs);
  r.qs += cq;
  r.ql = e - r.qs;
  r.len = r.hl + r.sl + r.pl + r.ql + 4;
  // all four lines there, the last one with its newline, and no '\r' in front of any: the input holds the unclipped record byte for byte
  if (4 * i + 4 <= in.lines) {
    const uint64_t r1 = in.line_off[4 * i + 4];
    if (r1 <= in.n && r1 - in.line_off[4 * i] == r.len + cs + cq) r.kind = clip == 0 ? kWhole : kRuns;
  }
  return r;
}

// a record, by the whole wave: len bytes at dst
__device__ __forceinline__ void write_read(const RecInput& in, const DxRead& r, uint8_t* dst, uint32_t lane) {
  if (r.kind == kWhole) { wave_copy(dst, in.base + r.hs, r.len, lane); return; }
  uint8_t* const s = dst + r.hl + 1;
  uint8_t* const p = s + r.sl + 1;
  uint8_t* const q = p + r.pl + 1;
  if (r.kind == kRuns) {
    wave_copy(dst, in.base + r.hs, r.hl + 1, lane);
    wave_copy(s, in.base + r.ss, r.sl + r.pl + 2, lane);
    wave_copy(q, in.base + r.qs, r.ql + 1, lane);
    return;
  }
  wave_copy(dst, in.base + r.hs, r.hl, lane);
  wave_copy(s, in.base + r.ss, r.sl, lane);
  wave_copy(p, in.base + r.ps, r.pl, lane);
  wave_copy(q, in.base + r.qs, r.ql, lane);
  if (lane == 0) dst[r.hl] = '\n';
  if (lane == 1) s[r.sl] = '\n';
  if (lane == 2) p[r.pl] = '\n';
  if (lane == 3) q[r.ql] = '\n';
}

// a unit: a single-end read, or a pair.  What its reads add to the two outputs, and where it goes
struct DxUnit {
  DxRead m[2];
  uint64_t len1, len2;                 // bytes for out1 and out2
  uint64_t first;                      // of len1, mate 1's record (interleaved input: mate 2's follows it)
  uint64_t seq_len[2];
  uint32_t dest;                       // 0 .. N
  uint32_t perfect;                    // assigned with t = 0
};

// clip_on: inline mode without SCFQ_DEMUX_KEEP_BARCODE
__device__ __forceinline__ DxUnit look_up(const RecInput& a, const RecInput& b, uint64_t stride, uint64_t second, uint32_t paired, uint64_t u,
                                          const scfq_demux_rec* recs, const DxSheet& sh, uint32_t clip_on) {
  DxUnit t = {};
  const scfq_demux_rec rec = recs[u];
  const bool assigned = rec.state == SCFQ_DEMUX_ASSIGNED && rec.sample < sh.n;      // (the sample number indexes lens: it is below N)
  t.dest = assigned ? rec.sample : sh.n;
  t.perfect = assigned && rec.mm1 == 0 && rec.mm2 == 0;
  const uint32_t ml = assigned && clip_on ? sh.lens[rec.sample] : 0u;
  t.m[0] = read_of(a, paired ? u * stride : u, ml & 0xFFu, t.seq_len[0]);
  if (paired) t.m[1] = read_of(b, u * stride + second, ml >> 8, t.seq_len[1]);
  t.first = t.m[0].len;
  t.len1 = t.first + (paired && second ? t.m[1].len : 0);
  t.len2 = paired && !second ? t.m[1].len : 0;
  return t;
}

// a destination's sums on the device: kRowWords words per destination, and two words behind the N + 1 rows
enum { kRowUnits = 0, kRowPerfect, kRowMismatched, kRowBases, kRowBytes1, kRowBytes2, kRowWords };
enum { kBasesIn = 0, kBasesClipped, kTotals };

// X2.  order: the sorted unit numbers.  group_len: two arrays of n_groups + 1 entries, one after the other (the last entry of each
// stays 0: the scan's total).  rows: (N + 1) * kRowWords words, then kTotals
__global__ __launch_bounds__(256) void dx_lengths(RecInput a, RecInput b, uint64_t stride, uint64_t second, uint32_t paired, uint64_t units, const uint32_t* order,
                                                 const scfq_demux_rec* recs, DxSheet sh, uint32_t clip_on, uint64_t n_groups, uint64_t* group_len,
                                                 unsigned long long* rows) {
  __shared__ unsigned long long total_sh[kTotals];
  if (threadIdx.x < kTotals) total_sh[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t u = p < units ? order[p] : units;
  const bool live = u < units;                           // (a unit number that is none adds nothing anywhere)
  uint64_t len[2] = {0, 0}, c[kRowWords], bases_in = 0;
#pragma unroll
  for (int x = 0; x < kRowWords; ++x) c[x] = 0;
  uint32_t dest = sh.n;
  if (live) {
    const DxUnit t = look_up(a, b, stride, second, paired, u, recs, sh, clip_on);
    len[0] = t.len1; len[1] = t.len2;
    dest = t.dest;
    bases_in = t.seq_len[0] + t.seq_len[1];
    c[kRowUnits] = 1;
    c[kRowPerfect] = t.perfect;
    c[kRowMismatched] = dest < sh.n && !t.perfect;
    c[kRowBases] = t.m[0].sl + t.m[1].sl;
    c[kRowBytes1] = t.len1;
    c[kRowBytes2] = t.len2;
  }
#pragma unroll
  for (int x = 0; x < 2; ++x) store_group_len(len[x], x, p, units, n_groups, group_len);
  // the rows.  A wave's positions are neighbours in sorted order and nearly always have one destination: then the wave sums first and
  // its first lane adds once per word.  Where destinations meet, every lane adds for itself (dest <= N by look_up)
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t dest0 = (uint32_t)__shfl((int)dest, 0, 64);
  const bool one_dest = __builtin_amdgcn_ballot_w64(live && dest != dest0) == 0;
  if (one_dest) {
#pragma unroll
    for (int x = 0; x < kRowWords; ++x) {
      const uint64_t s = wave_sum(c[x]);
      if (lane == 0 && s) atomicAdd(&rows[(uint64_t)dest0 * kRowWords + x], (unsigned long long)s);
    }
  } else if (live) {
#pragma unroll
    for (int x = 0; x < kRowWords; ++x)
      if (c[x]) atomicAdd(&rows[(uint64_t)dest * kRowWords + x], (unsigned long long)c[x]);
  }
  const uint64_t in_sum = wave_sum(bases_in), clipped_sum = wave_sum(bases_in - c[kRowBases]);
  if (lane == 0 && in_sum) atomicAdd(&total_sh[kBasesIn], (unsigned long long)in_sum);
  if (lane == 0 && clipped_sum) atomicAdd(&total_sh[kBasesClipped], (unsigned long long)clipped_sum);
  __syncthreads();
  if (threadIdx.x < kTotals && total_sh[threadIdx.x]) atomicAdd(&rows[(uint64_t)(sh.n + 1) * kRowWords + threadIdx.x], total_sh[threadIdx.x]);
}

using ::bcast;      // (the overload below hides the shared ones otherwise)
__device__ __forceinline__ DxRead bcast(const DxRead& m, uint32_t from) {
  DxRead r;
  r.len = bcast(m.len, from);
  r.hs = bcast(m.hs, from); r.ss = bcast(m.ss, from); r.ps = bcast(m.ps, from); r.qs = bcast(m.qs, from);
  r.hl = bcast(m.hl, from); r.sl = bcast(m.sl, from); r.pl = bcast(m.pl, from); r.ql = bcast(m.ql, from);
  r.kind = bcast(m.kind, from);
  return r;
}

// X3.  group_off: the two scanned arrays of X2's layout
__global__ __launch_bounds__(64 * kDxWaves) void dx_write(RecInput a, RecInput b, uint64_t stride, uint64_t second, uint32_t paired, uint64_t units,
                                                         const uint32_t* order, const scfq_demux_rec* recs, DxSheet sh, uint32_t clip_on, uint64_t n_groups,
                                                         const uint64_t* group_off, RecOut o1, RecOut o2) {
  const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // (when one result is more than its output holds, nothing is written to either)
  if (!(output_fits(o1, 0, n_groups, group_off) && output_fits(o2, 1, n_groups, group_off))) return;
  const uint64_t g = (uint64_t)blockIdx.x * kDxWaves + wave;
  if (g >= n_groups) return;
  const uint64_t p0 = g * kDxGroup;
  const uint32_t count = (uint32_t)std::min<uint64_t>(kDxGroup, units - p0);
  DxUnit mine = {};
  uint64_t my_unit = units;
  if (lane < count) my_unit = order[p0 + lane];
  if (my_unit < units) mine = look_up(a, b, stride, second, paired, my_unit, recs, sh, clip_on);      // (a number that is none: nothing, as in X2)
  const uint64_t len[2] = {mine.len1, mine.len2};
  uint64_t at[2];
  place_units(len, g, n_groups, group_off, lane, at);
  for (uint32_t q = 0; q < count; ++q) {
    const uint64_t l1 = bcast(mine.len1, q), l2 = bcast(mine.len2, q), first = bcast(mine.first, q), w1 = bcast(at[0], q), w2 = bcast(at[1], q);
    if (l1 + l2 == 0) continue;                            // (only a unit number that is none: a record has its four '\n' at the least)
    const DxRead m1 = bcast(mine.m[0], q);                 // (every lane takes part in the shuffles)
    if (o1.p) write_read(a, m1, o1.p + w1, lane);
    if (paired) {
      const DxRead m2 = bcast(mine.m[1], q);
      if (second) { if (o1.p) write_read(b, m2, o1.p + w1 + first, lane); }
      else if (o2.p) write_read(b, m2, o2.p + w2, lane);
    }
  }
}

using scfq_demux_host::Params;

uint32_t key_bits(uint32_t n_samples) {                  // ceil(log2(N + 1)): the keys are 0 .. N
  uint32_t bits = 1;
  while ((1u << bits) < n_samples + 1) ++bits;
  return bits;
}

// recs_out / rec_cap: the caller's per-unit table (device memory), or nullptr; recs_keep: where the table stays for the caller of this
// function to copy it (the file entry point).  rows: N + 1 entries, complete on SCFQ_OK and on a too-small output
int demux_device(const scfq_demux_host::Sheet& sheet, const uint8_t* d1, uint64_t n1, const uint8_t* d2, uint64_t n2, Mode mode, const Params& prm,
                 scfq_demux_rec* recs_out, uint64_t rec_cap, bool check_rec_cap, DevBuf& recs_keep, scfq_demux_row* rows, bool own_outputs, Dest dst[2],
                 DevBuf own[2], bool check_caps, scfq_demux_stats* st, hipStream_t stream) {
  for (double& m : g_stage_ms) m = 0;
  const uint32_t N = sheet.n();
  const bool paired = mode != Mode::single, interleaved = mode == Mode::interleaved;
  st->input_bytes1 = n1;
  st->input_bytes2 = n2;
  st->flags = prm.flags; st->mismatches = prm.mismatches; st->n_samples = N; st->dual = sheet.dual ? 1 : 0;
  std::memset(rows, 0, (size_t)(N + 1) * sizeof(scfq_demux_row));
  scfq_overlap::Indexed ix;
  int rc = SCFQ_OK;
  double index_ms = 0;
  uint64_t units = 0, reads = 0;
  if ((rc = scfq_reads::index_units(d1, n1, d2, n2, mode, stream, g_xerr, ix, &index_ms, st, &units, &reads))) return rc;
  st->units_in = units;
  st->reads_in = st->reads_out = reads;
  if (check_rec_cap && recs_out && rec_cap < units) {
    std::snprintf(g_xerr, sizeof g_xerr, "the per-unit table holds %llu entries, the input has %llu units", (unsigned long long)rec_cap, (unsigned long long)units);
    return SCFQ_EARG;
  }
  if (units == 0) return SCFQ_OK;           // (two empty outputs: they fit into anything; nothing is launched)
  const uint64_t n_groups = (units + kDxGroup - 1) / kDxGroup;
  const uint64_t row_words = (uint64_t)(N + 1) * kRowWords + kTotals;
  DevBuf codes, lens, keys, keys2, idx, idx2, group_len, group_off, counters, d_rows, tmp;
  scfq_reads::GroupScan gs(2, n_groups, group_len, group_off, stream, g_xerr);
  if ((!recs_out && (rc = recs_keep.alloc(units * sizeof(scfq_demux_rec), stream, g_xerr))) || (rc = codes.alloc((size_t)N * 16, stream, g_xerr)) ||
      (rc = lens.alloc((size_t)N * 4, stream, g_xerr)) || (rc = keys.alloc(units * 2, stream, g_xerr)) || (rc = keys2.alloc(units * 2, stream, g_xerr)) ||
      (rc = idx.alloc(units * 4, stream, g_xerr)) || (rc = idx2.alloc(units * 4, stream, g_xerr)) || (rc = gs.alloc()) ||
      (rc = counters.alloc(kKinds * 8, stream, g_xerr)) || (rc = d_rows.alloc(row_words * 8, stream, g_xerr)))
    return rc;
  scfq_demux_rec* const recs = recs_out ? recs_out : recs_keep.as<scfq_demux_rec>();
  const uint32_t bits = key_bits(N);
  size_t scan_bytes = 0, sort_bytes = 0;
  if ((rc = gs.scratch_bytes(&scan_bytes))) return rc;
  SCFQ_SCRATCH_CHK(g_xerr, rocprim::radix_sort_pairs(nullptr, sort_bytes, keys.as<uint16_t>(), keys2.as<uint16_t>(), idx.as<uint32_t>(), idx2.as<uint32_t>(),
                                                     (size_t)units, 0u, bits, stream));
  if ((rc = tmp.alloc(std::max(scan_bytes, sort_bytes), stream, g_xerr))) return rc;
  static const bool timing = scfq_scratch::env_switch("SCFQ_DEMUX_TIMING");
  scfq_scratch::StageClock clk(stream, timing);
  SCFQ_SCRATCH_CHK(g_xerr, hipMemcpyAsync(codes.p, sheet.codes.data(), (size_t)N * 16, hipMemcpyHostToDevice, stream));
  SCFQ_SCRATCH_CHK(g_xerr, hipMemcpyAsync(lens.p, sheet.lens.data(), (size_t)N * 4, hipMemcpyHostToDevice, stream));
  SCFQ_SCRATCH_CHK(g_xerr, hipMemsetAsync(counters.p, 0, kKinds * 8, stream));
  SCFQ_SCRATCH_CHK(g_xerr, hipMemsetAsync(d_rows.p, 0, row_words * 8, stream));
  if ((rc = gs.zero())) return rc;
  const RecInput a = {d1, n1, ix.off1.as<uint64_t>(), ix.lines1, ix.cr1};
  const RecInput b = mode == Mode::two ? RecInput{d2, n2, ix.off2.as<uint64_t>(), ix.lines2, ix.cr2} : a;
  const uint64_t stride = interleaved ? 2 : 1, second = interleaved ? 1 : 0;
  const uint32_t header = (prm.flags & SCFQ_DEMUX_HEADER) ? 1u : 0u;
  const uint32_t clip_on = !header && !(prm.flags & SCFQ_DEMUX_KEEP_BARCODE) ? 1u : 0u;
  const DxSheet dsh = {codes.as<uint64_t>(), lens.as<uint32_t>(), N};
  const unsigned blocks = (unsigned)((units + 255) / 256);
  clk.mark(0);
  hipLaunchKernelGGL(dx_assign, dim3(blocks), dim3(256), 0, stream, a, b, stride, second, paired ? 1u : 0u, header, units, codes.as<uint64_t>(), lens.as<uint32_t>(),
                     N, prm.mismatches, recs, keys.as<uint16_t>(), idx.as<uint32_t>(), counters.as<unsigned long long>());
  SCFQ_SCRATCH_CHK(g_xerr, hipGetLastError());
  clk.mark(1);
  SCFQ_SCRATCH_CHK(g_xerr, rocprim::radix_sort_pairs(tmp.p, sort_bytes, keys.as<uint16_t>(), keys2.as<uint16_t>(), idx.as<uint32_t>(), idx2.as<uint32_t>(),
                                                     (size_t)units, 0u, bits, stream));
  clk.mark(2);
  const uint32_t* const order = idx2.as<uint32_t>();
  hipLaunchKernelGGL(dx_lengths, dim3(blocks), dim3(256), 0, stream, a, b, stride, second, paired ? 1u : 0u, units, order, recs, dsh, clip_on, n_groups,
                     gs.len(), d_rows.as<unsigned long long>());
  SCFQ_SCRATCH_CHK(g_xerr, hipGetLastError());
  if ((rc = gs.scan(tmp.p, scan_bytes))) return rc;
  clk.mark(3);
  // the sizes, the rows and the kinds come back first: pool memory for the outputs is taken to fit, and a caller's buffer that is too
  // small is known here, before anything is stored
  uint64_t kinds[kKinds];
  std::vector<uint64_t> h_rows(row_words);
  if ((rc = gs.read_totals())) return rc;
  SCFQ_SCRATCH_CHK(g_xerr, hipMemcpyAsync(kinds, counters.p, sizeof kinds, hipMemcpyDeviceToHost, stream));
  SCFQ_SCRATCH_CHK(g_xerr, hipMemcpyAsync(h_rows.data(), d_rows.p, row_words * 8, hipMemcpyDeviceToHost, stream));
  SCFQ_SCRATCH_CHK(g_xerr, hipStreamSynchronize(stream));
  st->out1_bytes = gs.total[0]; st->out2_bytes = gs.total[1];
  st->perfect = kinds[kPerfect]; st->mismatched = kinds[kMismatched];
  st->unmatched = kinds[kUnmatched]; st->ambiguous = kinds[kAmbiguous]; st->no_barcode = kinds[kNoBarcode];
  st->assigned = st->perfect + st->mismatched;
  st->undetermined = st->unmatched + st->ambiguous + st->no_barcode;
  uint64_t off[2] = {0, 0};
  for (uint32_t d = 0; d <= N; ++d) {
    const uint64_t* w = &h_rows[(size_t)d * kRowWords];
    rows[d] = scfq_demux_row{w[kRowUnits], w[kRowPerfect], w[kRowMismatched], w[kRowBases], w[kRowBytes1], w[kRowBytes2], off[0], off[1]};
    off[0] += w[kRowBytes1]; off[1] += w[kRowBytes2];
    st->bases_out += w[kRowBases];
  }
  st->bases_in = h_rows[(size_t)(N + 1) * kRowWords + kBasesIn];
  st->bases_clipped = h_rows[(size_t)(N + 1) * kRowWords + kBasesClipped];
  const scfq_reads::Placement put = scfq_reads::place_outputs(gs, scfq_reads::kOutNames, dst, own_outputs, check_caps, false, own, stream, g_xerr);
  if (put.rc) return put.rc;
  if (put.out[0].p || put.out[1].p) {
    hipLaunchKernelGGL(dx_write, dim3((unsigned)((n_groups + kDxWaves - 1) / kDxWaves)), dim3(64 * kDxWaves), 0, stream, a, b, stride, second, paired ? 1u : 0u,
                       units, order, recs, dsh, clip_on, n_groups, gs.off(), put.out[0], put.out[1]);
    SCFQ_SCRATCH_CHK(g_xerr, hipGetLastError());
  }
  clk.mark(4);
  SCFQ_SCRATCH_CHK(g_xerr, hipStreamSynchronize(stream));
  for (int k = 0; k < 4; ++k) g_stage_ms[k] = clk.between(k, k + 1);
  return put.verdict;      // (SCFQ_EARG for an output that is too small: place_outputs has left the text)
}

// what both entry points decide before any device call
bool args_ok(const scfq_demux_sheet* sheet, const scfq_demux_opts* opts, const scfq_demux_stats* st, const scfq_demux_row* rows, uint64_t row_cap, Params& p) {
  if (!st || st->struct_size != sizeof(scfq_demux_stats) || (opts && opts->struct_size != sizeof(scfq_demux_opts))) return false;
  if (!sheet) { std::snprintf(g_xerr, sizeof g_xerr, "the sheet is NULL"); return false; }
  if (!scfq_demux_host::params_ok(opts, p, g_xerr)) return false;
  if (!rows || row_cap < (uint64_t)sheet->sh.n() + 1) {
    std::snprintf(g_xerr, sizeof g_xerr, "the rows hold %llu entries, the sheet needs %u (its samples and one more)", (unsigned long long)(rows ? row_cap : 0), sheet->sh.n() + 1);
    return false;
  }
  return true;
}

}  // namespace

extern "C" {

const char* scfq_demux_error_detail(void) { return g_xerr; }

int scfq_debug_demux_stages(double* ms, uint32_t cap) { return scfq_scratch::copy_stage_ms(g_stage_ms, ms, cap); }

int scfq_demux_sheet_new(const scfq_demux_sample* samples, uint32_t n, scfq_demux_sheet** out) {
  g_xerr[0] = '\0';
  if (!out) return SCFQ_EARG;
  *out = nullptr;
  scfq_demux_sheet* sheet = new scfq_demux_sheet();
  if (!scfq_demux_host::build_sheet(samples, n, sheet->sh, g_xerr)) { delete sheet; return SCFQ_EARG; }
  *out = sheet;
  return SCFQ_OK;
}

void scfq_demux_sheet_free(scfq_demux_sheet* sheet) { delete sheet; }

uint32_t scfq_demux_sheet_samples(const scfq_demux_sheet* sheet) { return sheet ? sheet->sh.n() : 0u; }

const char* scfq_demux_sheet_name(const scfq_demux_sheet* sheet, uint32_t s) {
  if (!sheet || s > sheet->sh.n()) return nullptr;
  return s == sheet->sh.n() ? "undetermined" : sheet->sh.name[s].c_str();
}

int scfq_format_demux_row_tsv(const scfq_demux_stats* s, const scfq_demux_sheet* sheet, uint32_t d, const scfq_demux_row* row, char* buf, uint64_t cap) {
  if (!sheet) return SCFQ_EARG;
  return scfq_demux_host::format_row(s, sheet->sh, d, row, buf, cap);
}

int scfq_demux_buffers(const scfq_demux_sheet* sheet, const void* r1, uint64_t n1, const void* r2, uint64_t n2, int is_device, const scfq_demux_opts* opts,
                       scfq_demux_rec* recs_device, uint64_t rec_cap, scfq_demux_row* rows_host, uint64_t row_cap, void* out1, uint64_t cap1, void* out2,
                       uint64_t cap2, int out_is_device, scfq_demux_stats* stats) {
  g_xerr[0] = '\0';
  Params prm;
  if (!args_ok(sheet, opts, stats, rows_host, row_cap, prm) || (!r1 && n1) || (!r2 && n2) || (!out1 && cap1) || (!out2 && cap2) || (!recs_device && rec_cap))
    return SCFQ_EARG;
  const bool interleaved = (prm.flags & SCFQ_DEMUX_INTERLEAVED) != 0;
  if (interleaved && (r2 || n2)) { std::snprintf(g_xerr, sizeof g_xerr, "interleaved input takes no second buffer"); return SCFQ_EARG; }
  const Mode mode = interleaved ? Mode::interleaved : (r2 ? Mode::two : Mode::single);
  if (mode != Mode::two && out2) { std::snprintf(g_xerr, sizeof g_xerr, "one input has no second output (out2)"); return SCFQ_EARG; }
  if (!scfq_demux_host::sheet_fits_input(sheet->sh, prm, mode != Mode::single, g_xerr)) return SCFQ_EARG;
  scfq_scratch::clear_keep_size(stats);
  Dest dst[2] = {{static_cast<uint8_t*>(out1), cap1, out1 != nullptr}, {static_cast<uint8_t*>(out2), cap2, out2 != nullptr}};
  const bool any_out = out1 || out2, direct = any_out && out_is_device;
  scfq_scratch::ResidentInput in1, in2;
  int rc = in1.from_buffer(r1, n1, is_device != 0, is_device || direct || recs_device, g_xerr);
  if (rc) return rc;
  if (mode == Mode::two && (rc = in2.from_buffer(r2, n2, is_device != 0, false, g_xerr))) return rc;
  DevBuf own[2], recs_keep;
  rc = demux_device(sheet->sh, in1.d_in, in1.n, in2.d_in, in2.n, mode, prm, recs_device, rec_cap, true, recs_keep, rows_host, /*own_outputs=*/!direct, dst, own,
                    /*check_caps=*/true, stats, in1.stream);
  if (rc) return finish(in1, rc);
  if (!direct) {
    const uint64_t bytes[2] = {stats->out1_bytes, stats->out2_bytes};
    if ((rc = scfq_reads::outputs_to_host(2, dst, own, bytes, in1.stream, g_xerr))) return rc;
    SCFQ_SCRATCH_CHK(g_xerr, hipStreamSynchronize(in1.stream));
  }
  for (DevBuf& o : own) o.drop();
  recs_keep.drop();
  in1.mark_clean();      // (the last act was to wait for the stream; behind it lie returns of pool memory only)
  return SCFQ_OK;
}

int scfq_demux_files(const scfq_demux_sheet* sheet, const char* path1, const char* path2, const scfq_opts* opts, const scfq_demux_opts* dopts, const char* out_dir,
                     scfq_demux_rec* recs_host, uint64_t rec_cap, scfq_demux_row* rows_host, uint64_t row_cap, scfq_demux_stats* stats) {
  g_xerr[0] = '\0';
  Params prm;
  if (!path1 || !args_ok(sheet, dopts, stats, rows_host, row_cap, prm) || (!recs_host && rec_cap)) return SCFQ_EARG;
  const bool interleaved = (prm.flags & SCFQ_DEMUX_INTERLEAVED) != 0;
  if (interleaved && path2) { std::snprintf(g_xerr, sizeof g_xerr, "interleaved input takes no second file"); return SCFQ_EARG; }
  const Mode mode = interleaved ? Mode::interleaved : (path2 ? Mode::two : Mode::single);
  const bool two = mode == Mode::two;
  if (!scfq_demux_host::sheet_fits_input(sheet->sh, prm, mode != Mode::single, g_xerr)) return SCFQ_EARG;
  if (out_dir) {
    struct stat sb;
    if (stat(out_dir, &sb) != 0 || !S_ISDIR(sb.st_mode)) { std::snprintf(g_xerr, sizeof g_xerr, "%.400s is not a directory", out_dir); return SCFQ_EARG; }
  }
  scfq_scratch::clear_keep_size(stats);
  scfq_scratch::ResidentInput in1, in2;
  int rc = in1.from_file(path1, opts, g_xerr);
  if (rc) return rc;
  if (two && (rc = in2.from_file(path2, opts, g_xerr))) return rc;      // (staged when this returns)
  Dest dst[2] = {{nullptr, 0, out_dir != nullptr}, {nullptr, 0, out_dir != nullptr && two}};
  DevBuf own[2], recs_keep;
  rc = demux_device(sheet->sh, in1.d_in, in1.n, in2.d_in, in2.n, mode, prm, nullptr, 0, false, recs_keep, rows_host, /*own_outputs=*/true, dst, own, /*check_caps=*/false, stats, in1.stream);
  if (rc) return finish(in1, rc);
  if (recs_host && stats->units_in) {
    if (rec_cap < stats->units_in) {
      std::snprintf(g_xerr, sizeof g_xerr, "the per-unit table holds %llu entries, the input has %llu units", (unsigned long long)rec_cap, (unsigned long long)stats->units_in);
      return finish(in1, SCFQ_EARG);
    }
    SCFQ_SCRATCH_CHK(g_xerr, hipMemcpyAsync(recs_host, recs_keep.p, stats->units_in * sizeof(scfq_demux_rec), hipMemcpyDeviceToHost, in1.stream));
    SCFQ_SCRATCH_CHK(g_xerr, hipStreamSynchronize(in1.stream));
  }
  if (!out_dir) { in1.mark_clean(); return SCFQ_OK; }
  // a file per destination and output, one after the other and ONE descriptor open at a time: HBM -> two pinned buffers -> write()
  scfq_fdwrite::Pinned pinned;
  if ((own[0].p || own[1].p) && (rc = pinned.init(g_xerr))) return finish(in1, rc);
  for (uint32_t d = 0; d <= sheet->sh.n(); ++d)
    for (int x = 0; x < (two ? 2 : 1); ++x) {
      const std::string path = scfq_demux_host::out_path(sheet->sh, out_dir, d, two, x + 1);
      const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
      if (fd < 0) { std::snprintf(g_xerr, sizeof g_xerr, "cannot create %.400s: %s", path.c_str(), std::strerror(errno)); return finish(in1, SCFQ_EIO); }
      const uint64_t off = x ? rows_host[d].off2 : rows_host[d].off1, bytes = x ? rows_host[d].bytes2 : rows_host[d].bytes1;
      rc = own[x].p && bytes ? pinned.device_to_fd(own[x].as<uint8_t>() + off, bytes, fd, in1.stream, g_xerr) : SCFQ_OK;
      if (close(fd) != 0 && rc == SCFQ_OK) { std::snprintf(g_xerr, sizeof g_xerr, "close %.400s: %s", path.c_str(), std::strerror(errno)); rc = SCFQ_EIO; }
      if (rc) return finish(in1, rc);
    }
  return SCFQ_OK;
}

}  // extern "C"

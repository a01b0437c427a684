// fa_tile_device.hpp — internal: the tile classifier the kernels of `sc fa-gc` (scfq_fagc.hip: fa_tile_scan, fa_contigs,
// fa_rank_count) share.  Definitions (lines, bases, classes) in include/sc_fqcount.h.
//
// A TILE is kFaTileBytes of the ADDRESS grid (the input pointer may have any alignment: the first and the last tile are
// ragged), walked by one wave in kFaSteps STEPS of 1 KiB: a lane holds 16 consecutive bytes, loaded as one aligned uint4
// (the wave's load is 1 KiB, coalesced), and makes of them 16-bit masks, bit i for its byte i.  What carries from a step to
// the next is wave-uniform: whether the step's last byte is '\n', and the kind of the line that is open.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

constexpr uint32_t kFaTileBytes = 4096;
constexpr uint32_t kFaStepBytes = 64 * 16;
constexpr uint32_t kFaSteps = kFaTileBytes / kFaStepBytes;

struct FaMasks {       // bit i: byte i of the lane's 16 (0 for a byte outside the input)
  uint32_t nl;         // '\n'
  uint32_t gt;         // '>'
  uint32_t base;       // 0x21 .. 0x7E
  uint32_t gc;         // G C g c
  uint32_t acgt;       // A C G T a c g t
};

// 0x80 in every byte of x that is zero (exact: no borrow runs from one byte into the next)
__device__ __forceinline__ uint32_t fa_zero_bytes(uint32_t x) { return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu); }
// the four 0x80 flags of a word as bits 0 .. 3
__device__ __forceinline__ uint32_t fa_pack4(uint32_t flags) { return ((flags >> 7) * 0x01020408u) >> 24 & 0xfu; }

// The per-lane classifier: 16 bytes -> masks.  valid: bit i set when byte i belongs to the input.
__device__ __forceinline__ FaMasks fa_classify(const uint32_t (&w)[4], uint32_t valid) {
  FaMasks m = {0, 0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t x = w[k];
    const uint32_t up = x & 0xdfdfdfdfu;                       // 'a' .. 'z' -> 'A' .. 'Z'; nothing else lands on A C G T
    const uint32_t low7 = x & 0x7f7f7f7fu;
    const uint32_t nl = fa_zero_bytes(x ^ 0x0a0a0a0au);
    const uint32_t gt = fa_zero_bytes(x ^ 0x3e3e3e3eu);
    const uint32_t gc = fa_zero_bytes(up ^ 0x43434343u) | fa_zero_bytes(up ^ 0x47474747u);
    const uint32_t at = fa_zero_bytes(up ^ 0x41414141u) | fa_zero_bytes(up ^ 0x54545454u);
    // 0x21 <= b <= 0x7E: the top bit clear, low7 + 0x5F carries into it, low7 + 0x01 does not
    const uint32_t base = (low7 + 0x5f5f5f5fu) & ~(low7 + 0x01010101u) & ~x & 0x80808080u;
    m.nl |= fa_pack4(nl) << (4 * k);
    m.gt |= fa_pack4(gt) << (4 * k);
    m.gc |= fa_pack4(gc) << (4 * k);
    m.acgt |= fa_pack4(gc | at) << (4 * k);
    m.base |= fa_pack4(base) << (4 * k);
  }
  m.nl &= valid; m.gt &= valid; m.base &= valid; m.gc &= valid; m.acgt &= valid;
  return m;
}

// A lane's 16 bytes at input offset o (o may be negative or reach behind the input in the ragged tiles): only bytes of the
// input are read.  base + o is 16-byte aligned.
__device__ __forceinline__ uint32_t fa_load16(const uint8_t* base, uint64_t n, int64_t o, uint32_t (&w)[4]) {
  if (o >= 0 && o + 16 <= (int64_t)n) {
    const uint4 q = *reinterpret_cast<const uint4*>(base + o);
    w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
    return 0xffffu;
  }
  uint32_t valid = 0;
  w[0] = w[1] = w[2] = w[3] = 0;
  for (int i = 0; i < 16; ++i) {
    const int64_t p = o + i;
    if (p >= 0 && p < (int64_t)n) {
      w[i >> 2] |= (uint32_t)base[p] << (8 * (i & 3));
      valid |= 1u << i;
    }
  }
  return valid;
}

// What a wave carries through the steps of a tile (every field wave-uniform).
struct FaCarry {
  bool prev_nl;        // the byte before the step's first one is '\n'
  bool known;          // the kind of the open line is known (false only in fa_tile_scan, before the tile's first line start)
  bool hdr;            // ... and it is a header line
};

struct FaStep {
  FaMasks m;
  uint32_t ls;         // line starts: the byte behind a '\n', and byte 0 of the input
  uint32_t hs;         // header-line starts: ls & '>'
  uint32_t hdr;        // bytes of header lines (of a line whose kind is known)
  uint32_t head;       // bytes before the tile's first line start while the kind of that line is not known
};

// One step of one tile.  o: input offset of this lane's byte 0.  first_step: the step is the tile's first one (the byte in
// front of the tile is looked at, one global load by lane 0).  The carry is advanced to the next step.
__device__ __forceinline__ FaStep fa_step(const uint8_t* base, uint64_t n, int64_t o, uint32_t lane, bool first_step, FaCarry& c) {
  FaStep s;
  uint32_t w[4];
  const uint32_t valid = fa_load16(base, n, o, w);
  s.m = fa_classify(w, valid);
  if (first_step) {
    int prev = 0;
    if (lane == 0 && o > 0 && o <= (int64_t)n) prev = base[o - 1] == '\n';
    c.prev_nl = __shfl(prev, 0, 64) != 0;
  }
  // line starts: behind the '\n' of this lane, of the lane before (of the step before for lane 0), and byte 0 of the input
  const uint32_t up = __shfl_up(s.m.nl >> 15, 1, 64);
  s.ls = ((s.m.nl << 1) | (lane ? up : (c.prev_nl ? 1u : 0u))) & 0xffffu;
  if (o <= 0 && o > -16) s.ls |= 1u << (uint32_t)(-o);
  s.hs = s.ls & s.m.gt;
  // the line open at this lane's byte 0: that of the last line start in a lane before it, else the carried one
  const uint32_t top = s.ls ? 31u - (uint32_t)__builtin_clz(s.ls) : 0u;
  const uint64_t b_has = __builtin_amdgcn_ballot_w64(s.ls != 0);
  const uint64_t b_hdr = __builtin_amdgcn_ballot_w64(s.ls != 0 && ((s.hs >> top) & 1u));
  const uint64_t below = b_has & ((1ull << lane) - 1ull);
  bool known = c.known, in_hdr = c.hdr;
  if (below) {
    known = true;
    in_hdr = (b_hdr >> (63 - __builtin_clzll(below))) & 1ull;
  }
  const uint32_t pre = s.ls ? (1u << (uint32_t)__builtin_ctz(s.ls)) - 1u : 0xffffu;
  s.head = known ? 0u : pre;
  s.hdr = (known && in_hdr) ? pre : 0u;
  for (uint32_t m = s.ls; m;) {
    const uint32_t b = (uint32_t)__builtin_ctz(m);
    m &= m - 1;
    const uint32_t end = m ? (uint32_t)__builtin_ctz(m) : 16u;
    if ((s.hs >> b) & 1u) s.hdr |= ((1u << end) - 1u) & ~((1u << b) - 1u);
  }
  // the carry of the next step
  c.prev_nl = __shfl((int)(s.m.nl >> 15), 63, 64) != 0;
  if (b_has) {
    c.known = true;
    c.hdr = (b_hdr >> (63 - __builtin_clzll(b_has))) & 1ull;
  }
  return s;
}

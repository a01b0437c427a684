// scfq_record_device.hpp — internal: the device-side helpers the kernels of the record pipelines (dd_*, rs_*, cy_*) share.
// (Not here: a lane's 16-byte chunk load of rs_reduce and cy_count.  The two are written differently — words in named registers
// there, an indexed array here — and either form as one shared function changes the other kernel's registers: rs_reduce goes
// from 62 to 65 VGPRs and from 8 to 7 waves per SIMD with its own form, cy_count from 61 to 81 VGPRs with rs_reduce's.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// text of line j: [line_off[j], end) where end excludes the '\n' and a '\r' directly before a REAL '\n'
// (Nim 1.0.6 readLine; a final line without '\n' keeps a trailing '\r')
__device__ __forceinline__ void line_span(const uint8_t* base, uint64_t n, const uint64_t* line_off, uint64_t j,
                                          uint64_t& s, uint64_t& e, bool has_cr = true) {
  s = line_off[j];
  const uint64_t nlpos = line_off[j + 1] - 1;     // position of the (real or implied) '\n'
  e = nlpos;
  if (has_cr && nlpos < n && e > s && base[e - 1] == '\r') --e;      // (has_cr: kernel-uniform, from the index pass)
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor((unsigned long long)v, o, 64);
  return v;
}
__device__ __forceinline__ uint64_t wave_max(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const uint64_t x = __shfl_xor((unsigned long long)v, o, 64); v = x > v ? x : v; }
  return v;
}
__device__ __forceinline__ uint64_t wave_min(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const uint64_t x = __shfl_xor((unsigned long long)v, o, 64); v = x < v ? x : v; }
  return v;
}

// A contiguous copy by one wave, source and destination arbitrarily aligned (fq-dedup's gather, fq-merge's echo of unmerged records).
// The copy keeps EIGHT 16-byte loads per lane in flight before the first store.  Measured r4 and left out again: non-temporal stores
// (8 % slower here, though 2 % faster in the aligned copy micro-benchmark), the body aligned to 64 or 128 bytes of the destination
// instead of 16 (no difference): profiles/r04/dedup_ab.txt, copy_shapes.txt — the gather runs at what a copy reaches on this device.
__device__ __forceinline__ void wave_copy(uint8_t* dst, const uint8_t* src, uint64_t len, uint32_t lane) {
  typedef uint32_t v4u __attribute__((ext_vector_type(4)));
  uint64_t head = (16 - ((uintptr_t)dst & 15)) & 15;
  if (head > len) head = len;
  if (lane < head) dst[lane] = src[lane];
  const uint64_t body = (len - head) / 16;
  const uint8_t* sp = src + head;
  uint8_t* dp = dst + head;
  auto put = [&](const v4u& v, uint64_t k) { *reinterpret_cast<v4u*>(dp + k * 16) = v; };
  uint64_t k = lane;
  for (; k + 7 * 64 < body; k += 8 * 64) {
    v4u v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) __builtin_memcpy(&v[u], sp + (k + 64u * u) * 16, 16);       // the source is arbitrarily aligned
#pragma unroll
    for (int u = 0; u < 8; ++u) put(v[u], k + 64u * u);
  }
  if (k + 3 * 64 < body) {
    v4u v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) __builtin_memcpy(&v[u], sp + (k + 64u * u) * 16, 16);
#pragma unroll
    for (int u = 0; u < 4; ++u) put(v[u], k + 64u * u);
    k += 4 * 64;
  }
  {   // at most four steps are left: all their loads first as well
    v4u v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) if (k + 64u * u < body) __builtin_memcpy(&v[u], sp + (k + 64u * u) * 16, 16);
#pragma unroll
    for (int u = 0; u < 4; ++u) if (k + 64u * u < body) put(v[u], k + 64u * u);
  }
  for (uint64_t t = head + body * 16 + lane; t < len; t += 64) dst[t] = src[t];
}

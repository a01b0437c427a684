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

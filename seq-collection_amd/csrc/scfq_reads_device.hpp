// scfq_reads_device.hpp — internal: the device side the pipelines that write reads (mg_*, tr_*, sc_*, dx_*, nm_*, cx_*, ru_*) share: an
// input and an output as a kernel sees them, a record echoed as it stands, and the steps every lengths and every write kernel takes
// around a group of kRecGroup units.  What a unit is, what it adds to the outputs (look_up, read_of, write_read) and the kernels
// themselves stay with their pipeline.
#pragma once
#include "scfq_record_device.hpp"

constexpr uint32_t kRecGroup = 32;     // units of a group: one wave of a write kernel, one entry of the scans, one half wave of a lengths kernel

struct RecInput {         // one input: the bytes and their line index
  const uint8_t* base;
  uint64_t n;
  const uint64_t* line_off;
  uint64_t lines;
  bool has_cr;
};

struct RecOut {           // one output: where it goes (nullptr: nowhere) and what it holds
  uint8_t* p;
  uint64_t cap;
};

// the text of line j (a line the input does not have is empty)
__device__ __forceinline__ void text_span(const RecInput& in, uint64_t j, uint64_t& s, uint64_t& e) {
  s = e = 0;
  if (j < in.lines) line_span(in.base, in.n, in.line_off, j, s, e, in.has_cr);
}

// bytes record i echoes: its lines 4i .. min(4i+3, lines-1), each text + '\n' (dd_record_lengths' rule)
__device__ __forceinline__ uint64_t echo_len(const RecInput& in, uint64_t i) {
  if (4 * i >= in.lines) return 0;
  if (!in.has_cr) {
    const uint64_t j1 = (4 * i + 4 < in.lines) ? 4 * i + 4 : in.lines;
    return in.line_off[j1] - in.line_off[4 * i];
  }
  uint64_t total = 0;
  for (uint64_t j = 4 * i; j < 4 * i + 4 && j < in.lines; ++j) {
    uint64_t s, e;
    line_span(in.base, in.n, in.line_off, j, s, e);
    total += e - s + 1;
  }
  return total;
}

// record i of `in` echoed to dst, len bytes (dd_gather's rule: one copy when the echo is the record's own bytes)
__device__ __forceinline__ void echo_record(const RecInput& in, uint64_t i, uint8_t* dst, uint64_t len, uint32_t lane) {
  if (!len) return;
  const uint64_t j0 = 4 * i, j1 = (j0 + 4 < in.lines) ? j0 + 4 : in.lines;
  const uint64_t r0 = in.line_off[j0], r1 = in.line_off[j1];
  if (r1 - r0 == len && r1 <= in.n) { wave_copy(dst, in.base + r0, len, lane); return; }
  uint64_t w = 0;
  for (uint64_t j = j0; j < j1; ++j) {
    uint64_t s, e;
    line_span(in.base, in.n, in.line_off, j, s, e);
    for (uint64_t k = lane; k < e - s; k += 64) dst[w + k] = in.base[s + k];
    if (lane == 0) dst[w + (e - s)] = '\n';
    w += e - s + 1;
  }
}

__device__ __forceinline__ uint64_t half_sum(uint64_t v) {      // over the 32 lanes of a half wave
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor((unsigned long long)v, o, 64);
  return v;
}

__device__ __forceinline__ uint64_t bcast(uint64_t v, uint32_t from) { return (uint64_t)__shfl((unsigned long long)v, (int)from, 64); }
__device__ __forceinline__ uint32_t bcast(uint32_t v, uint32_t from) { return (uint32_t)__shfl((int)v, (int)from, 64); }

// A lengths kernel (a thread per position, 256 per block): the bytes the group of position `pos` adds to output k, summed over its half
// wave and stored by the first lane of it.  group_len: one array of n_groups + 1 entries per output, one after the other (the last
// entry of each stays 0: the scan's total).  count: the positions there are; a lane at or behind it brings 0.  Every lane of the wave
// gets here, once per output
__device__ __forceinline__ void store_group_len(uint64_t len, uint32_t k, uint64_t pos, uint64_t count, uint64_t n_groups, uint64_t* group_len) {
  const uint64_t s = half_sum(len);
  if ((threadIdx.x & 31) == 0 && pos < count) group_len[(uint64_t)k * (n_groups + 1) + pos / kRecGroup] = s;
}

// A write kernel.  group_off: the K scanned arrays of group_len's layout; each scan's last entry is its output's size.  Output k of
// them holds its result (a write kernel stores nothing anywhere unless all do)
__device__ __forceinline__ bool output_fits(const RecOut& o, uint32_t k, uint64_t n_groups, const uint64_t* group_off) {
  const uint64_t* off = group_off + (uint64_t)k * (n_groups + 1);
  return !o.p || off[n_groups] <= o.cap;
}

// Where the unit of this lane goes in each of the K outputs: group g's offset and the lengths of the units in front of it in the
// group.  len: what this lane's unit adds (0 for a lane behind the group's count).  Every lane of the wave gets here
template <int K>
__device__ __forceinline__ void place_units(const uint64_t (&len)[K], uint64_t g, uint64_t n_groups, const uint64_t* group_off, uint32_t lane, uint64_t (&at)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    uint64_t v = len[k];
#pragma unroll
    for (int o = 1; o < (int)kRecGroup; o <<= 1) {
      const uint64_t up = __shfl_up((unsigned long long)v, o, 64);
      if (lane >= (uint32_t)o) v += up;
    }
    const uint64_t* off = group_off + (uint64_t)k * (n_groups + 1);
    at[k] = v + off[g] - len[k];
  }
}

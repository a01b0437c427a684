// scfq_reads_host.hpp — internal: the host side the pipelines that write reads (fq-merge, fq-trim, fq-screen, fq-demux, fq-normalize,
// fq-complexity, fq-rmdup, fq-repair) share, between the scaffold of every record pipeline (scfq_scratch.hpp) and their own kernels: the units of
// the inputs, the scans over the groups' lengths, where the outputs go and how they leave.  Every function takes the pipeline's
// thread-local error buffer (kErrBytes) as errbuf.
#pragma once
#include "../../include/sc_fqcount.h"

#include <cstring>        // (rocprim's texture iterator calls memset from host code)
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "scfq_copy_text.hpp"
#include "scfq_fdwrite.hpp"
#include "scfq_overlap.hpp"
#include "scfq_reads_device.hpp"
#include "scfq_scratch.hpp"

#include <cstdio>

namespace scfq_reads {

using scfq_scratch::DevBuf;

enum class Mode { single, two, interleaved };

// one output of a call: `want` it, and then the caller's device memory (p, cap) or, with own_outputs, pool memory that place_outputs
// takes by the size the scan reports (own[k]; cap is then the caller's host capacity, checked all the same)
struct Dest { uint8_t* p; uint64_t cap; bool want; };
constexpr int kMaxOutputs = 4;
constexpr const char* kOutNames[2] = {"out1", "out2"};

// after a failure kernels that read the second input may still be queued on the first one's stream: they are waited for before the
// second input's memory goes back
inline int finish(scfq_scratch::ResidentInput& in1, int rc) {
  if (rc != SCFQ_OK) (void)hipStreamSynchronize(in1.stream);
  return rc;
}

// K5 of the inputs and what follows from their line counts, into ix and st: index_inputs for paired input (*index_ms: its host
// clock), the one line index for single-end input.  units: the pairs, or the reads; reads (or nullptr): both mates of the pairs, or the reads.
// SCFQ_EARG with text for 2^31 records or more in one input: the lines and reads of st are set then as well
template <typename Stats>
int index_units(const uint8_t* d1, uint64_t n1, const uint8_t* d2, uint64_t n2, Mode mode, hipStream_t stream, char* errbuf, scfq_overlap::Indexed& ix,
                double* index_ms, Stats* st, uint64_t* units, uint64_t* reads) {
  const bool paired = mode != Mode::single;
  int rc = SCFQ_OK;
  if (paired) {
    rc = scfq_overlap::index_inputs(d1, n1, d2, n2, mode == Mode::interleaved, stream, errbuf, ix, index_ms);
  } else {
    if ((rc = scfq_scratch::build_line_index(d1, n1, stream, errbuf, ix.off1, &ix.lines1, &ix.cr1))) return rc;
    ix.reads1 = (ix.lines1 + 3) / 4;
    if (ix.reads1 >= (1ull << 31)) { std::snprintf(errbuf, scfq_scratch::kErrBytes, "more than 2^31 records in one input"); rc = SCFQ_EARG; }
  }
  st->lines1 = ix.lines1; st->lines2 = ix.lines2;
  st->reads1 = ix.reads1; st->reads2 = ix.reads2;
  if (rc) return rc;
  st->pairs = ix.pairs;
  st->unpaired = ix.unpaired;
  *units = paired ? ix.pairs : ix.reads1;
  if (reads) *reads = paired ? 2 * ix.pairs : ix.reads1;
  return SCFQ_OK;
}

// The scans between a lengths kernel and a write kernel: `rows` arrays (one per output) of n_groups + 1 entries, one after the other,
// hold the bytes every group adds; their exclusive scans are the groups' offsets, and each scan's last entry is its output's size.
// Every step queues on the call's stream, in the order the pipeline calls them
struct GroupScan {
  const int rows;
  const uint64_t n_groups, row;
  const hipStream_t stream;
  char* const errbuf;
  DevBuf &len_, &off_;                           // the caller's, declared among its other buffers: pool memory goes back in that order
  uint64_t total[kMaxOutputs] = {0, 0, 0, 0};    // the outputs' sizes: read_totals, once the stream has been waited for

  GroupScan(int rows_, uint64_t n_groups_, DevBuf& group_len, DevBuf& group_off, hipStream_t stream_, char* errbuf_)
      : rows(rows_), n_groups(n_groups_), row(n_groups_ + 1), stream(stream_), errbuf(errbuf_), len_(group_len), off_(group_off) {}
  uint64_t* len() { return len_.as<uint64_t>(); }
  uint64_t* off() { return off_.as<uint64_t>(); }
  int alloc() {
    const int rc = len_.alloc(rows * row * 8, stream, errbuf);
    return rc ? rc : off_.alloc(rows * row * 8, stream, errbuf);
  }
  // rocprim's temporary storage for one scan
  int scratch_bytes(size_t* bytes) {
    SCFQ_SCRATCH_CHK(errbuf, rocprim::exclusive_scan(nullptr, *bytes, len(), off(), (uint64_t)0, (size_t)row, rocprim::plus<uint64_t>(), stream));
    return SCFQ_OK;
  }
  // in front of the lengths kernel (each scan's last input stays 0: its last output is the total)
  int zero() {
    SCFQ_SCRATCH_CHK(errbuf, hipMemsetAsync(len_.p, 0, rows * row * 8, stream));
    return SCFQ_OK;
  }
  // behind the lengths kernel; tmp holds tmp_bytes, scratch_bytes at the least
  int scan(void* tmp, size_t tmp_bytes) {
    for (uint64_t k = 0; k < (uint64_t)rows; ++k) {
      size_t bytes = tmp_bytes;
      SCFQ_SCRATCH_CHK(errbuf, rocprim::exclusive_scan(tmp, bytes, len() + k * row, off() + k * row, (uint64_t)0, (size_t)row, rocprim::plus<uint64_t>(), stream));
    }
    return SCFQ_OK;
  }
  int read_totals() {
    for (uint64_t k = 0; k < (uint64_t)rows; ++k) SCFQ_SCRATCH_CHK(errbuf, hipMemcpyAsync(&total[k], off() + k * row + n_groups, 8, hipMemcpyDeviceToHost, stream));
    return SCFQ_OK;
  }
};

// Where the outputs go, once the totals are known.  out[k]: nowhere for an output that is not wanted, or when nothing is to be
// written at all (hold_back).  The caller's device memory otherwise, too small or not: the write kernel looks at the totals itself and
// stores nothing anywhere.  With own_outputs pool memory of the total's size into own[k], none where the total is 0 or where an output
// is too small.  rc: a failed allocation, which ends the call at once.  verdict: SCFQ_EARG, with the text in errbuf, when a wanted
// output's capacity (check_caps) is below its total (the first such output is named); the call returns it once its statistics are complete
struct Placement {
  RecOut out[kMaxOutputs];
  int rc, verdict;
};
inline Placement place_outputs(const GroupScan& gs, const char* const* names, const Dest* dst, bool own_outputs, bool check_caps, bool hold_back, DevBuf* own,
                               hipStream_t stream, char* errbuf) {
  Placement put = {{{nullptr, 0}, {nullptr, 0}, {nullptr, 0}, {nullptr, 0}}, SCFQ_OK, SCFQ_OK};
  int small = -1;
  for (int k = gs.rows - 1; k >= 0; --k)
    if (check_caps && dst[k].want && gs.total[k] > dst[k].cap) small = k;
  if (small >= 0) {
    std::snprintf(errbuf, scfq_scratch::kErrBytes, "the %s output holds %llu bytes, the result has %llu", names[small], (unsigned long long)dst[small].cap,
                  (unsigned long long)gs.total[small]);
    put.verdict = SCFQ_EARG;
  }
  for (int k = 0; k < gs.rows; ++k) {
    if (!dst[k].want || hold_back) continue;
    if (!own_outputs) { put.out[k] = RecOut{dst[k].p, dst[k].cap}; continue; }
    if (small >= 0 || gs.total[k] == 0) continue;
    if ((put.rc = own[k].alloc(gs.total[k], stream, errbuf))) return put;
    put.out[k] = RecOut{own[k].as<uint8_t>(), gs.total[k]};
  }
  return put;
}

// the tail of a *_buffers entry point with host outputs: the copies are queued, the caller waits for the stream
inline int outputs_to_host(int n, const Dest* dst, const DevBuf* own, const uint64_t* bytes, hipStream_t stream, char* errbuf) {
  for (int k = 0; k < n; ++k)
    if (own[k].p) SCFQ_SCRATCH_CHK(errbuf, hipMemcpyAsync(dst[k].p, own[k].p, bytes[k], hipMemcpyDeviceToHost, stream));
  return SCFQ_OK;
}

// the tail of a *_files entry point: one output after the other, each in full: HBM -> two pinned buffers -> write()
inline int outputs_to_fds(int n, DevBuf* own, const uint64_t* bytes, const int* fd, scfq_scratch::ResidentInput& in1, char* errbuf) {
  bool any = false;
  for (int k = 0; k < n; ++k) any = any || own[k].p;
  if (!any) { in1.mark_clean(); return SCFQ_OK; }
  scfq_fdwrite::Pinned pinned;
  int rc = pinned.init(errbuf);
  if (rc) return finish(in1, rc);
  for (int k = 0; k < n; ++k)
    if (own[k].p && (rc = pinned.device_to_fd(own[k].as<uint8_t>(), bytes[k], fd[k], in1.stream, errbuf))) return finish(in1, rc);
  return SCFQ_OK;
}

}  // namespace scfq_reads

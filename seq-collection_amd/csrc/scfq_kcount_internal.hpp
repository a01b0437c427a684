// scfq_kcount_internal.hpp — internal: what fq-kcount (scfq_kcount.hip) lends to fq-normalize (scfq_norm.hip).  The table's kernels
// and its handle stay in scfq_kcount.hip; a pipeline that reads the slots itself gets a view of the handle, and one that already holds
// the inputs in HBM with their line indexes has them counted without a second staging or index.
#pragma once
#include "../../include/sc_fqcount.h"

#include <hip/hip_runtime.h>

namespace scfq_kcount_internal {

// the handle as a reader sees it; slots: (key, count) pairs of 16 bytes, an empty one has the key ~0
struct View {
  const void* slots = nullptr;
  uint64_t n_slots = 0;
  uint64_t ones = 0;           // count of the key that equals the empty key (32 T, plain mode)
  uint64_t distinct = 0, passes = 0;
  uint32_t k = 0, flags = 0, max_probe = 0;
};
// host only; false for a NULL handle
bool view(const scfq_kcount* t, View* out);

// one input that is resident and indexed: line_off has lines + 1 entries
struct Resident {
  const uint8_t* d = nullptr;
  uint64_t n = 0;
  const uint64_t* line_off = nullptr;
  uint64_t lines = 0;
  bool has_cr = true;
};
// scfq_kcount_buffers behind its staging and its line indexes, every kernel on `stream`; o has passed the argument checks.  The text of
// a failure is scfq_kcount_error_detail's.  The stream has been waited for when this returns SCFQ_OK.
int count_resident(const Resident* in, int n_in, const scfq_kcount_opts& o, scfq_kcount** out, scfq_kcount_summary* sum, hipStream_t stream);

}  // namespace scfq_kcount_internal

// scfq_scratch.hpp — internal: the library-owned scratch of the record pipelines (fq-dedup, fq-readstats).  Implemented in
// scfq_dedup.hip, which owns the per-device memory pool and the list of idle streams (scfq_shutdown gives both back).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace scfq_scratch {
// stream-ordered memory from the library's pool; returned with hipFreeAsync(p, stream)
int pool_alloc(void** p, size_t bytes, hipStream_t stream);
// a private non-blocking stream of the current device; hand it back once nothing is pending on it (clean) or let
// return_stream wait for it
int lease_stream(hipStream_t* s, int* dev);
void return_stream(hipStream_t s, int dev, bool clean);
// the caller's stream (scfq_set_wait_stream) is ordered before `stream`
int order_after_caller(hipStream_t stream);
}  // namespace scfq_scratch

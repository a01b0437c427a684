// scfq_overlap.hpp — internal: what fq-insert-size (scfq_insert.hip) lends to fq-merge (scfq_merge.hip).  The overlap kernel P1
// (is_overlap) and the host code in front of it stay in scfq_insert.hip, compiled once; a pipeline that needs d* per pair indexes
// its inputs and queues P1 through the three functions below and reads the scfq_overlap_rec table P1 leaves.
#pragma once
#include "../../include/sc_fqcount.h"
#include "scfq_scratch.hpp"

namespace scfq_overlap {

struct Params { uint32_t flags, min_overlap, max_mm, max_pct; };

// 64-bit words P1 adds into (the bins of the inserts and its sums): zeroed by the caller, read by fq-insert-size only
constexpr uint32_t kAccWords = SCFQ_INSERT_HIST_BINS + 12;

// the line indexes of the inputs and what follows from their line counts
struct Indexed {
  scfq_scratch::DevBuf off1, off2;      // (off2 stays empty for interleaved input)
  uint64_t lines1 = 0, lines2 = 0, reads1 = 0, reads2 = 0, pairs = 0, unpaired = 0;
  bool cr1 = true, cr2 = true;
};

// min_overlap, max_mismatches and max_mismatch_pct inside their ranges; otherwise the text goes to errbuf (kErrBytes)
bool params_in_range(const Params& p, char* errbuf);
// K5 of each input (d2 is not looked at for interleaved input); *index_ms: host clock around the synchronous index calls.
// SCFQ_EARG with text for 2^31 records or more in one input: the counts of `ix` are set then as well
int index_inputs(const uint8_t* d1, uint64_t n1, const uint8_t* d2, uint64_t n2, bool interleaved, hipStream_t stream, char* errbuf, Indexed& ix,
                 double* index_ms);
// queues P1 on `stream` behind the caller's zeroing of acc (kAccWords words): recs[p] for p in [0, ix.pairs), which is above 0
int queue_overlap(const uint8_t* d1, uint64_t n1, const uint8_t* d2, uint64_t n2, bool interleaved, const Indexed& ix, const Params& prm,
                  scfq_overlap_rec* recs, unsigned long long* acc, hipStream_t stream, char* errbuf);

}  // namespace scfq_overlap

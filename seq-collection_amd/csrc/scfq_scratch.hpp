// scfq_scratch.hpp — internal: the host side every record pipeline (fq-dedup, fq-readstats, fq-cycles) is built on.  A record
// pipeline holds the whole inflated input in HBM, builds the line index and works on records by number; what it needs for that
// is here once: the library-owned scratch (a per-device memory pool and a list of idle streams, implemented in scfq_scratch.hip,
// given back by scfq_shutdown), the resident input, the line index with its guessed size, the error macro and the stage clock.
//
// The lifetime rules, each written here and nowhere else:
//   - a stream goes back to the idle list only when nothing is pending on it            (StreamLease)
//   - pool memory is returned stream-ordered, before the lease is                        (DevBuf; ~ResidentInput)
//   - the staged file buffer is freed after the stream has drained                       (~ResidentInput)
//   - the caller's stream is ordered before ours whenever the caller hands over a device pointer   (ResidentInput::from_buffer)
#pragma once
#include "../../include/sc_fqcount.h"
#include "scfq_index_aux.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>

// A failing HIP call leaves its text in `errbuf` (a char array: each pipeline's own thread-local one, behind its
// scfq_*_error_detail) and returns SCFQ_EHIP from the enclosing function.
#define SCFQ_SCRATCH_CHK(errbuf, call)                                                                          \
  do {                                                                                                          \
    hipError_t e_ = (call);                                                                                     \
    if (e_ != hipSuccess) {                                                                                     \
      std::snprintf(errbuf, scfq_scratch::kErrBytes, "%s -> %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
      if (std::getenv("SCFQ_VERBOSE")) std::fprintf(stderr, "scfq: %s\n", errbuf);                              \
      return SCFQ_EHIP;                                                                                         \
    }                                                                                                           \
  } while (0)

namespace scfq_scratch {

constexpr size_t kErrBytes = 512;      // size of every error-text buffer handed to this header

// ---- scfq_scratch.hip: what StreamLease, DevBuf and ResidentInput are built on; nothing else calls these ----
// the current device's pool (created on first use; release threshold: keep everything)
int pool(hipMemPool_t* out, char* errbuf);
// a private non-blocking stream of the current device, from the idle list when it has one
int lease_stream(hipStream_t* s, int* dev, char* errbuf);
// back to the idle list (at most 8 per device) once nothing is pending on it: `clean` says so, otherwise this waits; a stream
// whose wait fails, or that the list has no room for, is destroyed
void return_stream(hipStream_t s, int dev, bool clean);
// the caller's stream (scfq_set_wait_stream) is ordered before `stream`
int order_after_caller(hipStream_t stream, char* errbuf);
// scfq_shutdown(): the idle streams are destroyed, the pools go back to the driver
void release_all();

struct StreamLease {
  hipStream_t s = nullptr;
  int dev = -1;
  bool clean = false;            // set by the owner once nothing is pending on s
  StreamLease() = default;
  StreamLease(const StreamLease&) = delete;
  StreamLease& operator=(const StreamLease&) = delete;
  int acquire(char* errbuf) { return lease_stream(&s, &dev, errbuf); }
  ~StreamLease() { if (s) return_stream(s, dev, clean); }
};

struct DevBuf {   // pool memory, returned stream-ordered on scope exit
  void* p = nullptr;
  hipStream_t s = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { drop(); }
  template <typename T> T* as() { return static_cast<T*>(p); }
  int alloc(size_t bytes, hipStream_t stream, char* errbuf) {
    drop();                      // (over a live pointer: the old memory goes back first, on the stream it was taken on)
    s = stream;
    hipMemPool_t mp;
    const int rc = pool(&mp, errbuf);
    if (rc) return rc;
    SCFQ_SCRATCH_CHK(errbuf, hipMallocFromPoolAsync(&p, std::max<size_t>(bytes, 16), mp, stream));
    return SCFQ_OK;
  }
  // takes over pool memory that is returned on `stream`
  void adopt(void* q, hipStream_t stream) { drop(); p = q; s = stream; }
  void* release() { void* q = p; p = nullptr; return q; }
  void drop() { if (p) (void)hipFreeAsync(p, s); p = nullptr; }
};

// What an entry point does before and after its *_device function: the input in device memory and the call's private stream.
struct ResidentInput {
  const uint8_t* d_in = nullptr;
  uint64_t n = 0;
  hipStream_t stream = nullptr;

  ResidentInput() = default;
  ResidentInput(const ResidentInput&) = delete;
  ResidentInput& operator=(const ResidentInput&) = delete;

  // ptr: host or device memory.  after_caller: the caller hands over device memory (the input, or a destination), so its
  // stream (scfq_set_wait_stream) comes before ours.  A host buffer is copied into pool memory and the copy waited for.
  int from_buffer(const void* ptr, uint64_t bytes, bool is_device, bool after_caller, char* errbuf) {
    int rc = lease_.acquire(errbuf);
    if (rc) return rc;
    stream = lease_.s;
    d_in = static_cast<const uint8_t*>(ptr);
    n = bytes;
    if (after_caller && (rc = order_after_caller(stream, errbuf))) return rc;
    if (!is_device && n) {
      if ((rc = staged_.alloc(n, stream, errbuf))) return rc;
      SCFQ_SCRATCH_CHK(errbuf, hipMemcpyAsync(staged_.p, ptr, n, hipMemcpyHostToDevice, stream));
      SCFQ_SCRATCH_CHK(errbuf, hipStreamSynchronize(stream));
      d_in = staged_.as<uint8_t>();
    }
    return SCFQ_OK;
  }
  // the whole (inflated) file into HBM (scfq_stage_file: its text is scfq_last_error_detail's)
  int from_file(const char* path, const scfq_opts* opts, char* errbuf) {
    int rc = scfq_stage_file(path, opts, &file_.p, &n);
    if (rc) return rc;
    d_in = static_cast<const uint8_t*>(file_.p);
    if ((rc = lease_.acquire(errbuf))) return rc;
    stream = lease_.s;
    return SCFQ_OK;
  }
  // by the caller, after a hipStreamSynchronize(stream) behind which it put nothing but returns of pool memory
  void mark_clean() { lease_.clean = true; }

 private:
  // destroyed last to first: pool memory back, stream-ordered; then the stream drained (or known to be) and returned; only
  // then the staged file
  struct File { void* p = nullptr; ~File() { if (p) (void)hipFree(p); } } file_;
  StreamLease lease_;
  DevBuf staged_;
};

// The line index of the resident input, in ONE pass (count and offsets together): its size is guessed first — a FASTQ line is
// rarely shorter than 24 bytes on average — and only a wrong guess costs a second pass with the exact size.
// per_round(cap, &aux): called in each round, behind line_off's allocation, with the round's capacity in lines; it may size
// buffers of its own by it and set aux to what the index pass is to fill on its way (scfq_index_aux.hpp).  It returns an SCFQ
// code.  In a second round the first one's line_off has been returned already; per_round returns its own before it allocates.
// has_cr: the input may hold "\r\n" line ends.
template <typename PerRound>
int build_line_index(const uint8_t* d_in, uint64_t n, hipStream_t stream, char* errbuf, DevBuf& line_off, uint64_t* lines, bool* has_cr,
                     PerRound per_round) {
  uint32_t flags = 1;
  uint64_t cap = n / 24 + 1024;
  for (int round = 0; round < 2; ++round) {
    int rc = line_off.alloc(cap * 8, stream, errbuf);
    if (rc) return rc;
    scfq_index_aux* aux = nullptr;
    if ((rc = per_round(cap, &aux))) return rc;
    SCFQ_SCRATCH_CHK(errbuf, hipStreamSynchronize(stream));       // the index works on the library's own stream
    if ((rc = scfq_index_lines_ex2(d_in, n, line_off.as<uint64_t>(), cap, lines, &flags, aux))) return rc;
    if (*lines + 1 <= cap) break;
    // the guess was too small (lines shorter than 24 bytes on average): once more with the exact size
    line_off.drop();
    cap = *lines + 1;
  }
  *has_cr = (flags & 1u) != 0;
  return SCFQ_OK;
}
inline int build_line_index(const uint8_t* d_in, uint64_t n, hipStream_t stream, char* errbuf, DevBuf& line_off, uint64_t* lines, bool* has_cr) {
  return build_line_index(d_in, n, stream, errbuf, line_off, lines, has_cr, [](uint64_t, scfq_index_aux**) { return (int)SCFQ_OK; });
}

// HIP-event brackets around the stages of a pipeline, for its scfq_debug_*_stages.  `enabled`: the pipeline's environment
// switch, read once per process at the call site.
struct StageClock {
  bool on;
  hipStream_t s;
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  bool set[5] = {false, false, false, false, false};
  StageClock(hipStream_t stream, bool enabled) : on(enabled), s(stream) {
    if (on) for (auto& e : ev) if (hipEventCreate(&e) != hipSuccess) { on = false; break; }
  }
  StageClock(const StageClock&) = delete;
  StageClock& operator=(const StageClock&) = delete;
  ~StageClock() { for (auto e : ev) if (e) (void)hipEventDestroy(e); }
  void mark(int k) { if (on && hipEventRecord(ev[k], s) == hipSuccess) set[k] = true; }
  double between(int a, int b) {
    float ms = 0;
    return (on && set[a] && set[b] && hipEventElapsedTime(&ms, ev[a], ev[b]) == hipSuccess) ? (double)ms : 0.0;
  }
};
inline bool env_switch(const char* name) { const char* e = std::getenv(name); return e && std::atoi(e) != 0; }

// the per-thread stage times behind scfq_debug_read_stats_stages / scfq_debug_cycles_stages
inline int copy_stage_ms(const double (&stage_ms)[4], double* ms, uint32_t cap) {
  for (uint32_t k = 0; ms && k < cap && k < 4; ++k) ms[k] = stage_ms[k];
  return 4;
}

// an out-struct of the C ABI at the start of a call: struct_size kept, the rest zero, the ABI version stamped where there is one
template <typename T> auto stamp_abi(T* out, int) -> decltype((void)(out->abi_version = 0)) { out->abi_version = SCFQ_ABI_VERSION; }
template <typename T> void stamp_abi(T*, long) {}
template <typename T> void clear_keep_size(T* out) {
  const auto keep = out->struct_size;
  std::memset(out, 0, sizeof *out);
  out->struct_size = keep;
  stamp_abi(out, 0);
}

}  // namespace scfq_scratch

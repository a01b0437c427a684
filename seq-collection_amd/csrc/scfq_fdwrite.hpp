// scfq_fdwrite.hpp — internal: the one writer of the commands whose product is reads (fq-dedup, fq-merge): a result in device
// memory goes to a file descriptor through two pinned buffers, the copy of chunk k+1 overlapping the write() of chunk k.
#pragma once
#include "../../include/sc_fqcount.h"
#include "scfq_scratch.hpp"

#include <hip/hip_runtime.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstring>

namespace scfq_fdwrite {

inline int write_all(int fd, const uint8_t* p, uint64_t n, char* errbuf) {
  while (n) {
    ssize_t w = write(fd, p, (size_t)std::min<uint64_t>(n, 1u << 30));
    if (w < 0 && errno == EINTR) continue;
    if (w < 0) {       // only a vanished reader is the quiet case (sc.nim:304); a full disk or an I/O error is an error
      const int e = errno;
      std::snprintf(errbuf, scfq_scratch::kErrBytes, "write: %s", std::strerror(e));
      return e == EPIPE ? SCFQ_EPIPE : SCFQ_EIO;
    }
    p += w;
    n -= (uint64_t)w;
  }
  return SCFQ_OK;
}

// the two pinned buffers and their events: one set serves every output of a call
struct Pinned {
  static constexpr uint64_t kChunk = 32ull << 20;
  uint8_t* pin[2] = {nullptr, nullptr};
  hipEvent_t ev[2] = {nullptr, nullptr};
  Pinned() = default;
  Pinned(const Pinned&) = delete;
  Pinned& operator=(const Pinned&) = delete;
  ~Pinned() { for (int b = 0; b < 2; ++b) { if (pin[b]) (void)hipHostFree(pin[b]); if (ev[b]) (void)hipEventDestroy(ev[b]); } }
  int init(char* errbuf) {
    for (int b = 0; b < 2; ++b) { SCFQ_SCRATCH_CHK(errbuf, hipHostMalloc(&pin[b], kChunk, hipHostMallocDefault)); SCFQ_SCRATCH_CHK(errbuf, hipEventCreateWithFlags(&ev[b], hipEventDisableTiming)); }
    return SCFQ_OK;
  }
  // HBM -> two pinned buffers -> write(): the copy of chunk k+1 overlaps the write of chunk k.  The last chunk is waited for by its
  // event, not by the stream: the lease waits
  int device_to_fd(const uint8_t* d_out, uint64_t nb, int fd, hipStream_t stream, char* errbuf) {
    const uint64_t n_chunks = (nb + kChunk - 1) / kChunk;
    auto issue = [&](uint64_t k) -> hipError_t {
      const uint64_t lo = k * kChunk, len = std::min(kChunk, nb - lo);
      hipError_t e = hipMemcpyAsync(pin[k & 1], d_out + lo, len, hipMemcpyDeviceToHost, stream);
      return e != hipSuccess ? e : hipEventRecord(ev[k & 1], stream);
    };
    if (!n_chunks) return SCFQ_OK;
    SCFQ_SCRATCH_CHK(errbuf, issue(0));
    for (uint64_t k = 0; k < n_chunks; ++k) {
      SCFQ_SCRATCH_CHK(errbuf, hipEventSynchronize(ev[k & 1]));
      if (k + 1 < n_chunks) SCFQ_SCRATCH_CHK(errbuf, issue(k + 1));
      const uint64_t lo = k * kChunk, len = std::min(kChunk, nb - lo);
      const int rc = write_all(fd, pin[k & 1], len, errbuf);
      if (rc) {      // chunk k+1 is on its way into the other buffer: it lands before the caller may free that buffer (~Pinned)
        if (k + 1 < n_chunks) (void)hipEventSynchronize(ev[(k + 1) & 1]);
        return rc;
      }
    }
    return SCFQ_OK;
  }
};

}  // namespace scfq_fdwrite

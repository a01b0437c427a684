// scfq_copy_text.hpp — internal: the end of every scfq_format_*.  No HIP here: the host-only headers include it as well.
#pragma once
#include <cstdint>
#include <cstring>

namespace scfq_reads {

// as much of the m bytes of text as fits into buf[cap], always terminated; the full length comes back, so a call without a buffer
// is the sizing call
inline int copy_text(const char* text, int m, char* buf, uint64_t cap) {
  if (buf && cap) {
    const uint64_t ncopy = ((uint64_t)m < cap - 1) ? (uint64_t)m : cap - 1;
    std::memcpy(buf, text, ncopy);
    buf[ncopy] = 0;
  }
  return m;
}

}  // namespace scfq_reads

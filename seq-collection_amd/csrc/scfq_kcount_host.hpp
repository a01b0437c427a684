// scfq_kcount_host.hpp — internal: the parts of fq-kcount (scfq_kcount.hip) that need no device: the hash, the reverse complement of a
// 64-bit key, the argument checks (all of them come before the first HIP call), the sizing rules and the row formatter.
#pragma once
#include "../../include/sc_fqcount.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

#if defined(__HIPCC__)
#define SCFQ_KC_HD __host__ __device__ __forceinline__
#else
#define SCFQ_KC_HD inline
#endif

namespace scfq_kcount_host {

constexpr uint64_t kEmpty = ~0ull;                 // a slot without a key; the k-mer of 32 T (plain mode) has a counter of its own
constexpr uint32_t kMinBits = 10, kMaxBits = 32;   // of opts->table_bits
constexpr uint32_t kAutoMaxBits = 30;              // the first size of automatic sizing
constexpr uint32_t kAutoProbe = 512;               // slots a window probes: automatic sizing
constexpr uint32_t kFixedProbe = 4096;             //                        table_bits given: min(slots, this)
constexpr uint64_t kMaxBins = 1ull << 20;

SCFQ_KC_HD uint64_t mix64(uint64_t x) {            // (MurmurHash3's finalizer, as fq-screen's index)
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

SCFQ_KC_HD uint64_t key_mask(uint32_t k) { return k >= 32 ? ~0ull : (1ull << (2 * k)) - 1ull; }

// reverse complement of the k letters of key
SCFQ_KC_HD uint64_t revcomp(uint64_t key, uint32_t k) {
  uint64_t x = ~key;                                                        // complement: 3 - code
  x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
  x = ((x >> 4) & 0x0f0f0f0f0f0f0f0full) | ((x & 0x0f0f0f0f0f0f0f0full) << 4);
  x = ((x >> 8) & 0x00ff00ff00ff00ffull) | ((x & 0x00ff00ff00ff00ffull) << 8);
  x = ((x >> 16) & 0x0000ffff0000ffffull) | ((x & 0x0000ffff0000ffffull) << 16);
  x = (x >> 32) | (x << 32);
  return x >> (64 - 2 * k);                                                 // (1 <= k <= 32)
}

inline bool k_ok(uint32_t k) { return k >= SCFQ_KCOUNT_MIN_K && k <= SCFQ_KCOUNT_MAX_K; }

// SCFQ_OK, or SCFQ_EARG with the text in err
inline int check_opts(const scfq_kcount_opts* o, const scfq_kcount_summary* sum, bool have_out, char* err, size_t cap) {
  if (!o) { std::snprintf(err, cap, "opts is NULL"); return SCFQ_EARG; }
  if (o->struct_size != sizeof(scfq_kcount_opts)) {
    std::snprintf(err, cap, "opts->struct_size is %llu, not %llu", (unsigned long long)o->struct_size, (unsigned long long)sizeof(scfq_kcount_opts));
    return SCFQ_EARG;
  }
  if (sum && sum->struct_size != sizeof(scfq_kcount_summary)) {
    std::snprintf(err, cap, "sum->struct_size is %llu, not %llu", (unsigned long long)sum->struct_size, (unsigned long long)sizeof(scfq_kcount_summary));
    return SCFQ_EARG;
  }
  if (!sum && !have_out) { std::snprintf(err, cap, "neither a table nor a summary is asked for"); return SCFQ_EARG; }
  if (!k_ok(o->k)) {
    std::snprintf(err, cap, "k = %u is outside %u .. %u", o->k, (unsigned)SCFQ_KCOUNT_MIN_K, (unsigned)SCFQ_KCOUNT_MAX_K);
    return SCFQ_EARG;
  }
  if (o->flags & ~(uint32_t)SCFQ_KCOUNT_CANONICAL) {
    std::snprintf(err, cap, "unknown flag bits 0x%x", o->flags & ~(uint32_t)SCFQ_KCOUNT_CANONICAL);
    return SCFQ_EARG;
  }
  if (o->table_bits && (o->table_bits < kMinBits || o->table_bits > kMaxBits)) {
    std::snprintf(err, cap, "table_bits = %u is neither 0 nor in %u .. %u", o->table_bits, kMinBits, kMaxBits);
    return SCFQ_EARG;
  }
  if (o->reserved) { std::snprintf(err, cap, "reserved is %u, not 0", o->reserved); return SCFQ_EARG; }
  return SCFQ_OK;
}

// automatic sizing: log2 of the first number of slots for `bytes` of input; start_bits: SCFQ_KCOUNT_START_BITS, 0 when not set
inline uint32_t auto_bits(uint64_t bytes, uint32_t start_bits) {
  uint32_t bits = kMinBits;
  while (bits < kAutoMaxBits && (1ull << bits) < 2 * bytes) ++bits;
  if (start_bits >= kMinBits && start_bits < bits) bits = start_bits;
  return bits;
}

inline uint32_t probe_bound(uint64_t slots, bool fixed, uint32_t env_probe) {
  if (env_probe) return env_probe;
  return fixed ? (uint32_t)(slots < kFixedProbe ? slots : kFixedProbe) : kAutoProbe;
}

inline uint32_t env_u32(const char* name) {
  const char* e = std::getenv(name);
  const long v = e && *e ? std::atol(e) : 0;
  return v > 0 ? (uint32_t)v : 0;
}

inline int format_tsv(uint32_t k, uint64_t key, uint64_t count, char* buf, uint64_t cap) {
  if (!k_ok(k) || (key & ~key_mask(k))) return SCFQ_EARG;
  char row[SCFQ_KCOUNT_MAX_K + 24];
  for (uint32_t i = 0; i < k; ++i) row[i] = "ACGT"[(key >> (2 * (k - 1 - i))) & 3u];
  const int len = (int)k + std::snprintf(row + k, sizeof row - k, "\t%llu", (unsigned long long)count);
  if (buf && cap) {
    const uint64_t put = (uint64_t)len < cap - 1 ? (uint64_t)len : cap - 1;
    std::memcpy(buf, row, put);
    buf[put] = '\0';
  }
  return len;
}

}  // namespace scfq_kcount_host

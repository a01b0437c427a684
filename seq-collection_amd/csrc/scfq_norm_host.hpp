// scfq_norm_host.hpp — internal: the parts of fq-normalize (scfq_norm.hip) that need no device: the options with their defaults, the
// argument checks (all of them come before the first HIP call), the rule of a unit in plain C++ and the formatters.
#pragma once
#include "../../include/sc_fqcount.h"

#include "scfq_kcount_host.hpp"

#include <cstdio>
#include <cstring>

namespace scfq_norm_host {

struct Params {
  uint32_t flags = 0, k = 0, table_flags = 0, table_bits = 0, target = 0, min_depth = 0, weak_below = 2;
  uint64_t seed = 0;
};

// the classes of a unit
enum : uint32_t { kKept = 0, kNoKmers = 1, kLow = 2, kHigh = 3 };

constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;

// kmers and depth of the unit's mates (one mate: kmers2 = 0).  *d: D, when the unit is not kNoKmers
SCFQ_KC_HD uint32_t classify(uint32_t kmers1, uint32_t depth1, uint32_t kmers2, uint32_t depth2, uint64_t u, uint32_t target, uint32_t min_depth,
                             uint64_t seed, uint32_t* d) {
  if (!kmers1 && !kmers2) { *d = 0; return kNoKmers; }
  const uint32_t D = !kmers2 ? depth1 : (!kmers1 ? depth2 : (depth1 < depth2 ? depth1 : depth2));
  *d = D;
  if (D < min_depth) return kLow;
  if (target && D > target) {
    const uint64_t r = scfq_kcount_host::mix64(seed ^ (u * kGolden)) >> 32;
    if (((r * D) >> 32) >= target) return kHigh;
  }
  return kKept;
}

// SCFQ_OK with p filled, or SCFQ_EARG with the text in err.  have_table / table_k: the handle's; second: a second input (or path);
// out2: a second output; have_hist: hist_host is given
inline int check_args(const scfq_norm_opts* o, const scfq_norm_stats* st, bool have_table, uint32_t table_k, bool first, bool second, bool out2,
                      bool have_hist, uint64_t bins, Params& p, char* err, size_t cap) {
  if (!st) { std::snprintf(err, cap, "stats is NULL"); return SCFQ_EARG; }
  if (st->struct_size != sizeof(scfq_norm_stats)) {
    std::snprintf(err, cap, "stats->struct_size is %llu, not %llu", (unsigned long long)st->struct_size, (unsigned long long)sizeof(scfq_norm_stats));
    return SCFQ_EARG;
  }
  p = Params();
  if (o) {
    if (o->struct_size != sizeof(scfq_norm_opts)) {
      std::snprintf(err, cap, "opts->struct_size is %llu, not %llu", (unsigned long long)o->struct_size, (unsigned long long)sizeof(scfq_norm_opts));
      return SCFQ_EARG;
    }
    p.flags = o->flags; p.k = o->k; p.table_flags = o->table_flags; p.table_bits = o->table_bits;
    p.target = o->target; p.min_depth = o->min_depth; p.weak_below = o->weak_below; p.seed = o->seed;
    const uint32_t known = SCFQ_NORM_INTERLEAVED | SCFQ_NORM_KEEP_NO_KMERS;
    if (p.flags & ~known) { std::snprintf(err, cap, "unknown flag bits 0x%x", p.flags & ~known); return SCFQ_EARG; }
    if (o->reserved) { std::snprintf(err, cap, "reserved is %u, not 0", o->reserved); return SCFQ_EARG; }
  }
  if (have_hist ? (bins < 2 || bins > SCFQ_NORM_MAX_BINS) : bins != 0) {
    std::snprintf(err, cap, have_hist ? "bins = %llu is outside 2 .. %llu" : "bins = %llu without a histogram (0 .. %llu there)", (unsigned long long)bins,
                  have_hist ? (unsigned long long)SCFQ_NORM_MAX_BINS : 0ull);
    return SCFQ_EARG;
  }
  if (second && !first) { std::snprintf(err, cap, "a second input without a first"); return SCFQ_EARG; }
  const bool interleaved = (p.flags & SCFQ_NORM_INTERLEAVED) != 0;
  if (interleaved && second) { std::snprintf(err, cap, "interleaved input takes no second input"); return SCFQ_EARG; }
  if (out2 && (interleaved || !second)) { std::snprintf(err, cap, "one input has no second output (out2)"); return SCFQ_EARG; }
  if (have_table) {
    if (p.k && p.k != table_k) { std::snprintf(err, cap, "k = %u, the table was counted with k = %u", p.k, table_k); return SCFQ_EARG; }
  } else {
    scfq_kcount_opts ko;
    ko.struct_size = sizeof ko; ko.k = p.k; ko.flags = p.table_flags; ko.table_bits = p.table_bits; ko.reserved = 0;
    char why[256] = "";
    if (scfq_kcount_host::check_opts(&ko, nullptr, true, why, sizeof why)) {
      std::snprintf(err, cap, "without a table the inputs are counted first: %s", why);
      return SCFQ_EARG;
    }
  }
  return SCFQ_OK;
}

inline int put_row(const char* row, int len, char* buf, uint64_t cap) {
  if (buf && cap) {
    const uint64_t put = (uint64_t)len < cap - 1 ? (uint64_t)len : cap - 1;
    std::memcpy(buf, row, put);
    buf[put] = '\0';
  }
  return len;
}

inline int format_row(const scfq_norm_stats* s, int header, char* buf, uint64_t cap) {
  if (header) {
    static const char names[] = "units_in\tunits_out\treads_in\treads_out\tdropped_no_kmers\tdropped_low\tdropped_high\tbases_in\tbases_out\tkmers\tskipped\t"
                                "weak_kmers\tabsent_kmers\tk\ttarget\tmin_depth";
    return put_row(names, (int)sizeof names - 1, buf, cap);
  }
  if (!s || s->struct_size != sizeof(scfq_norm_stats)) return SCFQ_EARG;
  char row[16 * 21 + 1];
  const uint64_t v[16] = {s->units_in, s->units_out, s->reads_in, s->reads_out, s->dropped_no_kmers, s->dropped_low, s->dropped_high, s->bases_in,
                          s->bases_out, s->kmers, s->skipped, s->weak_kmers, s->absent_kmers, s->k, s->target, s->min_depth};
  int len = 0;
  for (int i = 0; i < 16; ++i) len += std::snprintf(row + len, sizeof row - len, i ? "\t%llu" : "%llu", (unsigned long long)v[i]);
  return put_row(row, len, buf, cap);
}

inline int format_hist(uint64_t depth, uint64_t in, uint64_t out, char* buf, uint64_t cap) {
  char row[3 * 21 + 1];
  const int len = std::snprintf(row, sizeof row, "%llu\t%llu\t%llu", (unsigned long long)depth, (unsigned long long)in, (unsigned long long)out);
  return put_row(row, len, buf, cap);
}

}  // namespace scfq_norm_host

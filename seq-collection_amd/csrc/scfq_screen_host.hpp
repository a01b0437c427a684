// scfq_screen_host.hpp — internal: the host-only part of `sc fq-screen` (scfq_screen.hip): S0, the references parsed into one byte
// string, the names' rules and the report row.  No HIP here: the file compiles on its own into a host program (a sanitizer build).
#pragma once
#include "../../include/sc_fqcount.h"

#include "scfq_copy_text.hpp"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace scfq_screen_host {

constexpr size_t kErrBytes = 512;
constexpr uint8_t kSeparator = 0;        // between contigs and references: no base, so no window crosses it

struct RefInfo {
  std::string name;
  uint64_t contigs = 0, bases = 0, windows = 0, kmers = 0, distinct = 0, shared = 0;
};

// the references as S1 reads them: text = contig, separator, contig, ... ; ref_begin[r] .. ref_begin[r + 1]: reference r's stretch
struct Parsed {
  std::vector<uint8_t> text;
  uint64_t ref_begin[SCFQ_SCREEN_MAX_REFS + 1] = {};
  uint64_t bases = 0, windows = 0;
};

inline bool name_ok(const char* name, uint32_t r, char* err) {
  if (!name) { std::snprintf(err, kErrBytes, "reference %u has no name", r); return false; }
  const size_t len = std::strlen(name);
  if (len < 1 || len > 63) { std::snprintf(err, kErrBytes, "the name of reference %u has %zu bytes: 1 .. 63 are allowed", r, len); return false; }
  for (size_t i = 0; i < len; ++i)
    if (name[i] == '\t' || name[i] == '\n' || name[i] == ':') {
      std::snprintf(err, kErrBytes, "the name of reference %u holds a tab, a newline or a ':'", r);
      return false;
    }
  return true;
}

// S0 for one reference, appended to p.  A contig's sequence bytes follow each other whatever the line ends were; a header line puts
// one separator behind the contig before it.  kmers: by a run length of A C G T bytes, as S1 counts them
inline bool append_reference(const uint8_t* t, uint64_t n, uint32_t k, uint32_t r, RefInfo& info, Parsed& p, char* err) {
  p.ref_begin[r] = p.text.size();
  uint64_t contig_len = 0, run = 0;
  bool open = false;                      // a contig has begun (a header line, or bases before the first one)
  auto close_contig = [&] {
    if (!open) return;
    info.contigs += 1;
    if (contig_len >= k) info.windows += contig_len - k + 1;
    p.text.push_back(kSeparator);
    contig_len = run = 0;
    open = false;
  };
  uint64_t i = 0;
  while (i < n) {
    uint64_t e = i;
    while (e < n && t[e] != '\n') ++e;
    if (t[i] == '>' ) {                   // (i < e or not: an empty line has no first byte and is a sequence line)
      if (i < e) { close_contig(); open = true; i = e + 1; continue; }
    }
    for (uint64_t j = i; j < e; ++j) {
      uint8_t b = t[j];
      if (b < 0x21 || b > 0x7E) continue;
      if (b >= 'a' && b <= 'z') b = (uint8_t)(b - 32);
      open = true;
      p.text.push_back(b);
      ++contig_len;
      ++info.bases;
      run = (b == 'A' || b == 'C' || b == 'G' || b == 'T') ? run + 1 : 0;
      if (run >= k) ++info.kmers;
      if (p.bases + info.bases > SCFQ_SCREEN_MAX_REF_BASES) {
        std::snprintf(err, kErrBytes, "the references hold more than %llu sequence bytes (reference %u)", (unsigned long long)SCFQ_SCREEN_MAX_REF_BASES, r);
        return false;
      }
    }
    i = e + 1;
  }
  close_contig();
  if (info.bases == 0) { std::snprintf(err, kErrBytes, "reference %u (%s) is empty: it has no sequence byte", r, info.name.c_str()); return false; }
  p.bases += info.bases;
  p.windows += info.windows;
  p.ref_begin[r + 1] = p.text.size();
  return true;
}

// every argument rule of scfq_screen_index_buffers that needs no device, then S0
inline bool parse_references(const scfq_screen_ref* refs, uint32_t n_refs, uint32_t k, std::vector<RefInfo>& infos, Parsed& p, char* err) {
  if (k < 8 || k > SCFQ_SCREEN_MAX_K) { std::snprintf(err, kErrBytes, "k = %u is not in 8 .. %d", k, SCFQ_SCREEN_MAX_K); return false; }
  if (!refs || n_refs < 1 || n_refs > SCFQ_SCREEN_MAX_REFS) { std::snprintf(err, kErrBytes, "%u references: 1 .. %d are allowed", refs ? n_refs : 0u, SCFQ_SCREEN_MAX_REFS); return false; }
  infos.assign(n_refs, RefInfo());
  for (uint32_t r = 0; r < n_refs; ++r) {
    if (!name_ok(refs[r].name, r, err)) return false;
    for (uint32_t q = 0; q < r; ++q)
      if (infos[q].name == refs[r].name) { std::snprintf(err, kErrBytes, "references %u and %u are both named %s", q, r, refs[r].name); return false; }
    infos[r].name = refs[r].name;
    if (!refs[r].text && refs[r].n) { std::snprintf(err, kErrBytes, "reference %u (%s) has no text", r, refs[r].name); return false; }
  }
  for (uint32_t r = 0; r < n_refs; ++r)
    if (!append_reference(static_cast<const uint8_t*>(refs[r].text), refs[r].n, k, r, infos[r], p, err)) return false;
  return true;
}

// slots of the table: a power of two, at least 2 x windows and 1024; forced_bits > 0: 2^forced_bits, which has to be more than `windows`
// (the keys are at most as many as the windows, so one slot at the least stays empty and every probe loop ends)
inline bool pick_slots(uint64_t windows, int forced_bits, uint64_t* slots, char* err) {
  if (forced_bits > 0) {
    if (forced_bits > 30 || (1ull << forced_bits) <= windows) {
      std::snprintf(err, kErrBytes, "SCFQ_SCREEN_TABLE_BITS=%d: 2^%d slots do not hold the %llu windows of the references and an empty slot", forced_bits,
                    forced_bits, (unsigned long long)windows);
      return false;
    }
    *slots = 1ull << forced_bits;
    return true;
  }
  uint64_t s = 1024;
  while (s < 2 * windows) s <<= 1;
  *slots = s;
  return true;
}

// the report row (include/sc_fqcount.h: scfq_format_screen_row_tsv)
inline int format_row(const scfq_screen_stats* s, const std::vector<RefInfo>& infos, uint32_t k, uint32_t r, char* buf, uint64_t cap) {
  if (!s || r > infos.size() || s->n_refs != infos.size() || s->k != k) return SCFQ_EARG;
  const bool all = r == infos.size();
  uint64_t bases = 0, kmers = 0;
  if (all) for (const RefInfo& i : infos) { bases += i.bases; kmers += i.kmers; }
  else { bases = infos[r].bases; kmers = infos[r].kmers; }
  const uint64_t reads = all ? s->matched_reads : s->ref_reads[r];
  const uint64_t pct = s->reads_in ? (uint64_t)(((unsigned __int128)reads * 10000u) / s->reads_in) : 0;
  char tmp[512];
  const int m = std::snprintf(tmp, sizeof tmp, "%s\t%llu\t%llu\t%llu\t%llu\t%llu.%02llu\t%llu\t%llu\t%llu", all ? "*" : infos[r].name.c_str(),
                              (unsigned long long)bases, (unsigned long long)kmers, (unsigned long long)s->reads_in, (unsigned long long)reads,
                              (unsigned long long)(pct / 100), (unsigned long long)(pct % 100),
                              (unsigned long long)(all ? s->matched_reads - s->multi_reads : s->ref_only_reads[r]),
                              (unsigned long long)(all ? s->multi_reads : s->ref_best_reads[r]),
                              (unsigned long long)(all ? s->hit_kmers : s->ref_kmer_hits[r]));
  return scfq_reads::copy_text(tmp, m, buf, cap);
}

}  // namespace scfq_screen_host

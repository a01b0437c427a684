// scfq_demux_host.hpp — internal: the host-only part of `sc fq-demux` (scfq_demux.hip): the sheet's rules, its packed form as X1
// reads it, the option rules, the names of the output files and the report row.  No HIP here: the file compiles on its own into a
// host program (a sanitizer build).
#pragma once
#include "../../include/sc_fqcount.h"

#include "scfq_copy_text.hpp"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace scfq_demux_host {

constexpr size_t kErrBytes = 512;

// a letter's 2-bit code (bits 1 and 2 of the byte: A 0, C 1, T 2, G 3); letter i of a barcode sits at bits 2i and 2i + 1 of its word
inline uint64_t code_of(uint8_t b) { return (b >> 1) & 3u; }

struct Sheet {
  std::vector<std::string> name, bc1, bc2;
  std::vector<uint64_t> codes;           // 2 words per sample: barcode1's, barcode2's (0 without one)
  std::vector<uint32_t> lens;            // m1 | m2 << 8
  bool dual = false;
  uint32_t n() const { return (uint32_t)name.size(); }
};

inline bool name_ok(const char* name, uint32_t s, char* err) {
  if (!name) { std::snprintf(err, kErrBytes, "sample %u has no name", s); return false; }
  const size_t len = std::strlen(name);
  if (len < 1 || len > 63) { std::snprintf(err, kErrBytes, "the name of sample %u has %zu bytes: 1 .. 63 are allowed", s, len); return false; }
  for (size_t i = 0; i < len; ++i) {
    const char c = name[i];
    const bool ok = (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') || (c >= '0' && c <= '9') || c == '.' || c == '_' || c == '-';
    if (!ok) { std::snprintf(err, kErrBytes, "the name of sample %u holds a byte other than A-Z a-z 0-9 . _ -", s); return false; }
  }
  if (name[0] == '.') { std::snprintf(err, kErrBytes, "the name of sample %u starts with '.'", s); return false; }
  if (std::strcmp(name, "undetermined") == 0) { std::snprintf(err, kErrBytes, "sample %u is named undetermined, which names the units without a sample", s); return false; }
  return true;
}

inline bool barcode_ok(const char* bc, uint32_t s, int which, char* err) {
  if (!bc) { std::snprintf(err, kErrBytes, "sample %u has no barcode%d", s, which); return false; }
  const size_t len = std::strlen(bc);
  if (len < 1 || len > SCFQ_DEMUX_MAX_BARCODE) {
    std::snprintf(err, kErrBytes, "barcode%d of sample %u has %zu letters: 1 .. %d are allowed", which, s, len, SCFQ_DEMUX_MAX_BARCODE);
    return false;
  }
  for (size_t i = 0; i < len; ++i)
    if (bc[i] != 'A' && bc[i] != 'C' && bc[i] != 'G' && bc[i] != 'T') {
      std::snprintf(err, kErrBytes, "barcode%d of sample %u holds a byte that is not A, C, G or T", which, s);
      return false;
    }
  return true;
}

inline uint64_t pack(const std::string& bc) {
  uint64_t w = 0;
  for (size_t i = 0; i < bc.size(); ++i) w |= code_of((uint8_t)bc[i]) << (2 * i);
  return w;
}

// every rule of scfq_demux_sheet_new
inline bool build_sheet(const scfq_demux_sample* samples, uint32_t n, Sheet& sh, char* err) {
  if (!samples || n < 1 || n > SCFQ_DEMUX_MAX_SAMPLES) { std::snprintf(err, kErrBytes, "%u samples: 1 .. %d are allowed", samples ? n : 0u, SCFQ_DEMUX_MAX_SAMPLES); return false; }
  sh.dual = samples[0].barcode2 != nullptr;
  for (uint32_t s = 0; s < n; ++s) {
    if (!name_ok(samples[s].name, s, err) || !barcode_ok(samples[s].barcode1, s, 1, err)) return false;
    if ((samples[s].barcode2 != nullptr) != sh.dual) {
      std::snprintf(err, kErrBytes, "sample %u has %s second barcode, sample 0 has %s: all samples have one or none has", s, sh.dual ? "no" : "a", sh.dual ? "one" : "none");
      return false;
    }
    if (sh.dual && !barcode_ok(samples[s].barcode2, s, 2, err)) return false;
    sh.name.push_back(samples[s].name);
    sh.bc1.push_back(samples[s].barcode1);
    sh.bc2.push_back(sh.dual ? samples[s].barcode2 : "");
    for (uint32_t q = 0; q < s; ++q) {
      if (sh.name[q] == sh.name[s]) { std::snprintf(err, kErrBytes, "samples %u and %u are both named %s", q, s, sh.name[s].c_str()); return false; }
      if (sh.bc1[q] == sh.bc1[s] && sh.bc2[q] == sh.bc2[s]) {
        std::snprintf(err, kErrBytes, "samples %u and %u have the same barcode%s %s%s%s", q, s, sh.dual ? "s" : "", sh.bc1[s].c_str(), sh.dual ? "+" : "", sh.bc2[s].c_str());
        return false;
      }
    }
    sh.codes.push_back(pack(sh.bc1[s]));
    sh.codes.push_back(pack(sh.bc2[s]));
    sh.lens.push_back((uint32_t)sh.bc1[s].size() | ((uint32_t)sh.bc2[s].size() << 8));
  }
  return true;
}

struct Params { uint32_t flags, mismatches; };

// the option rules of scfq_demux_buffers / scfq_demux_files that need no device; `paired`: two inputs or an interleaved one
inline bool params_ok(const scfq_demux_opts* opts, Params& p, char* err) {
  p = Params{0, 1};
  if (!opts) return true;
  p = Params{opts->flags, opts->mismatches};
  const uint32_t known = SCFQ_DEMUX_INTERLEAVED | SCFQ_DEMUX_HEADER | SCFQ_DEMUX_KEEP_BARCODE;
  if (p.flags & ~known) { std::snprintf(err, kErrBytes, "unknown flag bits 0x%x", p.flags & ~known); return false; }
  if (p.mismatches > 3) { std::snprintf(err, kErrBytes, "mismatches %u is not in 0 .. 3", p.mismatches); return false; }
  if (opts->reserved[0] || opts->reserved[1]) { std::snprintf(err, kErrBytes, "a reserved word is not 0"); return false; }
  return true;
}
inline bool sheet_fits_input(const Sheet& sh, const Params& p, bool paired, char* err) {
  if (sh.dual && !paired && !(p.flags & SCFQ_DEMUX_HEADER)) {
    std::snprintf(err, kErrBytes, "a sheet with second barcodes needs paired input in inline mode: the second barcode is read from mate 2");
    return false;
  }
  return true;
}

// <out_dir>/<name>.fq, or <out_dir>/<name>_R<mate>.fq for two inputs (mate: 1 or 2); destination N is "undetermined"
inline std::string out_path(const Sheet& sh, const char* out_dir, uint32_t d, bool two, int mate) {
  std::string p = out_dir;
  if (p.empty() || p.back() != '/') p += '/';
  p += d < sh.n() ? sh.name[d] : std::string("undetermined");
  if (two) p += mate == 1 ? "_R1" : "_R2";
  return p + ".fq";
}

// the report row (include/sc_fqcount.h: scfq_format_demux_row_tsv)
inline int format_row(const scfq_demux_stats* s, const Sheet& sh, uint32_t d, const scfq_demux_row* row, char* buf, uint64_t cap) {
  if (!s || !row || d > sh.n() || s->n_samples != sh.n()) return SCFQ_EARG;
  const bool und = d == sh.n();
  const std::string bc = und ? std::string("-") : (sh.dual ? sh.bc1[d] + "+" + sh.bc2[d] : sh.bc1[d]);
  const uint64_t pct = s->units_in ? (uint64_t)(((unsigned __int128)row->units * 10000u) / s->units_in) : 0;
  char tmp[512];
  const int m = std::snprintf(tmp, sizeof tmp, "%s\t%s\t%llu\t%llu.%02llu\t%llu\t%llu\t%llu\t%llu\t%llu", und ? "undetermined" : sh.name[d].c_str(), bc.c_str(),
                              (unsigned long long)row->units, (unsigned long long)(pct / 100), (unsigned long long)(pct % 100), (unsigned long long)row->perfect,
                              (unsigned long long)row->mismatched, (unsigned long long)row->bases_out, (unsigned long long)row->bytes1,
                              (unsigned long long)row->bytes2);
  return scfq_reads::copy_text(tmp, m, buf, cap);
}

}  // namespace scfq_demux_host

// scfq_host.cpp — device-independent part of the C ABI (include/sc_fqcount.h): the partial monoid
// on the host, finalisation into the reference's counters, and the reference's output formatting.
//
// Reference anchors:
//   src/fq_count.nim:39-41   reads = #{i : i mod 4 == 1}  == ceil(lines/4)
//   src/fq_count.nim:42-45   sequence line is i mod 4 == 2  == relative class r = 1 from phase 0
//   src/fq_count.nim:47-51   output fields and `$` formatting (Nim 1.0.6 `$float` = "%.16g" + ".0" rule)
#include "../../include/sc_fqcount.h"
#include "scfq_copy_text.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>

extern "C" {

void scfq_partial_identity(scfq_partial* p, uint64_t* hist) {
  if (p) std::memset(p, 0, sizeof(*p));
  if (hist) std::memset(hist, 0, SCFQ_HIST_WORDS * sizeof(uint64_t));
}

static inline void rot_add(uint64_t* acc, const uint64_t* b, unsigned k) {
  uint64_t t[4];
  for (unsigned r = 0; r < 4; ++r) t[r] = acc[r] + b[(r - k) & 3u];
  for (unsigned r = 0; r < 4; ++r) acc[r] = t[r];
}

int scfq_partial_combine(scfq_partial* acc, const scfq_partial* b, uint64_t* hist_acc, const uint64_t* hist_b) {
  if (!acc || !b) return SCFQ_EARG;
  const unsigned k = (unsigned)(acc->nl & 3u);
  rot_add(acc->gc, b->gc, k);
  rot_add(acc->n, b->n, k);
  rot_add(acc->len, b->len, k);
  rot_add(acc->starts, b->starts, k);
  rot_add(acc->first_at, b->first_at, k);
  rot_add(acc->first_plus, b->first_plus, k);
  {
    // which class histograms stay complete: b's class c lands on class (c + k) & 3 of the result
    const uint64_t cb = (b->hist_class >= 1 && b->hist_class <= 4) ? (((b->hist_class - 1) + k) & 3u) + 1 : b->hist_class;
    if (acc->hist_class == 0) acc->hist_class = cb;
    else if (cb != 0 && cb != acc->hist_class) acc->hist_class = 5;
  }
  if (hist_acc && hist_b) {
    for (unsigned c = 0; c < 4; ++c) {
      const uint64_t* src = hist_b + ((c - k) & 3u) * 256;
      uint64_t* dst = hist_acc + c * 256;
      for (unsigned v = 0; v < 256; ++v) dst[v] += src[v];
    }
  }
  acc->reserved[0] |= b->reserved[0];   // status word of a sharded count: non-zero when a contributing shard failed
  acc->nl += b->nl;
  if (b->bytes) acc->last_byte = b->last_byte;
  acc->bytes += b->bytes;
  return SCFQ_OK;
}

int scfq_partial_finalize(const scfq_partial* p, const uint64_t* hist, scfq_counts* out) {
  if (!p || !out) return SCFQ_EARG;
  if (out->struct_size != sizeof(scfq_counts)) return SCFQ_EARG;
  std::memset(out, 0, sizeof(*out));
  out->struct_size = sizeof(scfq_counts);
  out->abi_version = SCFQ_ABI_VERSION;
  // relative class 1 from phase 0 is the reference's `i mod 4 == 2`
  out->gc_bases = p->gc[1];
  out->n_bases = p->n[1];
  out->bases = p->len[1];
  out->newlines = p->nl;
  out->input_bytes = p->bytes;
  // a final line without '\n' still counts (Nim readLine returns it)
  out->lines = p->nl + ((p->bytes > 0 && p->last_byte != (uint64_t)'\n') ? 1u : 0u);
  out->reads = (out->lines + 3) / 4;
  out->bad_at = p->starts[0] - p->first_at[0];
  out->bad_plus = p->starts[2] - p->first_plus[2];
  if (hist) {
    if (p->hist_class != 0 && p->hist_class != 4) return SCFQ_ESPEC;   // the speculative form completed another class
    std::memcpy(out->qual_hist, hist + 3 * 256, 256 * sizeof(uint64_t));   // class 3 == `i mod 4 == 0`
  }
  return SCFQ_OK;
}

// Nim 1.0.6 system/formatfloat.nim writeFloatToBuffer: sprintf("%.16g"), ',' -> '.', append ".0"
// when no '.' and no letter, collapse any NaN spelling to "nan" and infinities to "inf"/"-inf".
static int nim_float_to_str(double v, char* f, size_t cap) {
  int m = std::snprintf(f, cap, "%.16g", v);
  bool has_dot = false;
  for (int k = 0; k < m; ++k) {
    if (f[k] == ',') { f[k] = '.'; has_dot = true; }
    else if ((f[k] >= 'a' && f[k] <= 'z') || (f[k] >= 'A' && f[k] <= 'Z') || f[k] == '.') has_dot = true;
  }
  if (!has_dot) { f[m] = '.'; f[m + 1] = '0'; f[m + 2] = 0; m += 2; }
  if (m > 0 && (f[m - 1] == 'n' || f[m - 1] == 'N')) { std::strcpy(f, "nan"); m = 3; }
  else if (m > 0 && (f[m - 1] == 'f' || f[m - 1] == 'F')) { std::strcpy(f, f[0] == '-' ? "-inf" : "inf"); m = (int)std::strlen(f); }
  return m;
}

int scfq_format_tsv(const scfq_counts* c, char* buf, uint64_t cap) {
  if (!c) return SCFQ_EARG;
  // $(gc_cnt.float / (total_len - n_cnt).float)      src/fq_count.nim:48 (int64 -> float64)
  const double v = (double)(int64_t)c->gc_bases / (double)(int64_t)(c->bases - c->n_bases);
  char f[96];
  nim_float_to_str(v, f, sizeof f);
  char tmp[256];
  const int m = std::snprintf(tmp, sizeof tmp, "%llu\t%s\t%llu\t%llu\t%llu", (unsigned long long)c->reads, f,
                              (unsigned long long)c->gc_bases, (unsigned long long)c->n_bases,
                              (unsigned long long)c->bases);
  return scfq_reads::copy_text(tmp, m, buf, cap);
}

// the fq-readstats row: mean_len and mean_qual by the same `$float` rule
int scfq_format_read_stats_tsv(const scfq_read_summary* s, char* buf, uint64_t cap) {
  if (!s) return SCFQ_EARG;
  char ml[96], mq[96];
  nim_float_to_str((double)s->bases / (double)s->reads, ml, sizeof ml);
  nim_float_to_str((double)s->qual_sum / (double)s->qual_bytes, mq, sizeof mq);
  char tmp[512];
  const int m = std::snprintf(tmp, sizeof tmp, "%llu\t%llu\t%llu\t%llu\t%s\t%llu\t%llu\t%llu\t%llu\t%s", (unsigned long long)s->reads,
                              (unsigned long long)s->bases, (unsigned long long)s->min_len, (unsigned long long)s->max_len, ml,
                              (unsigned long long)s->n50, (unsigned long long)s->l50, (unsigned long long)s->n90,
                              (unsigned long long)s->l90, mq);
  return scfq_reads::copy_text(tmp, m, buf, cap);
}

// the fq-cycles row: other = bases - a - c - g - t - n, mean_qual by the same `$float` rule
int scfq_format_cycle_row_tsv(const scfq_cycle_row* r, char* buf, uint64_t cap) {
  if (!r) return SCFQ_EARG;
  char mq[96];
  nim_float_to_str((double)r->qual_sum / (double)r->quals, mq, sizeof mq);
  char tmp[512];
  const int m = std::snprintf(tmp, sizeof tmp, "%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%s", (unsigned long long)r->bases,
                              (unsigned long long)r->a, (unsigned long long)r->c, (unsigned long long)r->g, (unsigned long long)r->t,
                              (unsigned long long)r->n, (unsigned long long)(r->bases - r->a - r->c - r->g - r->t - r->n),
                              (unsigned long long)r->quals, mq);
  return scfq_reads::copy_text(tmp, m, buf, cap);
}

// the fq-kmers row: the k letters of the index, first base first, and the count
int scfq_format_kmer_tsv(uint32_t k, uint64_t index, uint64_t count, char* buf, uint64_t cap) {
  if (k < 1 || k > SCFQ_KMERS_MAX_K || index >> (2 * k)) return SCFQ_EARG;
  char tmp[64];
  for (uint32_t i = 0; i < k; ++i) tmp[i] = "ACGT"[(index >> (2 * (k - 1 - i))) & 3u];
  const int m = (int)k + std::snprintf(tmp + k, sizeof tmp - k, "\t%llu", (unsigned long long)count);
  return scfq_reads::copy_text(tmp, m, buf, cap);
}

// the built-in probes of fq-adapters: the names and 12-mers the common QC tools use
int scfq_adapters_default(uint32_t i, const char** name, const char** seq) {
  static const char* const kSet[][2] = {
      {"illumina_universal", "AGATCGGAAGAG"}, {"illumina_small_rna_3p", "TGGAATTCTCGG"}, {"illumina_small_rna_5p", "GATCGTCGGACT"},
      {"nextera", "CTGTCTCTTATA"},            {"polya", "AAAAAAAAAAAA"},                 {"polyg", "GGGGGGGGGGGG"},
      {"solid_small_rna", "CGCCTTGGCCGT"}};
  const uint32_t size = sizeof kSet / sizeof kSet[0];
  if (i >= size) return SCFQ_EARG;
  if (name) *name = kSet[i][0];
  if (seq) *seq = kSet[i][1];
  return (int)size;
}

// the fq-adapters row: the integers, or their share of `reads` in percent by the same `$float` rule
int scfq_format_adapter_row_tsv(const scfq_adapter_row* r, uint32_t n_probes, uint64_t reads, int counts, char* buf, uint64_t cap) {
  if (!r || n_probes < 1 || n_probes > SCFQ_ADAPTERS_MAX_PROBES) return SCFQ_EARG;
  char tmp[(SCFQ_ADAPTERS_MAX_PROBES + 1) * 100];
  int m = 0;
  for (uint32_t j = 0; j <= n_probes; ++j) {
    const uint64_t v = j < n_probes ? r->first[j] : r->any;
    if (j) tmp[m++] = '\t';
    if (counts) m += std::snprintf(tmp + m, sizeof tmp - m, "%llu", (unsigned long long)v);
    else m += nim_float_to_str(100.0 * (double)v / (double)reads, tmp + m, 96);
  }
  tmp[m] = 0;
  return scfq_reads::copy_text(tmp, m, buf, cap);
}

// the fq-insert-size row.  The variance's numerator is exact (128 bits) and becomes a double once, so a checker with big integers
// gets the same bits
int scfq_format_insert_size_tsv(const scfq_insert_summary* s, char* buf, uint64_t cap) {
  if (!s) return SCFQ_EARG;
  const unsigned __int128 num = (unsigned __int128)s->overlapped * s->insert_sq_sum - (unsigned __int128)s->insert_sum * s->insert_sum;
  char pct[96], mean[96], sd[96], mr[96];
  nim_float_to_str(100.0 * (double)s->overlapped / (double)s->pairs, pct, sizeof pct);
  nim_float_to_str((double)s->insert_sum / (double)s->overlapped, mean, sizeof mean);
  nim_float_to_str(std::sqrt((double)num) / (double)s->overlapped, sd, sizeof sd);
  nim_float_to_str((double)s->mismatches / (double)s->overlap_bases, mr, sizeof mr);
  char tmp[1024];
  const int m = std::snprintf(tmp, sizeof tmp, "%llu\t%llu\t%s\t%llu\t%llu\t%s\t%s\t%llu\t%llu\t%llu\t%s", (unsigned long long)s->pairs,
                              (unsigned long long)s->overlapped, pct, (unsigned long long)s->min_insert, (unsigned long long)s->median_insert,
                              mean, sd, (unsigned long long)s->mode_insert, (unsigned long long)s->max_insert,
                              (unsigned long long)s->read_through, mr);
  return scfq_reads::copy_text(tmp, m, buf, cap);
}

// the fq-merge row: integers but for the share of merged pairs
int scfq_format_merge_stats_tsv(const scfq_merge_stats* s, char* buf, uint64_t cap) {
  if (!s) return SCFQ_EARG;
  char pct[96];
  nim_float_to_str(100.0 * (double)s->merged / (double)s->pairs, pct, sizeof pct);
  const uint64_t tail[] = {s->not_overlapped, s->too_long, s->unpaired, s->merged_bases, s->overlap_bases, s->mismatches, s->took_mate1,
                           s->took_mate2, s->neither_valid, s->merged_bytes, s->unmerged1_bytes, s->unmerged2_bytes};
  char tmp[1024];
  int m = std::snprintf(tmp, sizeof tmp, "%llu\t%llu\t%s", (unsigned long long)s->pairs, (unsigned long long)s->merged, pct);
  for (const uint64_t v : tail) m += std::snprintf(tmp + m, sizeof tmp - m, "\t%llu", (unsigned long long)v);
  return scfq_reads::copy_text(tmp, m, buf, cap);
}

// the fq-trim row: integers only; the reads per probe as one field
int scfq_format_trim_stats_tsv(const scfq_trim_stats* s, char* buf, uint64_t cap) {
  if (!s || s->n_probes > SCFQ_TRIM_MAX_PROBES) return SCFQ_EARG;
  const uint64_t head[] = {s->reads_in,     s->reads_out,    s->dropped_reads, s->short_reads, s->too_long,      s->pairs,     s->unpaired,
                           s->overlapped_pairs, s->bases_in, s->bases_out,     s->bases_dropped, s->cut_overlap, s->bases_overlap, s->cut_adapter,
                           s->bases_adapter, s->cut_polyg,   s->bases_polyg,   s->cut_quality, s->bases_quality};
  char tmp[1024];
  int m = 0;
  for (const uint64_t v : head) m += std::snprintf(tmp + m, sizeof tmp - m, "%llu\t", (unsigned long long)v);
  for (uint64_t j = 0; j < s->n_probes; ++j) m += std::snprintf(tmp + m, sizeof tmp - m, j ? ",%llu" : "%llu", (unsigned long long)s->adapter_reads[j]);
  if (!s->n_probes) m += std::snprintf(tmp + m, sizeof tmp - m, "-");
  m += std::snprintf(tmp + m, sizeof tmp - m, "\t%llu\t%llu", (unsigned long long)s->out1_bytes, (unsigned long long)s->out2_bytes);
  return scfq_reads::copy_text(tmp, m, buf, cap);
}

const char* scfq_strerror(int rc) {
  switch (rc) {
    case SCFQ_OK: return "ok";
    case SCFQ_EOPEN: return "unable to open file";
    case SCFQ_EGZ: return "gzip stream error";
    case SCFQ_EHIP: return "HIP runtime error (is a gfx950 GPU visible?)";
    case SCFQ_ERCCL: return "collective exchange error";
    case SCFQ_EARG: return "invalid argument";
    case SCFQ_EIO: return "read / write error";
    case SCFQ_EPIPE: return "broken pipe on the output descriptor";
    case SCFQ_ENOMEM: return "out of host memory";
    case SCFQ_ESPEC: return "speculative quality histogram did not verify across shards (retry with SCFQ_HIST_EXACT)";
    case SCFQ_EFULL: return "the k-mer table is full";
    default: return "unknown error";
  }
}

}  // extern "C"

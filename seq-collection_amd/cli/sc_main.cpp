// sc_main.cpp — C++ host for the `sc` commands over the C ABI (include/sc_fqcount.h).  What the commands share (error and
// filename-column helpers, the option parser, the per-file scaffold) is in sc_cli.hpp; this file holds one function per command.
//
// The reference host is Nim (sc.nim + src/fq_count.nim); no Nim toolchain exists in this image, so the
// host side above the C ABI is written in C++ and mirrors the reference's surface for this path:
//   sc.nim:103-116                 command "fq-count": -t/--header, -b/--basename, -a/--absolute, [fastq ...]
//   sc.nim:274-293                 stdin '-' -> literal "STDIN"; bare `sc` -> help
//   src/fq_count.nim:14-53         one TSV row per file, argv order; "Unable to open file" exit 2
// Everything between "open the file" and "format the row" is one call into libsc_fqcount_hip.so.
// GPU-only additions are new long options and never change the reference's 5-column row.
#include "sc_cli.hpp"
#include "../../include/sc_fqcount_debug.h"      // --stats: the library's stage marks

#include <fcntl.h>
#include <signal.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <condition_variable>
#include <mutex>
#include <thread>

static const char* kVersion = "0.0.2-mi355x";
static const char* kHeader = "reads\tgc_content\tgc_bases\tn_bases\tbases";   // src/fq_count.nim:7-11

static const char* const kHelpFqCount =   // docs/fq-count.md:5-19
      "Counts lines in a FASTQ\n\n"
      "Usage:\n"
      "  fq-count [options] [fastq ...]\n\n"
      "Arguments:\n"
      "  [fastq ...]      Input FASTQ\n\n"
      "Options:\n"
      "  -t, --header               Output the header\n"
      "  -b, --basename             Add basename column\n"
      "  -a, --absolute             Add column for absolute path\n"
      "  -h, --help                 Show this help\n"
      "\nMI355X options (additions; the TSV row is unchanged):\n"
      "      --devices=LIST         Comma-separated HIP device ids to shard each file across (default: current device)\n"
      "      --struct-check         Report header lines not starting '@' / separator lines not starting '+' on stderr\n"
      "      --qual-hist            Print the quality-byte histogram on stderr\n"
      "      --stats                Print bytes / device milliseconds / GB/s as JSON on stderr\n"
      "      --jobs=N               Keep up to N files in flight (default: 2; rows still come out in argument order)\n"
      "      --shard-rank=R --shard-world=W --rendezvous=HOST:PORT [--transport=rccl|tcp]\n"
      "                             One process per GPU: this process scans byte range R of W of every file on its device\n"
      "                             (--devices=ID, default R), the partials are exchanged (RCCL all-gather), rank 0 prints\n"
      "                             the rows. Defaults come from RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT.\n";

static void help_top(FILE* f) {
  std::fprintf(f,
               "sc (%s) — MI355X-native host for the fq-count path of seq-collection\n\n"
               "Usage:\n  sc COMMAND\n\nCommands:\n\nFASTQ\n  fq-count         Counts lines in a FASTQ\n"
               "  fq-dedup         Removes exact duplicates from FASTQ Files\n  fq-meta          Output metadata for FASTQ\n"
               "  fq-readstats     Per-read length, N50, GC and quality of a FASTQ\n"
               "  fq-cycles        Per-position base composition and quality of a FASTQ\n"
               "  fq-kmers         K-mer spectrum of the sequence lines of a FASTQ\n"
               "  fq-adapters      Adapter content by read position of a FASTQ\n"
               "  fq-insert-size   Insert sizes from the overlap of the mates of read pairs\n"
               "  fq-merge         Merge overlapping read pairs into single reads\n\n"
               "FASTA\n  fa-gc            Calculate GC content surrouding a location\n\n"
               "Options:\n  -h, --help                 Show this help\n  -v, --version              Show version\n"
               "      --debug                Debug mode\n",
               kVersion);
}

static bool stdin_is_fifo() {   // sc.nim:50-53
  struct stat st;
  return fstat(0, &st) == 0 && S_ISFIFO(st.st_mode);
}

// One file's outcome: what proc fq_count would have echoed / which error it would have quit with.
struct FileResult {
  int exit_code = 0;          // 0, or the quit_error code
  std::string error;          // message for quit_error
  std::string row;            // stdout line (without newline)
  std::string extra;          // stderr lines of the MI355X additions
};

// proc fq_count*(fastq: string, basename: bool, absolute: bool)      src/fq_count.nim:14  (compute part)
// (it runs on the threads of --jobs, so an error is handed back instead of quitting here)
static FileResult fq_count_compute(const std::string& fastq, const Columns& cols, const scfq_opts& opts, scfq_comm* comm = nullptr) {
  FileResult r;
  if (fastq.size() < 3) { r.exit_code = 1; r.error = kIndexOutOfBounds; return r; }   // as require_suffix_room()
  scfq_counts c = fresh<scfq_counts>();
  // one process per GPU: this rank's byte range, exchange, every rank gets the whole file's counters
  const int rc = comm ? scfq_count_file_sharded(fastq.c_str(), &opts, comm, &c) : scfq_count_file(fastq.c_str(), &opts, &c);
  if (rc == SCFQ_EOPEN) { r.exit_code = unable_to_open_code(fastq); r.error = unable_to_open(fastq); return r; }
  if (rc != SCFQ_OK) { r.exit_code = 1; r.error = library_error(rc); return r; }
  char row[256];
  scfq_format_tsv(&c, row, sizeof row);
  r.row = cols.row(row, fastq);
  char buf[512];
  if (opts.flags & SCFQ_STRUCT_CHECK) {
    std::snprintf(buf, sizeof buf, "%s\tbad_at=%llu\tbad_plus=%llu\n", fastq.c_str(), (unsigned long long)c.bad_at, (unsigned long long)c.bad_plus);
    r.extra += buf;
  }
  if (opts.flags & SCFQ_QUAL_HIST) {
    r.extra += fastq + "\tqual_hist";
    for (int v = 0; v < 256; ++v)
      if (c.qual_hist[v]) { std::snprintf(buf, sizeof buf, "\t%d:%llu", v, (unsigned long long)c.qual_hist[v]); r.extra += buf; }
    r.extra += "\n";
  }
  if (opts.flags & SCFQ_TIMING) {          // --stats
    scfq_timing t = fresh<scfq_timing>();
    scfq_last_timing(&t);
    const double gbs = t.scan_kernel_ms > 0 ? (double)t.scan_bytes / (t.scan_kernel_ms * 1e-3) / 1e9 : 0.0;
    char js[1024];
    std::snprintf(js, sizeof js,
                  "{\"file\": \"%s\", \"input_bytes\": %llu, \"scan_kernel_ms\": %.4f, \"fold_kernel_ms\": %.4f, "
                  "\"scan_launches\": %llu, \"scan_GBps\": %.1f, \"hbm_peak_GBps\": 8000, \"roofline_frac\": %.4f, "
                  "\"host_fill_ms\": %.2f, \"ingest_wall_ms\": %.2f, \"h2d_bytes\": %llu, \"device_bytes_high_water\": %llu, \"stages_ms\": ",
                  fastq.c_str(), (unsigned long long)c.input_bytes, t.scan_kernel_ms, t.fold_kernel_ms,
                  (unsigned long long)t.scan_launches, gbs, gbs / 8000.0, t.host_fill_ms, t.ingest_wall_ms,
                  (unsigned long long)t.h2d_bytes, (unsigned long long)scfq_device_bytes_high_water());
    r.extra += js;
    // where the process's time went up to this row: [name, ms since the library was loaded] (include/sc_fqcount_debug.h)
    scfq_debug_stage_mark("sc: row computed");
    // (with --jobs another session's thread may add a mark between the sizing call and the filling one: ask again until the
    // text fits, and keep the row valid JSON whatever happens)
    std::string stages;
    for (int attempt = 0; attempt < 8; ++attempt) {
      stages.assign((size_t)scfq_debug_stages(nullptr, 0) + 256, '\0');
      const uint64_t need = scfq_debug_stages(&stages[0], stages.size());
      if (need < stages.size()) { stages.resize(std::strlen(stages.c_str())); break; }
      stages.clear();
    }
    if (stages.empty()) stages = "[]";
    r.extra += stages + "}\n";
  }
  return r;
}

// ... and its output part: echo the row (fq_count.nim:53) or quit_error
static void fq_count_emit(const FileResult& r) {
  if (r.exit_code) quit_error(r.error, r.exit_code);
  std::printf("%s\n", r.row.c_str());
  if (std::fflush(stdout) != 0) { /* EPIPE is swallowed like sc.nim:304 */ }
  if (!r.extra.empty()) std::fputs(r.extra.c_str(), stderr);
}

// Nim 1.0.6 `$float` as used by stderr.writeLine (src/fq_dedup.nim:80): "%.16g", ".0" appended when the text has neither
// '.' nor a letter, NaN -> "nan"
static std::string nim_float(double v) {
  if (v != v) return "nan";
  char f[64];
  std::snprintf(f, sizeof f, "%.16g", v);
  std::string t(f);
  if (t.find_first_of(".abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ") == std::string::npos) t += ".0";
  return t;
}

// command "fq-dedup" (sc.nim:118-122): one positional FASTQ, no options; proc fq_dedup (src/fq_dedup.nim:14-84)
static int cmd_fq_dedup(const std::vector<std::string>& params) {
  static const char* const help =
      "Removes exact duplicates from FASTQ Files\n\nUsage:\n  fq-dedup [options] fastq\n\nArguments:\n"
      "  fastq            Input FASTQ\n\nOptions:\n  -h, --help                 Show this help\n";
  // the reference's grammar: every argument but -h is a file
  std::vector<std::string> files;
  for (size_t i = 1; i < params.size(); ++i) {
    if (params[i] == "-h" || params[i] == "--help") { std::fputs(help, stdout); return 0; }
    files.push_back(params[i]);
  }
  if (files.size() != 1) { std::fputs(help, stdout); quit_error(files.empty() ? "Missing argument: fastq" : "Unknown argument(s): " + files[1], 1); }
  const std::string& fastq = files[0];
  if (fastq == "STDIN") quit_error("This command does not support stdin");                    // sc.nim:58-60
  struct stat sb;
  if (stat(fastq.c_str(), &sb) != 0 || S_ISDIR(sb.st_mode))                                    // helpers.nim:39-43
    quit_error(fastq + " does not exist or is not readable");
  scfq_dedup_stats st = fresh<scfq_dedup_stats>();
  // the reference announces "No Duplicates Found" before pass 2 starts echoing (fq_dedup.nim:51-53); here the FASTQ goes
  // to fd 1 first and all diagnostics follow: stdout is byte-identical and the lines on stderr keep their order
  std::fflush(stdout);
  const int rc = scfq_dedup_file(fastq.c_str(), nullptr, 1, &st);
  if (rc == SCFQ_EOPEN) quit_unable_to_open(fastq, 2);                                          // fq_dedup.nim:37-38
  if (rc == SCFQ_EPIPE) return 0;              // `errno: 32 Broken pipe` is swallowed (sc.nim:304); any other IOError exits 1 (sc.nim:299-305)
  if (rc != SCFQ_OK) quit_error(std::string(scfq_strerror(rc)) + ": " + scfq_dedup_error_detail() + scfq_last_error_detail(), 1);
  if (st.duplicates == 0) std::fputs("No Duplicates Found\nCopying fq to stdout\n", stderr);   // :51-53 (check.len == 0)
  std::fprintf(stderr, "total_reads: %llu\n", (unsigned long long)st.total_reads);            // :74
  std::fprintf(stderr, "duplicates %llu\n", (unsigned long long)st.duplicates);                // :75
  std::fprintf(stderr, "false-positive: %llu\n", (unsigned long long)st.false_positive);      // :79
  std::fprintf(stderr, "false-positive-rate: %s\n", nim_float((double)st.false_positive / (double)st.duplicates).c_str());   // :80
  return 0;
}

// command "fq-meta" (sc.nim:67-79): -n/--lines (default 100), -t/--header, -b/--basename, -a/--absolute, [fastq ...]
static int cmd_fq_meta(const std::vector<std::string>& params) {
  static const char* const help =
      "Output metadata for FASTQ\n\nUsage:\n  fq-meta [options] [fastq ...]\n\nArguments:\n  [fastq ...]      List of FASTQ files\n\n"
      "Options:\n  -n, --lines=LINES          Number of sequences to sample (n_lines) for qual and index/barcode determination (default: 100)\n"
      "  -t, --header               Output the header\n  -b, --basename             Add basename column\n"
      "  -a, --absolute             Add column for absolute path\n  -h, --help                 Show this help\n"
      "\nMI355X option (addition):\n      --whole-file           Quality range from the histogram of every quality line (device scan)\n";
  // the reference's grammar (no "--", no short cluster, -n 5 / -n5 / -n=5 / --lines 5), so not a table for parse_options()
  Columns cols;
  uint32_t flags = 0;
  std::string lines = "100";
  std::vector<std::string> files;
  for (size_t i = 1; i < params.size(); ++i) {
    const std::string& a = params[i];
    if (a == "-h" || a == "--help") { std::fputs(help, stdout); return 0; }
    else if (a == "-t" || a == "--header") cols.header = true;
    else if (a == "-b" || a == "--basename") cols.basename = true;
    else if (a == "-a" || a == "--absolute") cols.absolute = true;
    else if (a == "--whole-file") flags |= SCFQ_META_WHOLE_FILE;
    else if ((a == "-n" || a == "--lines") && i + 1 < params.size()) lines = params[++i];
    else if (a.rfind("--lines=", 0) == 0) lines = a.substr(8);
    else if (a.rfind("-n", 0) == 0 && a.size() > 2 && a[1] == 'n') lines = a.substr(a[2] == '=' ? 3 : 2);
    else if (a.size() > 1 && a[0] == '-' && a != "-") unknown_option(help, a);
    else files.push_back(a);
  }
  char* endp = nullptr;
  const long n = std::strtol(lines.c_str(), &endp, 10);
  if (lines.empty() || *endp || n < 0) quit_error("invalid integer: " + lines, 1);      // parseInt raises ValueError (sc.nim:79)
  cols.header_or_no_input(scfq_meta_header(), false);                                      // sc.nim:75-76 (no file is no error here)
  for (const auto& fastq : files) {                                                          // sc.nim:77-79
    char row[4096];
    const int rc = scfq_meta_file_tsv(fastq.c_str(), (uint32_t)n, flags, row, sizeof row);
    if (rc == SCFQ_EOPEN) quit_unable_to_open(fastq, 2);                                     // fq_meta.nim:223-224
    if (rc == SCFQ_EARG) quit_error(kIndexOutOfBounds, 1);                                   // extract_read_info IndexError -> sc.nim:299-305
    if (rc < 0) quit_error(std::string(scfq_strerror(rc)) + ": " + scfq_last_error_detail(), 1);
    cols.emit_row(row, fastq);
  }
  std::fflush(stdout);
  return 0;
}

// command "fq-readstats" (addition, not in the reference): -t/--header, -b/--basename, -a/--absolute as fq-count, [fastq ...]
static const char* kReadStatsHeader = "reads\tbases\tmin_len\tmax_len\tmean_len\tn50\tl50\tn90\tl90\tmean_qual";
static int cmd_fq_readstats(const std::vector<std::string>& params) {
  static const char* const help =
      "Per-read length, N50, GC and quality of a FASTQ\n\nUsage:\n  fq-readstats [options] [fastq ...]\n\nArguments:\n"
      "  [fastq ...]      Input FASTQ\n\nOptions:\n  -t, --header               Output the header\n"
      "  -b, --basename             Add basename column\n  -a, --absolute             Add column for absolute path\n"
      "      --hist=len|gc|qual     Print bin<TAB>count of the non-empty bins of a histogram instead of the row:\n"
      "                             len: bit length of the read length; gc: percent G+C of the non-N bases (101: none);\n"
      "                             qual: mean quality byte\n"
      "  -h, --help                 Show this help\n";
  Columns cols;
  std::string hist;
  std::vector<std::string> files;
  const std::vector<Opt> table = cols.options({
      opt_custom("hist", [&](std::string& v) {     // one of the three names; any other spelling is no option at all
        if (v != "len" && v != "gc" && v != "qual") return Reject::unknown_option;
        hist = v;
        return Reject::none;
      }),
  });
  if (!parse_options(params, help, table, &files)) return 0;
  cols.header_or_no_input(hist.empty() ? kReadStatsHeader : "bin\tcount", files.empty());
  for (const auto& fastq : files) {
    require_suffix_room(fastq);
    scfq_read_summary s = fresh<scfq_read_summary>();
    const int rc = scfq_read_stats_file(fastq.c_str(), nullptr, &s);
    if (rc == SCFQ_EOPEN) quit_unable_to_open(fastq);
    if (rc != SCFQ_OK) quit_error(library_error(rc, scfq_read_stats_error_detail()), 1);
    if (hist.empty()) {
      char row[512];
      scfq_format_read_stats_tsv(&s, row, sizeof row);
      cols.emit_row(row, fastq);
    } else {
      const uint64_t* h = hist == "len" ? s.len_hist : (hist == "gc" ? s.gc_hist : s.meanq_hist);
      const int bins = hist == "len" ? SCFQ_LEN_HIST_BINS : (hist == "gc" ? SCFQ_GC_HIST_BINS : SCFQ_MEANQ_HIST_BINS);
      for (int k = 0; k < bins; ++k) {
        if (!h[k]) continue;
        char line[64];
        std::snprintf(line, sizeof line, "%d\t%llu", k, (unsigned long long)h[k]);
        cols.emit_row(line, fastq);
      }
    }
  }
  std::fflush(stdout);
  return 0;
}

// command "fq-cycles" (addition, not in the reference): -t/--header, -b/--basename, -a/--absolute as fq-count, --max-cycles=N, [fastq ...]
static const char* kCyclesHeader = "cycle\tbases\tA\tC\tG\tT\tN\tother\tquals\tmean_qual";
static int cmd_fq_cycles(const std::vector<std::string>& params) {
  static const char* const help =
      "Per-position base composition and quality of a FASTQ\n\nUsage:\n  fq-cycles [options] [fastq ...]\n\nArguments:\n"
      "  [fastq ...]      Input FASTQ\n\nOptions:\n  -t, --header               Output the header\n"
      "  -b, --basename             Add basename column\n  -a, --absolute             Add column for absolute path\n"
      "      --max-cycles=N         One row per position up to N (default: 1000, at most 16777216); what lies beyond\n"
      "                             comes added up as one last row \">N\"\n"
      "  -h, --help                 Show this help\n";
  Columns cols;
  uint64_t max_cycles = 1000;
  std::vector<std::string> files;
  const std::vector<Opt> table = cols.options({opt_number("max-cycles", 8, 0, SCFQ_CYCLES_MAX_CAP, &max_cycles)});
  if (!parse_options(params, help, table, &files)) return 0;
  cols.header_or_no_input(kCyclesHeader, files.empty());
  std::vector<scfq_cycle_row> rows;
  for (const auto& fastq : files) {
    require_suffix_room(fastq);
    scfq_cycle_summary s;
    // the table is as long as the file's longest line, not as --max-cycles
    const int rc = size_then_fill(
        &rows, &s, [&](scfq_cycle_row* r, uint64_t n, scfq_cycle_summary* out) { return scfq_cycles_file(fastq.c_str(), nullptr, r, n, out); },
        [&](const scfq_cycle_summary& sized) { return std::min<uint64_t>(max_cycles, std::max(sized.max_seq_len, sized.max_qual_len)); });
    if (rc == SCFQ_EOPEN) quit_unable_to_open(fastq);
    if (rc != SCFQ_OK) quit_error(library_error(rc, scfq_cycles_error_detail()), 1);
    char row[512];
    for (uint64_t p = 0; p < s.cycles; ++p) {
      scfq_format_cycle_row_tsv(&rows[p], row, sizeof row);
      cols.emit_row(std::to_string(p + 1) + "\t" + row, fastq);
    }
    if (s.tail.bases || s.tail.quals) {
      scfq_format_cycle_row_tsv(&s.tail, row, sizeof row);
      cols.emit_row(">" + std::to_string(max_cycles) + "\t" + row, fastq);
    }
  }
  std::fflush(stdout);
  return 0;
}

// command "fq-insert-size" (addition, not in the reference): -t/--header, -b/--basename, -a/--absolute as fq-count, --interleaved,
// --min-overlap=N, --max-mismatches=N, --max-mismatch-pct=N, --dist, R1.fq R2.fq [R1.fq R2.fq ...]
static const char* kInsertHeader = "pairs\toverlapped\tpercent_overlapped\tmin\tmedian\tmean\tstd_dev\tmode\tmax\tread_through\tmismatch_rate";
static const char* kInsertDistHeader = "insert_size\tcount";
static int cmd_fq_insert_size(const std::vector<std::string>& params) {
  static const char* const help =
      "Insert sizes from the overlap of the two mates of a read pair\n\nUsage:\n  fq-insert-size [options] R1.fq R2.fq [R1.fq R2.fq ...]\n\n"
      "Arguments:\n  R1.fq R2.fq      Input FASTQs, two at a time: record i of each is pair i\n\nOptions:\n"
      "  -t, --header               Output the header\n"
      "  -b, --basename             Add basename column\n  -a, --absolute             Add column for absolute path\n"
      "      --interleaved          Every argument is one interleaved FASTQ: records 2i and 2i+1 are pair i\n"
      "      --min-overlap=N        Shortest overlap that is accepted (default: 30, 1 .. 512)\n"
      "      --max-mismatches=N     Most mismatches inside the overlap (default: 5, 0 .. 65535)\n"
      "      --max-mismatch-pct=N   ... and in percent of the overlap (default: 20, 0 .. 100)\n"
      "      --dist                 One row \"insert_size count\" per insert size that occurs instead of the summary row\n"
      "  -h, --help                 Show this help\n";
  Columns cols;
  bool dist = false;
  scfq_insert_opts io = fresh<scfq_insert_opts>();
  io.min_overlap = 30; io.max_mismatches = 5; io.max_mismatch_pct = 20;
  std::vector<std::string> files;
  const std::vector<Opt> table = cols.options({
      opt_bits("interleaved", &io.flags, SCFQ_INSERT_INTERLEAVED),
      opt_flag("dist", 0, &dist),
      opt_number("min-overlap", 6, 1, SCFQ_INSERT_MAX_LEN, &io.min_overlap),
      opt_number("max-mismatches", 6, 0, 65535, &io.max_mismatches),
      opt_number("max-mismatch-pct", 6, 0, 100, &io.max_mismatch_pct),
  });
  if (!parse_options(params, help, table, &files)) return 0;
  const bool interleaved = io.flags & SCFQ_INSERT_INTERLEAVED;
  if (!interleaved && files.size() % 2) usage_error(help, "FASTQs come two at a time (R1 R2), or one at a time with --interleaved");
  cols.header_or_no_input(dist ? kInsertDistHeader : kInsertHeader, files.empty());
  std::vector<uint64_t> hist(SCFQ_INSERT_HIST_BINS);
  for (size_t i = 0; i < files.size(); i += interleaved ? 1 : 2) {
    const std::string& r1 = files[i];
    const std::string* r2 = interleaved ? nullptr : &files[i + 1];
    require_suffix_room(r1);
    if (r2) require_suffix_room(*r2);
    scfq_insert_summary s = fresh<scfq_insert_summary>();
    const int rc = scfq_insert_size_files(r1.c_str(), r2 ? r2->c_str() : nullptr, nullptr, &io, nullptr, 0, hist.data(), &s);
    if (rc == SCFQ_EOPEN) quit_unable_to_open(first_unopenable(r1, r2));
    if (rc != SCFQ_OK) quit_error(library_error(rc, scfq_insert_size_error_detail()), 1);
    if (dist) {
      for (uint32_t k = 0; k < SCFQ_INSERT_HIST_BINS; ++k)
        if (hist[k]) cols.emit_row(std::to_string(k) + "\t" + std::to_string(hist[k]), r1);
    } else {
      char row[1024];
      scfq_format_insert_size_tsv(&s, row, sizeof row);
      cols.emit_row(row, r1);
    }
  }
  std::fflush(stdout);
  return 0;
}

// command "fq-merge" (addition, not in the reference): R1.fq R2.fq, or --interleaved IN.fq; merged FASTQ to stdout, --unmerged1=PATH /
// --unmerged2=PATH (--unmerged=PATH with --interleaved), --min-overlap=N, --max-mismatches=N, --max-mismatch-pct=N, --phred-offset=33|64,
// --stats (header and row of scfq_format_merge_stats_tsv to stderr)
static const char* kMergeStatsHeader = "pairs\tmerged\tpercent_merged\tnot_overlapped\ttoo_long\tunpaired\tmerged_bases\toverlap_bases\tmismatches\ttook_mate1\t"
                                       "took_mate2\tneither_valid\tmerged_bytes\tunmerged1_bytes\tunmerged2_bytes";
static int cmd_fq_merge(const std::vector<std::string>& params) {
  static const char* const help =
      "Merge overlapping read pairs into single reads; the merged FASTQ goes to stdout\n\nUsage:\n  fq-merge [options] R1.fq R2.fq\n"
      "  fq-merge [options] --interleaved IN.fq\n\n"
      "Arguments:\n  R1.fq R2.fq      Input FASTQs: record i of each is pair i\n\nOptions:\n"
      "      --interleaved          The one argument is an interleaved FASTQ: records 2i and 2i+1 are pair i\n"
      "      --unmerged1=PATH       Mate 1 of the pairs that were not merged goes to PATH\n"
      "      --unmerged2=PATH       Mate 2 of the pairs that were not merged goes to PATH\n"
      "      --unmerged=PATH        With --interleaved: both mates of the pairs that were not merged, interleaved\n"
      "      --min-overlap=N        Shortest overlap that is accepted (default: 30, 1 .. 512)\n"
      "      --max-mismatches=N     Most mismatches inside the overlap (default: 5, 0 .. 65535)\n"
      "      --max-mismatch-pct=N   ... and in percent of the overlap (default: 20, 0 .. 100)\n"
      "      --phred-offset=N       Quality offset, 33 or 64 (default: 33)\n"
      "      --stats                Print a header and a row of statistics to stderr\n"
      "  -h, --help                 Show this help\n";
  bool stats = false;
  scfq_merge_opts mo = fresh<scfq_merge_opts>();
  mo.min_overlap = 30; mo.max_mismatches = 5; mo.max_mismatch_pct = 20; mo.phred_offset = 33;
  std::vector<std::string> files;
  std::string un1, un2, un;
  // (no row has a letter: the command has no short options)
  const std::vector<Opt> table = {
      opt_bits("interleaved", &mo.flags, SCFQ_MERGE_INTERLEAVED),
      opt_flag("stats", 0, &stats),
      opt_text("unmerged1", &un1),
      opt_text("unmerged2", &un2),
      opt_text("unmerged", &un),
      opt_number("min-overlap", 6, 1, SCFQ_INSERT_MAX_LEN, &mo.min_overlap),
      opt_number("max-mismatches", 6, 0, 65535, &mo.max_mismatches),
      opt_number("max-mismatch-pct", 6, 0, 100, &mo.max_mismatch_pct),
      opt_custom("phred-offset", [&](std::string& v) {     // a number in 33 .. 64 first, then one of the two
        uint64_t n = 0;
        if (!bounded_number(v, 6, 33, 64, &n)) return Reject::bad_value;
        mo.phred_offset = (uint32_t)n;
        if (n == 33 || n == 64) return Reject::none;
        v = std::to_string(n);                             // (this message shows the number, not the text)
        return Reject::bad_value;
      }),
  };
  if (!parse_options(params, help, table, &files)) return 0;
  const bool interleaved = mo.flags & SCFQ_MERGE_INTERLEAVED;
  if (files.empty()) quit_no_fastq();
  if (files.size() != (interleaved ? 1u : 2u)) usage_error(help, "fq-merge takes R1.fq and R2.fq, or one FASTQ with --interleaved");
  if (interleaved && (!un1.empty() || !un2.empty())) usage_error(help, "--interleaved writes its unmerged pairs with --unmerged=PATH");
  if (!interleaved && !un.empty()) usage_error(help, "--unmerged=PATH goes with --interleaved; otherwise --unmerged1=PATH --unmerged2=PATH");
  if (interleaved) un1 = un;
  for (const std::string& f : files) require_suffix_room(f);
  // the inputs are looked at before an output file is made
  for (const std::string& f : files)
    if (access(f.c_str(), R_OK) != 0) quit_unable_to_open(f);
  int fd1 = -1, fd2 = -1;
  // a call that fails leaves no output file behind: what this process created goes again
  auto discard = [&]() {
    // (only a regular file: a FIFO or a device the caller named is the caller's)
    auto drop = [](int fd, const std::string& p) {
      struct stat st;
      const bool regular = fstat(fd, &st) == 0 && S_ISREG(st.st_mode);
      close(fd);
      if (regular) unlink(p.c_str());
    };
    if (fd1 >= 0) drop(fd1, un1);
    if (fd2 >= 0) drop(fd2, un2);
    fd1 = fd2 = -1;
  };
  auto create = [&](const std::string& p) -> int {
    const int fd = open(p.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (fd < 0) { discard(); quit_error("Unable to create file: " + p, 1); }
    return fd;
  };
  if (!un1.empty()) fd1 = create(un1);
  if (!un2.empty()) fd2 = create(un2);
  scfq_merge_stats st = fresh<scfq_merge_stats>();
  std::fflush(stdout);
  const int rc = scfq_merge_files(files[0].c_str(), interleaved ? nullptr : files[1].c_str(), nullptr, &mo, 1, fd1, fd2, &st);
  if (rc != SCFQ_OK && rc != SCFQ_EPIPE) discard();
  else { if (fd1 >= 0) close(fd1); if (fd2 >= 0) close(fd2); }
  if (rc == SCFQ_EOPEN) quit_unable_to_open(first_unopenable(files[0], interleaved ? nullptr : &files[1]));
  if (rc == SCFQ_EPIPE) return 0;              // a reader of stdout that went away: quiet, as `sc fq-dedup | head`
  if (rc != SCFQ_OK) quit_error(library_error(rc, scfq_merge_error_detail()), 1);
  if (stats) {
    char row[1024];
    scfq_format_merge_stats_tsv(&st, row, sizeof row);
    std::fprintf(stderr, "%s\n%s\n", kMergeStatsHeader, row);
  }
  return 0;
}

// command "fq-trim" (addition, not in the reference): IN.fq, R1.fq R2.fq with --out1=PATH --out2=PATH, or --interleaved IN.fq; the
// trimmed FASTQ of one input goes to stdout; --adapter=NAME:SEQ, --no-adapters, --min-adapter-overlap=N, --adapter-mismatch-pct=N,
// --poly-g=N, --window=N, --window-quality=N, --min-length=N, --no-overlap-trim, --min-overlap=N, --max-mismatches=N,
// --max-mismatch-pct=N, --phred-offset=33|64, --stats (header and row of scfq_format_trim_stats_tsv to stderr)
static const char* kTrimStatsHeader = "reads_in\treads_out\tdropped_reads\tshort_reads\ttoo_long\tpairs\tunpaired\toverlapped_pairs\tbases_in\tbases_out\t"
                                      "bases_dropped\tcut_overlap\tbases_overlap\tcut_adapter\tbases_adapter\tcut_polyg\tbases_polyg\tcut_quality\t"
                                      "bases_quality\tadapter_reads\tout1_bytes\tout2_bytes";
static int cmd_fq_trim(const std::vector<std::string>& params) {
  static const char* const help =
      "Cut adapters, poly-G tails, bad quality and read-through off the 3' ends of reads; pairs stay in step\n\nUsage:\n"
      "  fq-trim [options] IN.fq > out.fq\n  fq-trim [options] --out1=PATH --out2=PATH R1.fq R2.fq\n"
      "  fq-trim [options] --interleaved IN.fq > out.fq\n\n"
      "Arguments:\n  IN.fq            One FASTQ: single-end reads, or pairs with --interleaved; the result goes to stdout\n"
      "  R1.fq R2.fq      Two FASTQs: record i of each is pair i\n\nOptions:\n"
      "      --interleaved          The one argument is an interleaved FASTQ: records 2i and 2i+1 are pair i\n"
      "      --out1=PATH            With R1.fq R2.fq: the trimmed mate 1 goes to PATH\n"
      "      --out2=PATH            With R1.fq R2.fq: the trimmed mate 2 goes to PATH\n"
      "      --adapter=NAME:SEQ     Cut at SEQ (1 .. 32 letters of A C G T) and call it NAME; up to eight, and giving any\n"
      "                             replaces the built-in set (Illumina universal and small RNA, Nextera, SOLiD)\n"
      "      --no-adapters          Look for no adapter\n"
      "      --min-adapter-overlap=N   Shortest part of an adapter that is cut at the end of a read (default: 5, 1 .. 32)\n"
      "      --adapter-mismatch-pct=N  Most mismatches in percent of the compared letters (default: 10, 0 .. 100)\n"
      "      --poly-g=N             Cut a tail of N or more G (default: 0 = off, 1 .. 512)\n"
      "      --window=N             Width of the quality window (default: 4, 1 .. 32)\n"
      "      --window-quality=N     Cut at the first window whose mean quality is below N (default: 0 = off, 1 .. 93)\n"
      "      --min-length=N         Drop a read, or its pair, that is left shorter than N (default: 15, 0 .. 512)\n"
      "      --no-overlap-trim      Pairs: do not cut read-through found by the overlap of the mates\n"
      "      --min-overlap=N        Shortest overlap that is accepted (default: 30, 1 .. 512)\n"
      "      --max-mismatches=N     Most mismatches inside the overlap (default: 5, 0 .. 65535)\n"
      "      --max-mismatch-pct=N   ... and in percent of the overlap (default: 20, 0 .. 100)\n"
      "      --phred-offset=N       Quality offset, 33 or 64 (default: 33)\n"
      "      --stats                Print a header and a row of statistics to stderr\n"
      "  -h, --help                 Show this help\n";
  bool stats = false;
  scfq_trim_opts to = fresh<scfq_trim_opts>();
  to.min_overlap = 30; to.max_mismatches = 5; to.max_mismatch_pct = 20; to.min_adapter_overlap = 5; to.adapter_mismatch_pct = 10;
  to.window = 4; to.min_length = 15; to.phred_offset = 33;
  std::vector<std::string> files, names, seqs;
  std::string out1, out2;
  // (no row has a letter: the command has no short options)
  const std::vector<Opt> table = {
      opt_bits("interleaved", &to.flags, SCFQ_TRIM_INTERLEAVED),
      opt_bits("no-overlap-trim", &to.flags, SCFQ_TRIM_NO_OVERLAP),
      opt_bits("no-adapters", &to.flags, SCFQ_TRIM_NO_ADAPTERS),
      opt_flag("stats", 0, &stats),
      opt_text("out1", &out1),
      opt_text("out2", &out2),
      opt_custom("adapter", [&](std::string& v) {          // (fq-adapters' rule)
        const size_t colon = v.find(':');
        const std::string name = colon == std::string::npos ? "" : v.substr(0, colon), seq = colon == std::string::npos ? "" : v.substr(colon + 1);
        if (name.empty() || name.find('\t') != std::string::npos || seq.empty() || seq.size() > SCFQ_ADAPTERS_MAX_LEN ||
            seq.find_first_not_of("ACGT") != std::string::npos || names.size() >= SCFQ_TRIM_MAX_PROBES)
          return Reject::bad_value;
        names.push_back(name);
        seqs.push_back(seq);
        return Reject::none;
      }),
      opt_number("min-adapter-overlap", 6, 1, 32, &to.min_adapter_overlap),
      opt_number("adapter-mismatch-pct", 6, 0, 100, &to.adapter_mismatch_pct),
      opt_number("poly-g", 6, 0, SCFQ_TRIM_MAX_LEN, &to.poly_g),
      opt_number("window", 6, 1, 32, &to.window),
      opt_number("window-quality", 6, 0, 93, &to.window_quality),
      opt_number("min-length", 6, 0, SCFQ_TRIM_MAX_LEN, &to.min_length),
      opt_number("min-overlap", 6, 1, SCFQ_INSERT_MAX_LEN, &to.min_overlap),
      opt_number("max-mismatches", 6, 0, 65535, &to.max_mismatches),
      opt_number("max-mismatch-pct", 6, 0, 100, &to.max_mismatch_pct),
      opt_custom("phred-offset", [&](std::string& v) {     // a number in 33 .. 64 first, then one of the two
        uint64_t n = 0;
        if (!bounded_number(v, 6, 33, 64, &n)) return Reject::bad_value;
        to.phred_offset = (uint32_t)n;
        if (n == 33 || n == 64) return Reject::none;
        v = std::to_string(n);                             // (this message shows the number, not the text)
        return Reject::bad_value;
      }),
  };
  if (!parse_options(params, help, table, &files)) return 0;
  const bool interleaved = to.flags & SCFQ_TRIM_INTERLEAVED;
  if (files.empty()) quit_no_fastq();
  if (files.size() > 2 || (interleaved && files.size() != 1)) usage_error(help, "fq-trim takes one FASTQ, R1.fq and R2.fq, or one FASTQ with --interleaved");
  const bool two = files.size() == 2;
  if ((to.flags & SCFQ_TRIM_NO_ADAPTERS) && !names.empty()) usage_error(help, "--no-adapters goes without --adapter=NAME:SEQ");
  if (two && (out1.empty() || out2.empty())) usage_error(help, "R1.fq R2.fq write to --out1=PATH and --out2=PATH");
  if (!two && (!out1.empty() || !out2.empty())) usage_error(help, "--out1=PATH and --out2=PATH go with R1.fq R2.fq; one input is written to stdout");
  to.n_probes = (uint32_t)seqs.size();
  for (size_t j = 0; j < seqs.size(); ++j) to.probes[j] = seqs[j].c_str();
  for (const std::string& f : files) require_suffix_room(f);
  // the inputs are looked at before an output file is made
  for (const std::string& f : files)
    if (access(f.c_str(), R_OK) != 0) quit_unable_to_open(f);
  int fd1 = 1, fd2 = -1;
  // a call that fails leaves no output file behind: what this process created goes again
  auto discard = [&]() {
    // (only a regular file: a FIFO or a device the caller named is the caller's)
    auto drop = [](int fd, const std::string& p) {
      struct stat st;
      const bool regular = fstat(fd, &st) == 0 && S_ISREG(st.st_mode);
      close(fd);
      if (regular) unlink(p.c_str());
    };
    if (two && fd1 >= 0) drop(fd1, out1);
    if (two && fd2 >= 0) drop(fd2, out2);
    fd1 = fd2 = -1;
  };
  auto create = [&](const std::string& p) -> int {
    const int fd = open(p.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (fd < 0) { discard(); quit_error("Unable to create file: " + p, 1); }
    return fd;
  };
  if (two) { fd1 = -1; fd1 = create(out1); fd2 = create(out2); }
  scfq_trim_stats st = fresh<scfq_trim_stats>();
  std::fflush(stdout);
  const int rc = scfq_trim_files(files[0].c_str(), two ? files[1].c_str() : nullptr, nullptr, &to, fd1, fd2, &st);
  if (rc != SCFQ_OK && rc != SCFQ_EPIPE) discard();
  else if (two) { close(fd1); close(fd2); }
  if (rc == SCFQ_EOPEN) quit_unable_to_open(first_unopenable(files[0], two ? &files[1] : nullptr));
  if (rc == SCFQ_EPIPE) return 0;              // a reader of stdout that went away: quiet, as `sc fq-dedup | head`
  if (rc != SCFQ_OK) quit_error(library_error(rc, scfq_trim_error_detail()), 1);
  if (stats) {
    char row[1024];
    scfq_format_trim_stats_tsv(&st, row, sizeof row);
    std::fprintf(stderr, "%s\n%s\n", kTrimStatsHeader, row);
  }
  return 0;
}

// command "fq-screen" (addition, not in the reference): --ref=NAME:PATH (or --ref=PATH) up to 16 times, then IN.fq, R1.fq R2.fq or
// --interleaved IN.fq; the report goes to stdout, reads only where --out / --out1 / --out2 say; --k=N, --min-hits=N, --min-hit-pct=N,
// --keep-matched, --per-read=PATH, -t/--header, -b/--basename, -a/--absolute
static const char* kScreenHeader = "ref\tref_bases\tref_kmers\treads_in\treads\tpct_reads\tonly_reads\tbest_reads\tkmer_hits";
static int cmd_fq_screen(const std::vector<std::string>& params) {
  static const char* const help =
      "Screen reads for k-mers of reference sequences (spike-ins, vectors, rRNA, another species) and filter by it; pairs stay in step\n\nUsage:\n"
      "  fq-screen [options] --ref=NAME:PATH [--ref=...] IN.fq\n  fq-screen [options] --ref=... [--out1=PATH --out2=PATH] R1.fq R2.fq\n"
      "  fq-screen [options] --ref=... --interleaved [--out=PATH] IN.fq\n\n"
      "Arguments:\n  IN.fq            One FASTQ: single-end reads, or pairs with --interleaved\n"
      "  R1.fq R2.fq      Two FASTQs: record i of each is pair i\n\nOptions:\n"
      "      --ref=NAME:PATH        A reference FASTA (all its contigs) and its name in the report; up to 16. --ref=PATH alone:\n"
      "                             the name is the file's base name up to its first '.'\n"
      "      --k=N                  Length of the k-mers (default: 31, 8 .. 32)\n"
      "      --min-hits=N           A reference matches a read that shares N k-mers with it (default: 1, 1 .. 65535)\n"
      "      --min-hit-pct=N        ... and N percent of the read's own k-mers (default: 0, 0 .. 100)\n"
      "      --interleaved          The one argument is an interleaved FASTQ: records 2i and 2i+1 are pair i\n"
      "      --out=PATH             With one FASTQ: the reads, or pairs, that match no reference go to PATH\n"
      "      --out1=PATH            With R1.fq R2.fq: mate 1 of those pairs goes to PATH\n"
      "      --out2=PATH            With R1.fq R2.fq: mate 2 of those pairs goes to PATH\n"
      "      --keep-matched         Write the reads, or pairs, that match a reference instead\n"
      "      --per-read=PATH        One row per read to PATH: read_index kmers hit_kmers best best_hits mask\n"
      "  -t, --header               Output the header\n  -b, --basename             Add a column with the basename of the first FASTQ\n"
      "  -a, --absolute             Add a column with the absolute path of the first FASTQ\n"
      "  -h, --help                 Show this help\n";
  Columns cols;
  scfq_screen_opts so = fresh<scfq_screen_opts>();
  so.min_hits = 1;
  uint32_t k = 31;
  std::vector<std::string> files, names, paths;
  std::string out, out1, out2, per_read;
  const std::vector<Opt> table = cols.options({
      opt_custom("ref", [&](std::string& v) {
        const size_t colon = v.find(':');
        std::string name = colon == std::string::npos ? "" : v.substr(0, colon), path = colon == std::string::npos ? v : v.substr(colon + 1);
        if (colon == std::string::npos) { name = last_path_part(path); name = name.substr(0, name.find('.')); }
        if (name.empty() || name.size() > 63 || name.find('\t') != std::string::npos || name.find('\n') != std::string::npos || path.empty() ||
            names.size() >= SCFQ_SCREEN_MAX_REFS)
          return Reject::bad_value;
        for (const std::string& n : names) if (n == name) return Reject::bad_value;
        names.push_back(name);
        paths.push_back(path);
        return Reject::none;
      }),
      opt_number("k", 6, 8, SCFQ_SCREEN_MAX_K, &k),
      opt_number("min-hits", 6, 1, 65535, &so.min_hits),
      opt_number("min-hit-pct", 6, 0, 100, &so.min_hit_pct),
      opt_bits("interleaved", &so.flags, SCFQ_SCREEN_INTERLEAVED),
      opt_bits("keep-matched", &so.flags, SCFQ_SCREEN_KEEP_MATCHED),
      opt_text("out", &out),
      opt_text("out1", &out1),
      opt_text("out2", &out2),
      opt_text("per-read", &per_read),
  });
  if (!parse_options(params, help, table, &files)) return 0;
  const bool interleaved = so.flags & SCFQ_SCREEN_INTERLEAVED;
  if (names.empty()) usage_error(help, "fq-screen needs a reference: --ref=NAME:PATH");
  if (files.empty()) quit_no_fastq();
  if (files.size() > 2 || (interleaved && files.size() != 1)) usage_error(help, "fq-screen takes one FASTQ, R1.fq and R2.fq, or one FASTQ with --interleaved");
  const bool two = files.size() == 2;
  if (two && !out.empty()) usage_error(help, "R1.fq R2.fq write to --out1=PATH and --out2=PATH");
  if (two && out1.empty() != out2.empty()) usage_error(help, "--out1=PATH and --out2=PATH go together");
  if (!two && (!out1.empty() || !out2.empty())) usage_error(help, "--out1=PATH and --out2=PATH go with R1.fq R2.fq; one input is written to --out=PATH");
  for (const std::string& f : files) require_suffix_room(f);
  // the inputs and the references are looked at before an output file is made
  for (const std::string& f : files)
    if (access(f.c_str(), R_OK) != 0) quit_unable_to_open(f);
  for (const std::string& f : paths)
    if (access(f.c_str(), R_OK) != 0) quit_unable_to_open(f, 2);
  std::vector<const char*> name_ptrs, path_ptrs;
  for (size_t r = 0; r < names.size(); ++r) { name_ptrs.push_back(names[r].c_str()); path_ptrs.push_back(paths[r].c_str()); }
  scfq_screen_index* index = nullptr;
  scfq_screen_summary sum = fresh<scfq_screen_summary>();
  int rc = scfq_screen_index_files(name_ptrs.data(), path_ptrs.data(), (uint32_t)names.size(), k, nullptr, &index, &sum);
  if (rc != SCFQ_OK) quit_error(library_error(rc, scfq_screen_error_detail()), 1);
  const std::string p1 = two ? out1 : out;
  int fd1 = -1, fd2 = -1;
  // a call that fails leaves no output file behind: what this process created goes again (fq-trim's rule)
  auto discard = [&]() {
    auto drop = [](int fd, const std::string& p) {
      struct stat st;
      const bool regular = fstat(fd, &st) == 0 && S_ISREG(st.st_mode);
      close(fd);
      if (regular) unlink(p.c_str());
    };
    if (fd1 >= 0) drop(fd1, p1);
    if (fd2 >= 0) drop(fd2, out2);
    fd1 = fd2 = -1;
  };
  auto create = [&](const std::string& p) -> int {
    const int fd = open(p.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (fd < 0) { discard(); quit_error("Unable to create file: " + p, 1); }
    return fd;
  };
  if (!p1.empty()) fd1 = create(p1);
  if (two && !out2.empty()) fd2 = create(out2);
  scfq_screen_stats st = fresh<scfq_screen_stats>();
  const char* path2 = two ? files[1].c_str() : nullptr;
  std::vector<scfq_screen_rec> recs;
  if (!per_read.empty()) {
    // the table's length is the number of reads: a call without outputs tells it (the screen runs twice with --per-read)
    rc = scfq_screen_files(index, files[0].c_str(), path2, nullptr, &so, -1, -1, nullptr, 0, &st);
    if (rc == SCFQ_OK) recs.assign((size_t)st.reads_in, scfq_screen_rec());
    st = fresh<scfq_screen_stats>();
  }
  if (rc == SCFQ_OK) rc = scfq_screen_files(index, files[0].c_str(), path2, nullptr, &so, fd1, fd2, recs.empty() ? nullptr : recs.data(), recs.size(), &st);
  if (rc != SCFQ_OK) discard();
  else { if (fd1 >= 0) close(fd1); if (fd2 >= 0) close(fd2); }
  if (rc == SCFQ_EOPEN) quit_unable_to_open(first_unopenable(files[0], two ? &files[1] : nullptr));
  if (rc != SCFQ_OK) quit_error(library_error(rc, scfq_screen_error_detail()), 1);
  if (!per_read.empty()) {
    FILE* f = std::fopen(per_read.c_str(), "w");
    if (!f) quit_error("Unable to create file: " + per_read, 1);
    for (size_t i = 0; i < recs.size(); ++i)
      std::fprintf(f, "%zu\t%u\t%u\t%s\t%u\t%u\n", i, recs[i].kmers, recs[i].hit_kmers, recs[i].best == 0xFF ? "-" : scfq_screen_ref_name(index, recs[i].best),
                   recs[i].best_hits, (unsigned)recs[i].mask);
    if (std::fclose(f) != 0) quit_error("Unable to write file: " + per_read, 1);
  }
  if (cols.header) std::printf("%s\n", output_header(kScreenHeader, cols.basename, cols.absolute).c_str());
  for (uint32_t r = 0; r <= names.size(); ++r) {
    char row[1024];
    scfq_format_screen_row_tsv(&st, index, r, row, sizeof row);
    cols.emit_row(row, files[0]);
  }
  scfq_screen_index_free(index);
  return 0;
}

// command "fq-demux" (addition, not in the reference): --sheet=PATH or --sample=NAME:BC1[+BC2] (up to 1024 times), then IN.fq, R1.fq R2.fq
// or --interleaved IN.fq; the report goes to stdout, a row per sample and a last row "undetermined"; reads only where --out-dir=DIR
// says (a file per sample and mate); --barcodes=inline|header, --mismatches=N, --keep-barcode, --per-read=PATH, -t/--header,
// -b/--basename, -a/--absolute
static const char* kDemuxHeader = "sample\tbarcode\tunits\tpct_units\tperfect\tmismatched\tbases_out\tbytes1\tbytes2";
static int cmd_fq_demux(const std::vector<std::string>& params) {
  static const char* const help =
      "Split the reads of a pooled run by sample barcode; pairs stay in step\n\nUsage:\n"
      "  fq-demux [options] (--sheet=PATH | --sample=NAME:BC1[+BC2] ...) [--out-dir=DIR] IN.fq\n"
      "  fq-demux [options] (--sheet=PATH | --sample=...) [--out-dir=DIR] R1.fq R2.fq\n"
      "  fq-demux [options] (--sheet=PATH | --sample=...) --interleaved [--out-dir=DIR] IN.fq\n\n"
      "Arguments:\n  IN.fq            One FASTQ: single-end reads, or pairs with --interleaved\n"
      "  R1.fq R2.fq      Two FASTQs: record i of each is pair i\n\nOptions:\n"
      "      --sheet=PATH           The samples, one per line: name<TAB>barcode1[<TAB>barcode2]; '#' lines and blank lines are skipped\n"
      "      --sample=NAME:BC1[+BC2]  One sample; up to 1024, instead of --sheet\n"
      "      --out-dir=DIR          An existing directory: NAME.fq per sample and undetermined.fq, or NAME_R1.fq and NAME_R2.fq\n"
      "                             with R1.fq R2.fq. Without it only the report is made\n"
      "      --barcodes=inline|header  Where the barcode is read: the first bases of the read (mate 2 for the second barcode), or\n"
      "                             the header behind its last ':' (BC1+BC2) (default: inline)\n"
      "      --mismatches=N         Mismatches allowed per barcode (default: 1, 0 .. 3)\n"
      "      --keep-barcode         Inline barcodes stay in the written reads\n"
      "      --interleaved          The one argument is an interleaved FASTQ: records 2i and 2i+1 are pair i\n"
      "      --per-read=PATH        One row per read, or pair, to PATH: unit sample mm1 mm2 state\n"
      "  -t, --header               Output the header\n  -b, --basename             Add a column with the basename of the first FASTQ\n"
      "  -a, --absolute             Add a column with the absolute path of the first FASTQ\n"
      "  -h, --help                 Show this help\n";
  Columns cols;
  scfq_demux_opts dopts = fresh<scfq_demux_opts>();
  dopts.mismatches = 1;
  std::vector<std::string> files, names, bc1, bc2;
  std::vector<char> has2;
  std::string sheet_path, out_dir, per_read;
  const std::vector<Opt> table = cols.options({
      opt_text("sheet", &sheet_path),
      opt_custom("sample", [&](std::string& v) {
        const size_t colon = v.find(':');
        if (colon == std::string::npos || colon == 0 || colon + 1 == v.size() || names.size() >= SCFQ_DEMUX_MAX_SAMPLES) return Reject::bad_value;
        const std::string bc = v.substr(colon + 1);
        const size_t plus = bc.find('+');
        names.push_back(v.substr(0, colon));
        bc1.push_back(bc.substr(0, plus));
        bc2.push_back(plus == std::string::npos ? "" : bc.substr(plus + 1));
        has2.push_back(plus != std::string::npos);
        return Reject::none;
      }),
      opt_text("out-dir", &out_dir),
      opt_custom("barcodes", [&](std::string& v) {
        if (v == "header") dopts.flags |= SCFQ_DEMUX_HEADER;
        else if (v == "inline") dopts.flags &= ~SCFQ_DEMUX_HEADER;
        else return Reject::bad_value;
        return Reject::none;
      }),
      opt_number("mismatches", 1, 0, 3, &dopts.mismatches),
      opt_bits("keep-barcode", &dopts.flags, SCFQ_DEMUX_KEEP_BARCODE),
      opt_bits("interleaved", &dopts.flags, SCFQ_DEMUX_INTERLEAVED),
      opt_text("per-read", &per_read),
  });
  if (!parse_options(params, help, table, &files)) return 0;
  const bool interleaved = dopts.flags & SCFQ_DEMUX_INTERLEAVED;
  if (sheet_path.empty() == names.empty()) usage_error(help, "fq-demux needs its samples: --sheet=PATH, or --sample=NAME:BC1[+BC2] once per sample");
  if (files.empty()) quit_no_fastq();
  if (files.size() > 2 || (interleaved && files.size() != 1)) usage_error(help, "fq-demux takes one FASTQ, R1.fq and R2.fq, or one FASTQ with --interleaved");
  const bool two = files.size() == 2;
  for (const std::string& f : files) require_suffix_room(f);
  // the inputs, the sheet and the directory are looked at before an output file is made
  for (const std::string& f : files)
    if (access(f.c_str(), R_OK) != 0) quit_unable_to_open(f);
  if (!sheet_path.empty()) {
    FILE* f = std::fopen(sheet_path.c_str(), "r");
    if (!f) quit_unable_to_open(sheet_path, 2);
    std::string line;
    size_t line_no = 0;
    for (int c = 0; c != EOF;) {
      line.clear();
      while ((c = std::fgetc(f)) != EOF && c != '\n') line += (char)c;
      ++line_no;
      if (!line.empty() && line.back() == '\r') line.pop_back();
      if (line.empty() || line[0] == '#') continue;
      std::vector<std::string> cell(1);
      for (char ch : line) { if (ch == '\t') cell.emplace_back(); else cell.back() += ch; }
      if (cell.size() < 2 || cell.size() > 3 || names.size() >= SCFQ_DEMUX_MAX_SAMPLES) {
        std::fclose(f);
        quit_error(sheet_path + ": line " + std::to_string(line_no) + " is not name<TAB>barcode1[<TAB>barcode2], or is sample " +
                   std::to_string(SCFQ_DEMUX_MAX_SAMPLES + 1), 1);
      }
      names.push_back(cell[0]);
      bc1.push_back(cell[1]);
      bc2.push_back(cell.size() == 3 ? cell[2] : "");
      has2.push_back(cell.size() == 3);
    }
    std::fclose(f);
    if (names.empty()) quit_error(sheet_path + ": no sample", 1);
  }
  std::vector<scfq_demux_sample> samples(names.size());
  for (size_t s = 0; s < names.size(); ++s) samples[s] = scfq_demux_sample{names[s].c_str(), bc1[s].c_str(), has2[s] ? bc2[s].c_str() : nullptr};
  scfq_demux_sheet* sheet = nullptr;
  int rc = scfq_demux_sheet_new(samples.data(), (uint32_t)samples.size(), &sheet);
  if (rc != SCFQ_OK) quit_error(library_error(rc, scfq_demux_error_detail()), 1);
  if (!out_dir.empty()) {
    struct stat sb;
    if (stat(out_dir.c_str(), &sb) != 0 || !S_ISDIR(sb.st_mode)) quit_error("Not a directory: " + out_dir, 1);
  }
  const char* path2 = two ? files[1].c_str() : nullptr;
  const char* dir = out_dir.empty() ? nullptr : out_dir.c_str();
  std::vector<scfq_demux_row> rows(samples.size() + 1);
  scfq_demux_stats st = fresh<scfq_demux_stats>();
  std::vector<scfq_demux_rec> recs;
  if (!per_read.empty()) {
    // the table's length is the number of units: a call without outputs tells it (the assignment runs twice with --per-read)
    rc = scfq_demux_files(sheet, files[0].c_str(), path2, nullptr, &dopts, nullptr, nullptr, 0, rows.data(), rows.size(), &st);
    if (rc == SCFQ_OK) recs.assign((size_t)st.units_in, scfq_demux_rec());
    st = fresh<scfq_demux_stats>();
  }
  if (rc == SCFQ_OK)
    rc = scfq_demux_files(sheet, files[0].c_str(), path2, nullptr, &dopts, dir, recs.empty() ? nullptr : recs.data(), recs.size(), rows.data(), rows.size(), &st);
  if (rc == SCFQ_EOPEN) quit_unable_to_open(first_unopenable(files[0], two ? &files[1] : nullptr));
  if (rc != SCFQ_OK) quit_error(library_error(rc, scfq_demux_error_detail()), 1);
  if (!per_read.empty()) {
    static const char* const kState[4] = {"assigned", "unmatched", "ambiguous", "no_barcode"};
    FILE* f = std::fopen(per_read.c_str(), "w");
    if (!f) quit_error("Unable to create file: " + per_read, 1);
    for (size_t u = 0; u < recs.size(); ++u) {
      const bool assigned = recs[u].state == SCFQ_DEMUX_ASSIGNED;
      if (assigned) std::fprintf(f, "%zu\t%s\t%u\t%u\t%s\n", u, scfq_demux_sheet_name(sheet, recs[u].sample), (unsigned)recs[u].mm1, (unsigned)recs[u].mm2, kState[0]);
      else std::fprintf(f, "%zu\t-\t-\t-\t%s\n", u, kState[recs[u].state & 3u]);
    }
    if (std::fclose(f) != 0) quit_error("Unable to write file: " + per_read, 1);
  }
  if (cols.header) std::printf("%s\n", output_header(kDemuxHeader, cols.basename, cols.absolute).c_str());
  for (uint32_t d = 0; d <= samples.size(); ++d) {
    char row[1024];
    scfq_format_demux_row_tsv(&st, sheet, d, &rows[d], row, sizeof row);
    cols.emit_row(row, files[0]);
  }
  scfq_demux_sheet_free(sheet);
  return 0;
}

// command "fq-kmers" (addition, not in the reference): -t/--header, -b/--basename, -a/--absolute as fq-count, --k=N, --canonical, --top=N,
// --totals, [fastq ...]
static const char* kKmersHeader = "kmer\tcount";
static const char* kKmersTotalsHeader = "k\twindows\tkmers\tskipped\tshort_lines\tdistinct\tmax_count";
static int cmd_fq_kmers(const std::vector<std::string>& params) {
  static const char* const help =
      "K-mer spectrum of the sequence lines of a FASTQ\n\nUsage:\n  fq-kmers [options] [fastq ...]\n\nArguments:\n"
      "  [fastq ...]      Input FASTQ\n\nOptions:\n  -t, --header               Output the header\n"
      "  -b, --basename             Add basename column\n  -a, --absolute             Add column for absolute path\n"
      "      --k=N                  Length of the k-mers, 1 .. 12 (default: 7); only windows of A C G T count\n"
      "      --canonical            Count a k-mer and its reverse complement as the smaller of the two\n"
      "      --top=N                The N largest counts, ties in k-mer order (default: every k-mer that occurs, in\n"
      "                             k-mer order)\n"
      "      --totals               One row per file instead: k windows kmers skipped short_lines distinct max_count\n"
      "  -h, --help                 Show this help\n";
  const uint64_t kNoTop = ~0ull;          // (more than the 18 digits of --top=N can say)
  Columns cols;
  bool totals = false;
  uint32_t k = 7, flags = 0;
  uint64_t top = kNoTop;
  std::vector<std::string> files;
  const std::vector<Opt> options = cols.options({
      opt_number("k", 18, 1, SCFQ_KMERS_MAX_K, &k),
      opt_bits("canonical", &flags, SCFQ_KMERS_CANONICAL),
      opt_number("top", 18, 0, ~0ull, &top),
      opt_flag("totals", 0, &totals),
  });
  if (!parse_options(params, help, options, &files)) return 0;
  cols.header_or_no_input(totals ? kKmersTotalsHeader : kKmersHeader, files.empty());
  const uint64_t entries = 1ull << (2 * k);
  std::vector<uint64_t> table(totals ? 0 : entries);
  std::vector<uint64_t> order;
  for (const auto& fastq : files) {
    require_suffix_room(fastq);
    scfq_kmer_summary s = fresh<scfq_kmer_summary>();
    const int rc = scfq_kmers_file(fastq.c_str(), nullptr, k, flags, table.empty() ? nullptr : table.data(), table.size(), &s);
    if (rc == SCFQ_EOPEN) quit_unable_to_open(fastq);
    if (rc != SCFQ_OK) quit_error(library_error(rc, scfq_kmers_error_detail()), 1);
    char row[64];
    if (totals) {
      const std::string line = std::to_string(s.k) + "\t" + std::to_string(s.windows) + "\t" + std::to_string(s.kmers) + "\t" +
                               std::to_string(s.skipped) + "\t" + std::to_string(s.short_lines) + "\t" + std::to_string(s.distinct) + "\t" +
                               std::to_string(s.max_count);
      cols.emit_row(line, fastq);
      continue;
    }
    order.clear();
    for (uint64_t e = 0; e < entries; ++e) if (table[e]) order.push_back(e);
    if (top != kNoTop) {
      // the N largest counts, ties by ascending index (order is ascending already)
      const size_t keep = (size_t)std::min<uint64_t>(top, order.size());
      std::partial_sort(order.begin(), order.begin() + keep, order.end(),
                        [&](uint64_t a, uint64_t b) { return table[a] != table[b] ? table[a] > table[b] : a < b; });
      order.resize(keep);
    }
    for (const uint64_t e : order) {
      scfq_format_kmer_tsv(k, e, table[e], row, sizeof row);
      cols.emit_row(row, fastq);
    }
  }
  std::fflush(stdout);
  return 0;
}

// command "fq-normalize" (addition, not in the reference): IN.fq (the kept reads to stdout, or to --out=PATH), R1.fq R2.fq with
// --out1=PATH --out2=PATH (or neither: the report only), or --interleaved IN.fq; --k=N, --plain, --target=N, --min-depth=N, --weak-below=N,
// --seed=N, --keep-no-kmers, --table-bits=N, --stats, --hist[=BINS], --per-read=PATH, -t/--header, -b/--basename, -a/--absolute.  The
// report goes to stdout, or to stderr while stdout carries the reads.
static const char* kNormHistHeader = "depth\tunits_in\tunits_out";
static int cmd_fq_normalize(const std::vector<std::string>& params) {
  static const char* const help =
      "Normalize reads by the depth of their k-mers: thin over-covered regions to a target depth, drop reads of rare k-mers; pairs stay in step\n\n"
      "Usage:\n  fq-normalize [options] IN.fq > out.fq\n  fq-normalize [options] --out1=PATH --out2=PATH R1.fq R2.fq\n"
      "  fq-normalize [options] --interleaved [--out=PATH] IN.fq\n\n"
      "Arguments:\n  IN.fq            One FASTQ: single-end reads, or pairs with --interleaved; the kept reads go to stdout or to --out=PATH\n"
      "  R1.fq R2.fq      Two FASTQs: record i of each is pair i; without --out1 and --out2 only the report is produced\n\nOptions:\n"
      "      --k=N                  Length of the k-mers, 13 .. 32 (default: 21); the inputs are counted first, then normalized\n"
      "      --plain                Count a k-mer and its reverse complement apart (default: as the smaller of the two)\n"
      "      --target=N             Thin units whose depth D is above N to about N (default: 0 = off)\n"
      "      --min-depth=N          Drop units with D below N (default: 0)\n"
      "      --weak-below=N         Count k-mers that occur fewer than N times as weak (default: 2, 0 = none)\n"
      "      --seed=N               Seed of the thinning (default: 0)\n"
      "      --keep-no-kmers        Keep the units that have no k-mer at all\n"
      "      --table-bits=N         A table of 2^N slots, 10 .. 32, that does not grow (default: sized by the input)\n"
      "      --interleaved          The one argument is an interleaved FASTQ: records 2i and 2i+1 are pair i\n"
      "      --out=PATH             With one FASTQ: the kept reads, or pairs, go to PATH and the report to stdout\n"
      "      --out1=PATH            With R1.fq R2.fq: mate 1 of the kept pairs goes to PATH\n"
      "      --out2=PATH            With R1.fq R2.fq: mate 2 of the kept pairs goes to PATH\n"
      "      --stats                While stdout carries the reads: the report row to stderr\n"
      "      --hist[=BINS]          Instead of the report row the table \"depth units_in units_out\", the last bin gathering\n"
      "                             D >= BINS - 1 (default: 1002, 2 .. 1048576)\n"
      "      --per-read=PATH        One row per read to PATH: read_index kmers depth min_count weak\n"
      "  -t, --header               Output the header\n  -b, --basename             Add a column with the basename of the first FASTQ\n"
      "  -a, --absolute             Add a column with the absolute path of the first FASTQ\n"
      "  -h, --help                 Show this help\n";
  Columns cols;
  scfq_norm_opts no = fresh<scfq_norm_opts>();
  no.k = 21;
  no.weak_below = 2;
  uint32_t plain = 0;
  bool stats = false, hist = false;
  uint64_t bins = 1002;
  std::vector<std::string> files;
  std::string out, out1, out2, per_read;
  const std::vector<Opt> table = cols.options({
      opt_number("k", 6, SCFQ_KCOUNT_MIN_K, SCFQ_KCOUNT_MAX_K, &no.k),
      opt_bits("plain", &plain, 1u),
      opt_number("target", 10, 0, SCFQ_NORM_MAX_DEPTH, &no.target),
      opt_number("min-depth", 10, 0, SCFQ_NORM_MAX_DEPTH, &no.min_depth),
      opt_number("weak-below", 10, 0, SCFQ_NORM_MAX_DEPTH, &no.weak_below),
      opt_custom("seed", [&](std::string& v) {             // all of 64 bits: twenty digits may be too many
        if (v.empty() || v.size() > 20 || v.find_first_not_of("0123456789") != std::string::npos) return Reject::bad_value;
        uint64_t n = 0;
        for (const char c : v) {
          if (n > (~0ull - (uint64_t)(c - '0')) / 10) return Reject::bad_value;
          n = 10 * n + (uint64_t)(c - '0');
        }
        no.seed = n;
        return Reject::none;
      }),
      opt_bits("keep-no-kmers", &no.flags, SCFQ_NORM_KEEP_NO_KMERS),
      opt_number("table-bits", 6, 10, 32, &no.table_bits),
      opt_bits("interleaved", &no.flags, SCFQ_NORM_INTERLEAVED),
      opt_text("out", &out),
      opt_text("out1", &out1),
      opt_text("out2", &out2),
      opt_flag("stats", 0, &stats),
      opt_flag("hist", 0, &hist),
      opt_custom("hist", [&](std::string& v) {
        hist = true;
        return bounded_number(v, 7, 2, SCFQ_NORM_MAX_BINS, &bins) ? Reject::none : Reject::bad_value;
      }),
      opt_text("per-read", &per_read),
  });
  if (!parse_options(params, help, table, &files)) return 0;
  no.table_flags = plain ? 0u : (uint32_t)SCFQ_KCOUNT_CANONICAL;
  const bool interleaved = no.flags & SCFQ_NORM_INTERLEAVED;
  if (files.empty()) quit_no_fastq();
  if (files.size() > 2 || (interleaved && files.size() != 1)) usage_error(help, "fq-normalize takes one FASTQ, R1.fq and R2.fq, or one FASTQ with --interleaved");
  const bool two = files.size() == 2;
  if (two && !out.empty()) usage_error(help, "R1.fq R2.fq write to --out1=PATH and --out2=PATH");
  if (two && out1.empty() != out2.empty()) usage_error(help, "--out1=PATH and --out2=PATH go together");
  if (!two && (!out1.empty() || !out2.empty())) usage_error(help, "--out1=PATH and --out2=PATH go with R1.fq R2.fq; one input is written to stdout or to --out=PATH");
  for (const std::string& f : files) require_suffix_room(f);
  // the inputs are looked at before an output file is made
  for (const std::string& f : files)
    if (access(f.c_str(), R_OK) != 0) quit_unable_to_open(f);
  const bool to_stdout = !two && out.empty();          // stdout carries the reads: the report goes to stderr
  const std::string p1 = two ? out1 : out;
  int fd1 = to_stdout ? 1 : -1, fd2 = -1;
  // a call that fails leaves no output file behind: what this process created goes again (fq-trim's rule)
  auto discard = [&]() {
    auto drop = [](int fd, const std::string& p) {
      struct stat st;
      const bool regular = fstat(fd, &st) == 0 && S_ISREG(st.st_mode);
      close(fd);
      if (regular) unlink(p.c_str());
    };
    if (!to_stdout && fd1 >= 0) drop(fd1, p1);
    if (fd2 >= 0) drop(fd2, out2);
    fd1 = fd2 = -1;
  };
  auto create = [&](const std::string& p) -> int {
    const int fd = open(p.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (fd < 0) { discard(); quit_error("Unable to create file: " + p, 1); }
    return fd;
  };
  if (!p1.empty()) fd1 = create(p1);
  if (two && !out2.empty()) fd2 = create(out2);
  scfq_norm_stats st = fresh<scfq_norm_stats>();
  const char* path2 = two ? files[1].c_str() : nullptr;
  std::vector<scfq_norm_rec> recs;
  std::vector<uint64_t> bin_words(hist ? 2 * bins : 0);
  scfq_kcount* kc = nullptr;
  int rc = SCFQ_OK;
  bool counting = false;
  if (!per_read.empty()) {
    // the per-read table's length is the number of reads: the inputs are counted into a table that stays, and a call without outputs
    // tells the length
    scfq_kcount_opts ko = fresh<scfq_kcount_opts>();
    ko.k = no.k; ko.flags = no.table_flags; ko.table_bits = no.table_bits;
    counting = true;
    rc = scfq_kcount_files(files[0].c_str(), path2, nullptr, &ko, &kc, nullptr);
    if (rc == SCFQ_OK) {
      counting = false;
      rc = scfq_norm_files(kc, files[0].c_str(), path2, nullptr, &no, -1, -1, nullptr, 0, nullptr, 0, &st);
    }
    if (rc == SCFQ_OK) recs.assign((size_t)st.reads_in, scfq_norm_rec());
    st = fresh<scfq_norm_stats>();
  }
  std::fflush(stdout);
  if (rc == SCFQ_OK)
    rc = scfq_norm_files(kc, files[0].c_str(), path2, nullptr, &no, fd1, fd2, recs.empty() ? nullptr : recs.data(), recs.size(), hist ? bin_words.data() : nullptr,
                         hist ? bins : 0, &st);
  const std::string detail = counting ? scfq_kcount_error_detail() : scfq_norm_error_detail();
  scfq_kcount_free(kc);
  if (rc != SCFQ_OK && rc != SCFQ_EPIPE) discard();
  else { if (!to_stdout && fd1 >= 0) close(fd1); if (fd2 >= 0) close(fd2); }
  if (rc == SCFQ_EOPEN) quit_unable_to_open(first_unopenable(files[0], two ? &files[1] : nullptr));
  if (rc == SCFQ_EPIPE) return 0;              // a reader of stdout that went away: quiet, as `sc fq-dedup | head`
  if (rc != SCFQ_OK) quit_error(library_error(rc, detail.c_str()), 1);
  if (!per_read.empty()) {
    FILE* f = std::fopen(per_read.c_str(), "w");
    if (!f) quit_error("Unable to create file: " + per_read, 1);
    for (size_t i = 0; i < recs.size(); ++i) std::fprintf(f, "%zu\t%u\t%u\t%u\t%u\n", i, recs[i].kmers, recs[i].depth, recs[i].min_count, recs[i].weak);
    if (std::fclose(f) != 0) quit_error("Unable to write file: " + per_read, 1);
  }
  FILE* report = to_stdout ? stderr : stdout;
  if (to_stdout && !stats && !hist) return 0;
  char row[1024];
  if (cols.header) {
    scfq_format_norm_row_tsv(nullptr, 1, row, sizeof row);
    std::fprintf(report, "%s\n", output_header(hist ? kNormHistHeader : row, cols.basename, cols.absolute).c_str());
  }
  if (hist) {
    for (uint64_t d = 0; d < bins; ++d) {
      scfq_format_norm_hist_tsv(d, bin_words[2 * d], bin_words[2 * d + 1], row, sizeof row);
      std::fprintf(report, "%s\n", cols.row(row, files[0]).c_str());
    }
  } else {
    scfq_format_norm_row_tsv(&st, 0, row, sizeof row);
    std::fprintf(report, "%s\n", cols.row(row, files[0]).c_str());
  }
  return 0;
}

// command "fq-complexity" (addition, not in the reference): IN.fq, R1.fq R2.fq with --out1=PATH --out2=PATH (or neither: the report
// only), or --interleaved IN.fq; --window=N, --threshold=N, --mask=lower|n|none, --max-masked-pct=N, --report, --stats, --hist,
// --per-read=PATH, --out=PATH, -t/--header, -b/--basename, -a/--absolute.  The report goes to stdout, or to stderr while stdout carries the reads.
static const char* kCplxHistHeader = "score\treads";
static int cmd_fq_complexity(const std::vector<std::string>& params) {
  static const char* const help =
      "Mask and filter low-complexity sequence (symmetric DUST): homopolymer runs, microsatellites and other short-period repeats inside reads\n\n"
      "Usage:\n  fq-complexity [options] IN.fq > out.fq\n  fq-complexity [options] --out1=PATH --out2=PATH R1.fq R2.fq\n"
      "  fq-complexity [options] --interleaved IN.fq > out.fq\n\n"
      "Arguments:\n  IN.fq            One FASTQ: single-end reads, or pairs with --interleaved; the kept reads go to stdout or to --out=PATH\n"
      "  R1.fq R2.fq      Two FASTQs: record i of each is pair i; without --out1 and --out2 only the report is produced\n\nOptions:\n"
      "      --window=N             Longest interval that is scored, in bases, 8 .. 64 (default: 64)\n"
      "      --threshold=N          An interval is low-complexity when ten times its score is above N, 1 .. 310 (default: 20)\n"
      "      --mask=lower|n|none    Masked bases become lower case, become N, or stay as they are (default: lower)\n"
      "      --max-masked-pct=N     Drop a read, or a pair with such a mate, when more than N percent of it is masked (default: 100)\n"
      "      --interleaved          The one argument is an interleaved FASTQ: records 2i and 2i+1 are pair i\n"
      "      --out=PATH             With one FASTQ: the kept reads, or pairs, go to PATH and the report to stdout\n"
      "      --out1=PATH            With R1.fq R2.fq: mate 1 of the kept pairs goes to PATH\n"
      "      --out2=PATH            With R1.fq R2.fq: mate 2 of the kept pairs goes to PATH\n"
      "      --report               No reads are written: the one-row report on stdout\n"
      "      --stats                While stdout carries the reads: the report row to stderr\n"
      "      --hist                 Instead of the report row the table \"score reads\"; the reads that are too long in a last row\n"
      "      --per-read=PATH        One row per read to PATH: read length score masked first intervals\n"
      "  -t, --header               Output the header\n  -b, --basename             Add a column with the basename of the first FASTQ\n"
      "  -a, --absolute             Add a column with the absolute path of the first FASTQ\n"
      "  -h, --help                 Show this help\n";
  Columns cols;
  scfq_cplx_opts co = fresh<scfq_cplx_opts>();
  co.window = 64;
  co.threshold = 20;
  co.mask = SCFQ_CPLX_MASK_LOWER;
  co.max_masked_pct = 100;
  bool stats = false, hist = false, report_only = false;
  std::vector<std::string> files;
  std::string out, out1, out2, per_read;
  const std::vector<Opt> table = cols.options({
      opt_number("window", 6, 8, 64, &co.window),
      opt_number("threshold", 6, 1, 310, &co.threshold),
      opt_custom("mask", [&](std::string& v) {
        if (v == "lower") co.mask = SCFQ_CPLX_MASK_LOWER;
        else if (v == "n") co.mask = SCFQ_CPLX_MASK_N;
        else if (v == "none") co.mask = SCFQ_CPLX_MASK_NONE;
        else return Reject::bad_value;
        return Reject::none;
      }),
      opt_number("max-masked-pct", 6, 0, 100, &co.max_masked_pct),
      opt_bits("interleaved", &co.flags, SCFQ_CPLX_INTERLEAVED),
      opt_text("out", &out),
      opt_text("out1", &out1),
      opt_text("out2", &out2),
      opt_flag("report", 0, &report_only),
      opt_flag("stats", 0, &stats),
      opt_flag("hist", 0, &hist),
      opt_text("per-read", &per_read),
  });
  if (!parse_options(params, help, table, &files)) return 0;
  const bool interleaved = co.flags & SCFQ_CPLX_INTERLEAVED;
  if (files.empty()) quit_no_fastq();
  if (files.size() > 2 || (interleaved && files.size() != 1)) usage_error(help, "fq-complexity takes one FASTQ, R1.fq and R2.fq, or one FASTQ with --interleaved");
  const bool two = files.size() == 2;
  if (two && !out.empty()) usage_error(help, "R1.fq R2.fq write to --out1=PATH and --out2=PATH");
  if (two && out1.empty() != out2.empty()) usage_error(help, "--out1=PATH and --out2=PATH go together");
  if (!two && (!out1.empty() || !out2.empty())) usage_error(help, "--out1=PATH and --out2=PATH go with R1.fq R2.fq; one input is written to stdout or to --out=PATH");
  if (report_only && (!out.empty() || !out1.empty())) usage_error(help, "--report writes no reads: it goes without --out, --out1 and --out2");
  for (const std::string& f : files) require_suffix_room(f);
  // the inputs are looked at before an output file is made
  for (const std::string& f : files)
    if (access(f.c_str(), R_OK) != 0) quit_unable_to_open(f);
  const bool to_stdout = !two && out.empty() && !report_only;      // stdout carries the reads: the report goes to stderr
  const std::string p1 = two ? out1 : out;
  int fd1 = to_stdout ? 1 : -1, fd2 = -1, fdr = -1;
  // a call that fails leaves no output file behind: what this process created goes again (fq-trim's rule)
  auto discard = [&]() {
    auto drop = [](int fd, const std::string& p) {
      struct stat st;
      const bool regular = fstat(fd, &st) == 0 && S_ISREG(st.st_mode);
      close(fd);
      if (regular) unlink(p.c_str());
    };
    if (!to_stdout && fd1 >= 0) drop(fd1, p1);
    if (fd2 >= 0) drop(fd2, out2);
    if (fdr >= 0) drop(fdr, per_read);
    fd1 = fd2 = fdr = -1;
  };
  auto create = [&](const std::string& p) -> int {
    const int fd = open(p.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (fd < 0) { discard(); quit_error("Unable to create file: " + p, 1); }
    return fd;
  };
  if (!p1.empty()) fd1 = create(p1);
  if (two && !out2.empty()) fd2 = create(out2);
  if (!per_read.empty()) fdr = create(per_read);
  scfq_cplx_stats st = fresh<scfq_cplx_stats>();
  std::vector<uint64_t> bins(SCFQ_CPLX_SCORE_BINS);
  std::fflush(stdout);
  const int rc = scfq_cplx_files(files[0].c_str(), two ? files[1].c_str() : nullptr, nullptr, &co, fd1, fd2, fdr, bins.data(), &st);
  if (rc != SCFQ_OK && rc != SCFQ_EPIPE) discard();
  else { if (!to_stdout && fd1 >= 0) close(fd1); if (fd2 >= 0) close(fd2); if (fdr >= 0) close(fdr); }
  if (rc == SCFQ_EOPEN) quit_unable_to_open(first_unopenable(files[0], two ? &files[1] : nullptr));
  if (rc == SCFQ_EPIPE) return 0;              // a reader of stdout that went away: quiet, as `sc fq-dedup | head`
  if (rc != SCFQ_OK) quit_error(library_error(rc, scfq_cplx_error_detail()), 1);
  FILE* report = to_stdout ? stderr : stdout;
  if (to_stdout && !stats && !hist) return 0;
  char row[1024];
  if (cols.header) {
    scfq_format_cplx_stats_tsv(nullptr, 1, row, sizeof row);
    std::fprintf(report, "%s\n", output_header(hist ? kCplxHistHeader : row, cols.basename, cols.absolute).c_str());
  }
  if (hist) {
    for (uint64_t s = 0; s < SCFQ_CPLX_SCORE_BINS; ++s) {
      if (!bins[s]) continue;
      if (s + 1 < SCFQ_CPLX_SCORE_BINS) std::snprintf(row, sizeof row, "%llu\t%llu", (unsigned long long)s, (unsigned long long)bins[s]);
      else std::snprintf(row, sizeof row, "too_long\t%llu", (unsigned long long)bins[s]);
      std::fprintf(report, "%s\n", cols.row(row, files[0]).c_str());
    }
  } else {
    scfq_format_cplx_stats_tsv(&st, 0, row, sizeof row);
    std::fprintf(report, "%s\n", cols.row(row, files[0]).c_str());
  }
  return 0;
}

// command "fq-rmdup" (addition, not in the reference): IN.fq, R1.fq R2.fq with --out1=PATH --out2=PATH (or neither: the report only), or
// --interleaved IN.fq; --prefix=N, --swapped, --report, --stats, --hist, --per-read=PATH, --out=PATH, -t/--header, -b/--basename,
// -a/--absolute.  The forms and output rules are fq-complexity's: the report goes to stdout, or to stderr while stdout carries the reads.
static const char* kRmdupHistHeader = "copies\tclasses\tunits";
static int cmd_fq_rmdup(const std::vector<std::string>& params) {
  static const char* const help =
      "Remove duplicate reads and pairs by sequence: of the units with the same sequence text(s) the first in input order is kept\n\n"
      "Usage:\n  fq-rmdup [options] IN.fq > out.fq\n  fq-rmdup [options] --out1=PATH --out2=PATH R1.fq R2.fq\n"
      "  fq-rmdup [options] --interleaved IN.fq > out.fq\n\n"
      "Arguments:\n  IN.fq            One FASTQ: single-end reads, or pairs with --interleaved; the kept reads go to stdout or to --out=PATH\n"
      "  R1.fq R2.fq      Two FASTQs: record i of each is pair i; without --out1 and --out2 only the report is produced\n\nOptions:\n"
      "      --prefix=N             Compare the first N bytes of every sequence, 1 .. 65535 (default: 0, the whole sequence)\n"
      "      --swapped              Pairs: (a, b) and (b, a) are duplicates too, the same fragment read from the other strand\n"
      "      --interleaved          The one argument is an interleaved FASTQ: records 2i and 2i+1 are pair i\n"
      "      --out=PATH             With one FASTQ: the kept reads, or pairs, go to PATH and the report to stdout\n"
      "      --out1=PATH            With R1.fq R2.fq: mate 1 of the kept pairs goes to PATH\n"
      "      --out2=PATH            With R1.fq R2.fq: mate 2 of the kept pairs goes to PATH\n"
      "      --report               No reads are written: the one-row report on stdout\n"
      "      --stats                While stdout carries the reads: the report row to stderr\n"
      "      --hist                 Instead of the report row the table \"copies classes units\"; the classes of 1024 and more in a last row\n"
      "      --per-read=PATH        One row per read, or pair, to PATH: unit rep copies\n"
      "  -t, --header               Output the header\n  -b, --basename             Add a column with the basename of the first FASTQ\n"
      "  -a, --absolute             Add a column with the absolute path of the first FASTQ\n"
      "  -h, --help                 Show this help\n";
  Columns cols;
  scfq_rmdup_opts co = fresh<scfq_rmdup_opts>();
  bool stats = false, hist = false, report_only = false;
  std::vector<std::string> files;
  std::string out, out1, out2, per_read;
  const std::vector<Opt> table = cols.options({
      opt_number("prefix", 6, 0, SCFQ_RMDUP_MAX_PREFIX, &co.prefix),
      opt_bits("swapped", &co.flags, SCFQ_RMDUP_SWAPPED),
      opt_bits("interleaved", &co.flags, SCFQ_RMDUP_INTERLEAVED),
      opt_text("out", &out),
      opt_text("out1", &out1),
      opt_text("out2", &out2),
      opt_flag("report", 0, &report_only),
      opt_flag("stats", 0, &stats),
      opt_flag("hist", 0, &hist),
      opt_text("per-read", &per_read),
  });
  if (!parse_options(params, help, table, &files)) return 0;
  const bool interleaved = co.flags & SCFQ_RMDUP_INTERLEAVED;
  if (files.empty()) quit_no_fastq();
  if (files.size() > 2 || (interleaved && files.size() != 1)) usage_error(help, "fq-rmdup takes one FASTQ, R1.fq and R2.fq, or one FASTQ with --interleaved");
  const bool two = files.size() == 2;
  if ((co.flags & SCFQ_RMDUP_SWAPPED) && !two && !interleaved) usage_error(help, "--swapped compares the mates of pairs: it goes with R1.fq R2.fq or --interleaved");
  if (two && !out.empty()) usage_error(help, "R1.fq R2.fq write to --out1=PATH and --out2=PATH");
  if (two && out1.empty() != out2.empty()) usage_error(help, "--out1=PATH and --out2=PATH go together");
  if (!two && (!out1.empty() || !out2.empty())) usage_error(help, "--out1=PATH and --out2=PATH go with R1.fq R2.fq; one input is written to stdout or to --out=PATH");
  if (report_only && (!out.empty() || !out1.empty())) usage_error(help, "--report writes no reads: it goes without --out, --out1 and --out2");
  for (const std::string& f : files) require_suffix_room(f);
  // the inputs are looked at before an output file is made
  for (const std::string& f : files)
    if (access(f.c_str(), R_OK) != 0) quit_unable_to_open(f);
  const bool to_stdout = !two && out.empty() && !report_only;      // stdout carries the reads: the report goes to stderr
  const std::string p1 = two ? out1 : out;
  int fd1 = to_stdout ? 1 : -1, fd2 = -1, fdr = -1;
  // a call that fails leaves no output file behind: what this process created goes again (fq-trim's rule)
  auto discard = [&]() {
    auto drop = [](int fd, const std::string& p) {
      struct stat st;
      const bool regular = fstat(fd, &st) == 0 && S_ISREG(st.st_mode);
      close(fd);
      if (regular) unlink(p.c_str());
    };
    if (!to_stdout && fd1 >= 0) drop(fd1, p1);
    if (fd2 >= 0) drop(fd2, out2);
    if (fdr >= 0) drop(fdr, per_read);
    fd1 = fd2 = fdr = -1;
  };
  auto create = [&](const std::string& p) -> int {
    const int fd = open(p.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (fd < 0) { discard(); quit_error("Unable to create file: " + p, 1); }
    return fd;
  };
  if (!p1.empty()) fd1 = create(p1);
  if (two && !out2.empty()) fd2 = create(out2);
  if (!per_read.empty()) fdr = create(per_read);
  scfq_rmdup_stats st = fresh<scfq_rmdup_stats>();
  std::vector<uint64_t> bins(SCFQ_RMDUP_HIST_BINS);
  std::fflush(stdout);
  const int rc = scfq_rmdup_files(files[0].c_str(), two ? files[1].c_str() : nullptr, &co, nullptr, fd1, fd2, fdr, bins.data(), &st);
  if (rc != SCFQ_OK && rc != SCFQ_EPIPE) discard();
  else { if (!to_stdout && fd1 >= 0) close(fd1); if (fd2 >= 0) close(fd2); if (fdr >= 0) close(fdr); }
  if (rc == SCFQ_EOPEN) quit_unable_to_open(first_unopenable(files[0], two ? &files[1] : nullptr));
  if (rc == SCFQ_EPIPE) return 0;              // a reader of stdout that went away: quiet, as `sc fq-dedup | head`
  if (rc != SCFQ_OK) quit_error(library_error(rc, scfq_rmdup_error_detail()), 1);
  FILE* report = to_stdout ? stderr : stdout;
  if (to_stdout && !stats && !hist) return 0;
  char row[1024];
  if (cols.header) {
    scfq_format_rmdup_stats_tsv(nullptr, 1, row, sizeof row);
    std::fprintf(report, "%s\n", output_header(hist ? kRmdupHistHeader : row, cols.basename, cols.absolute).c_str());
  }
  if (hist) {
    // the units of the last bin are what the other bins leave of units_in
    uint64_t below = 0;
    for (uint64_t c = 1; c + 1 < SCFQ_RMDUP_HIST_BINS; ++c) below += c * bins[c];
    for (uint64_t c = 1; c < SCFQ_RMDUP_HIST_BINS; ++c) {
      if (!bins[c]) continue;
      if (c + 1 < SCFQ_RMDUP_HIST_BINS) std::snprintf(row, sizeof row, "%llu\t%llu\t%llu", (unsigned long long)c, (unsigned long long)bins[c], (unsigned long long)(c * bins[c]));
      else std::snprintf(row, sizeof row, "1024+\t%llu\t%llu", (unsigned long long)bins[c], (unsigned long long)(st.units_in - below));
      std::fprintf(report, "%s\n", cols.row(row, files[0]).c_str());
    }
  } else {
    scfq_format_rmdup_stats_tsv(&st, 0, row, sizeof row);
    std::fprintf(report, "%s\n", cols.row(row, files[0]).c_str());
  }
  return 0;
}

// command "fq-repair" (addition, not in the reference): R1.fq R2.fq with --out1=PATH --out2=PATH (or neither: the report only),
// --singles1=PATH, --singles2=PATH, --check, --per-read=PATH, -t/--header, -b/--basename, -a/--absolute.  The report goes to stdout.
static int cmd_fq_repair(const std::vector<std::string>& params) {
  static const char* const help =
      "Re-pair R1 and R2 by read name: the mates that find each other leave in step, the others as singles\n\n"
      "Usage:\n  fq-repair [options] --out1=PATH --out2=PATH [--singles1=PATH] [--singles2=PATH] R1.fq R2.fq\n"
      "  fq-repair [options] --check R1.fq R2.fq\n\n"
      "Arguments:\n  R1.fq R2.fq      Two FASTQs. A record's name is its header without the first byte, up to the first blank or tab,\n"
      "                   without one trailing /1 or /2; without --out1 and --out2 only the report is produced\n\nOptions:\n"
      "      --out1=PATH            The R1 records that have a mate, in R1's order\n"
      "      --out2=PATH            Their mates from R2, in that same order\n"
      "      --singles1=PATH        The R1 records without a mate\n"
      "      --singles2=PATH        The R2 records without a mate\n"
      "      --check                No reads are written: the one-row report, and exit status 0 when the inputs are in step, else 1\n"
      "      --per-read=PATH        One row per record to PATH: input record mate (\"-\" for a single)\n"
      "  -t, --header               Output the header\n  -b, --basename             Add a column with the basename of the first FASTQ\n"
      "  -a, --absolute             Add a column with the absolute path of the first FASTQ\n"
      "  -h, --help                 Show this help\n";
  Columns cols;
  scfq_repair_opts co = fresh<scfq_repair_opts>();
  bool check = false;
  std::vector<std::string> files;
  std::string path[4], per_read;          // out1, out2, singles1, singles2
  const std::vector<Opt> table = cols.options({
      opt_text("out1", &path[0]),
      opt_text("out2", &path[1]),
      opt_text("singles1", &path[2]),
      opt_text("singles2", &path[3]),
      opt_flag("check", 0, &check),
      opt_text("per-read", &per_read),
  });
  if (!parse_options(params, help, table, &files)) return 0;
  if (files.empty()) quit_no_fastq();
  if (files.size() != 2) usage_error(help, "fq-repair takes R1.fq and R2.fq");
  if (path[0].empty() != path[1].empty()) usage_error(help, "--out1=PATH and --out2=PATH go together");
  if (check && !(path[0].empty() && path[2].empty() && path[3].empty())) usage_error(help, "--check writes no reads: it goes without --out1, --out2, --singles1 and --singles2");
  for (const std::string& f : files) require_suffix_room(f);
  // the inputs are looked at before an output file is made
  for (const std::string& f : files)
    if (access(f.c_str(), R_OK) != 0) quit_unable_to_open(f);
  int fd[4] = {-1, -1, -1, -1}, fdr = -1;
  // a call that fails leaves no output file behind: what this process created goes again (fq-trim's rule)
  auto discard = [&]() {
    auto drop = [](int& d, const std::string& p) {
      if (d < 0) return;
      struct stat st;
      const bool regular = fstat(d, &st) == 0 && S_ISREG(st.st_mode);
      close(d);
      if (regular) unlink(p.c_str());
      d = -1;
    };
    for (int k = 0; k < 4; ++k) drop(fd[k], path[k]);
    drop(fdr, per_read);
  };
  auto create = [&](const std::string& p) -> int {
    const int d = open(p.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (d < 0) { discard(); quit_error("Unable to create file: " + p, 1); }
    return d;
  };
  for (int k = 0; k < 4; ++k)
    if (!path[k].empty()) fd[k] = create(path[k]);
  if (!per_read.empty()) fdr = create(per_read);
  scfq_repair_stats st = fresh<scfq_repair_stats>();
  std::fflush(stdout);
  const int rc = scfq_repair_files(files[0].c_str(), files[1].c_str(), &co, nullptr, fd[0], fd[1], fd[2], fd[3], fdr, &st);
  if (rc != SCFQ_OK && rc != SCFQ_EPIPE) discard();
  else { for (int d : fd) if (d >= 0) close(d); if (fdr >= 0) close(fdr); }
  if (rc == SCFQ_EOPEN) quit_unable_to_open(first_unopenable(files[0], &files[1]));
  if (rc == SCFQ_EPIPE) return 0;              // a reader that went away: quiet, as `sc fq-dedup | head`
  if (rc != SCFQ_OK) quit_error(library_error(rc, scfq_repair_error_detail()), 1);
  char row[1024];
  if (cols.header) {
    scfq_format_repair_stats_tsv(nullptr, 1, row, sizeof row);
    std::printf("%s\n", output_header(row, cols.basename, cols.absolute).c_str());
  }
  scfq_format_repair_stats_tsv(&st, 0, row, sizeof row);
  std::printf("%s\n", cols.row(row, files[0]).c_str());
  std::fflush(stdout);
  return check && !st.in_step ? 1 : 0;
}

// command "fq-kcount" (addition, not in the reference): -t/--header, -b/--basename, -a/--absolute as fq-count, --k=N, --canonical,
// --table-bits=N, --high=N, --totals, --dump [--min-count=C] [--max-count=C], --top=N, IN.fq [IN2.fq]
static const char* kKcountHistHeader = "count\tkmers";
static const char* kKcountTotalsHeader = "k\twindows\tkmers\tskipped\tshort_lines\tdistinct\tunique\tmax_count";
static int cmd_fq_kcount(const std::vector<std::string>& params) {
  static const char* const help =
      "K-mer counts of the sequence lines of one or two FASTQ, k = 13 .. 32, in a hash table on the device\n\n"
      "Usage:\n  fq-kcount [options] IN.fq [IN2.fq]\n\nArguments:\n"
      "  IN.fq [IN2.fq]   Input FASTQ; two files are counted together into one table\n\nOptions:\n"
      "  -t, --header               Output the header\n"
      "  -b, --basename             Add basename column (of IN.fq)\n  -a, --absolute             Add column for absolute path (of IN.fq)\n"
      "      --k=N                  Length of the k-mers, 13 .. 32 (default: 21); only windows of A C G T count\n"
      "      --canonical            Count a k-mer and its reverse complement as the smaller of the two\n"
      "      --table-bits=N         A table of 2^N slots, 10 .. 32, that does not grow (default: sized by the input, and\n"
      "                             grown fourfold when it turns out too small)\n"
      "      --high=N               The default output, the histogram of the counts: a row \"count kmers\" for every count\n"
      "                             from 1 to min(largest count, N), zeros included, and a row N + 1 that holds everything\n"
      "                             above when there is any (default: 10000, at most 1048574)\n"
      "      --totals               One row instead: k windows kmers skipped short_lines distinct unique max_count\n"
      "      --dump                 The k-mers and their counts instead, in k-mer order\n"
      "      --min-count=C          With --dump: only k-mers that occur at least C times (default: 1)\n"
      "      --max-count=C          With --dump: only k-mers that occur at most C times\n"
      "      --top=N                The N most frequent k-mers instead, ties in k-mer order\n"
      "  -h, --help                 Show this help\n";
  const uint64_t kNone = ~0ull, kTopCandidates = 1ull << 24;
  Columns cols;
  bool totals = false, dump = false;
  uint32_t k = 21, flags = 0, table_bits = 0;
  uint64_t high = 10000, top = kNone, min_count = kNone, max_count = kNone;
  std::vector<std::string> files;
  const std::vector<Opt> options = cols.options({
      opt_number("k", 18, SCFQ_KCOUNT_MIN_K, SCFQ_KCOUNT_MAX_K, &k),
      opt_bits("canonical", &flags, SCFQ_KCOUNT_CANONICAL),
      opt_number("table-bits", 18, 10, 32, &table_bits),
      opt_number("high", 18, 1, (1ull << 20) - 2, &high),
      opt_flag("totals", 0, &totals),
      opt_flag("dump", 0, &dump),
      opt_number("min-count", 18, 1, ~0ull, &min_count),
      opt_number("max-count", 18, 1, ~0ull, &max_count),
      opt_number("top", 18, 0, kNone - 1, &top),      // (18 digits cannot say kNone)
  });
  if (!parse_options(params, help, options, &files)) return 0;
  if ((int)totals + (int)dump + (int)(top != kNone) > 1) usage_error(help, "--totals, --dump and --top exclude each other");
  if (!dump && (min_count != kNone || max_count != kNone)) usage_error(help, "--min-count and --max-count go with --dump");
  if (min_count != kNone && max_count != kNone && max_count < min_count) usage_error(help, "--max-count is below --min-count");
  if (files.size() > 2) usage_error(help, "at most two FASTQ are counted together");
  cols.header_or_no_input(totals ? kKcountTotalsHeader : (dump || top != kNone) ? kKmersHeader : kKcountHistHeader, files.empty());
  if (files.empty()) return 0;
  for (const auto& f : files) require_suffix_room(f);
  const std::string* second = files.size() > 1 ? &files[1] : nullptr;
  scfq_kcount_opts ko = fresh<scfq_kcount_opts>();
  ko.k = k;
  ko.flags = flags;
  ko.table_bits = table_bits;
  scfq_kcount_summary s = fresh<scfq_kcount_summary>();
  scfq_kcount* table = nullptr;
  int rc = scfq_kcount_files(files[0].c_str(), second ? second->c_str() : nullptr, nullptr, &ko, totals ? nullptr : &table, &s);
  if (rc == SCFQ_EOPEN) quit_unable_to_open(first_unopenable(files[0], second));
  if (rc != SCFQ_OK) quit_error(library_error(rc, scfq_kcount_error_detail()), 1);
  auto must = [&](int code) { if (code != SCFQ_OK) quit_error(library_error(code, scfq_kcount_error_detail()), 1); };
  char row[96];
  if (totals) {
    cols.emit_row(std::to_string(s.k) + "\t" + std::to_string(s.windows) + "\t" + std::to_string(s.kmers) + "\t" + std::to_string(s.skipped) + "\t" +
                      std::to_string(s.short_lines) + "\t" + std::to_string(s.distinct) + "\t" + std::to_string(s.unique) + "\t" +
                      std::to_string(s.max_count),
                  files[0]);
  } else if (dump) {
    std::vector<scfq_kmer_count> rows;
    uint64_t total = 0;
    const uint64_t lo = min_count == kNone ? 1 : min_count, hi = max_count == kNone ? 0 : max_count;
    must(scfq_kcount_dump(table, lo, hi, nullptr, 0, &total));
    rows.resize((size_t)total);
    if (total) must(scfq_kcount_dump(table, lo, hi, rows.data(), total, &total));
    for (const auto& r : rows) {
      scfq_format_kcount_tsv(k, r.key, r.count, row, sizeof row);
      cols.emit_row(row, files[0]);
    }
  } else if (top != kNone) {
    // the count of the last place is read off the histogram; the k-mers with that count or more are the candidates
    const uint64_t bins = std::min<uint64_t>(s.max_count + 2, 1ull << 20);
    std::vector<uint64_t> hist((size_t)bins);
    must(scfq_kcount_hist(table, hist.data(), bins));
    uint64_t threshold = bins - 1, above = 0;
    for (; threshold > 1 && above + hist[threshold] < top; --threshold) above += hist[threshold];
    std::vector<scfq_kmer_count> rows;
    uint64_t total = 0;
    if (top) must(scfq_kcount_dump(table, threshold, 0, nullptr, 0, &total));
    if (total > kTopCandidates)
      usage_error(help, "--top=" + std::to_string(top) + ": " + std::to_string(total) + " k-mers occur " + std::to_string(threshold) +
                            " times or more, which are more than " + std::to_string(kTopCandidates) + " candidates; use --dump --min-count=C");
    rows.resize((size_t)total);
    if (total) must(scfq_kcount_dump(table, threshold, 0, rows.data(), total, &total));
    const size_t keep = (size_t)std::min<uint64_t>(top, rows.size());
    std::partial_sort(rows.begin(), rows.begin() + keep, rows.end(), [](const scfq_kmer_count& a, const scfq_kmer_count& b) {
      return a.count != b.count ? a.count > b.count : a.key < b.key;
    });
    rows.resize(keep);
    for (const auto& r : rows) {
      scfq_format_kcount_tsv(k, r.key, r.count, row, sizeof row);
      cols.emit_row(row, files[0]);
    }
  } else {
    const uint64_t bins = high + 2;
    std::vector<uint64_t> hist((size_t)bins);
    must(scfq_kcount_hist(table, hist.data(), bins));
    for (uint64_t c = 1; c <= std::min<uint64_t>(s.max_count, high); ++c) cols.emit_row(std::to_string(c) + "\t" + std::to_string(hist[c]), files[0]);
    if (hist[high + 1]) cols.emit_row(std::to_string(high + 1) + "\t" + std::to_string(hist[high + 1]), files[0]);
  }
  scfq_kcount_free(table);
  std::fflush(stdout);
  return 0;
}

// command "fq-adapters" (addition, not in the reference): -t/--header, -b/--basename, -a/--absolute as fq-count, --adapter=NAME:SEQ,
// --max-positions=N, --counts, --totals, [fastq ...]
static const char* kAdaptersTotalsHeader = "adapter\tsequence\treads\treads_with\tpercent\thits";
static int cmd_fq_adapters(const std::vector<std::string>& params) {
  static const char* const help =
      "Adapter content by read position of a FASTQ\n\nUsage:\n  fq-adapters [options] [fastq ...]\n\nArguments:\n"
      "  [fastq ...]      Input FASTQ\n\nOptions:\n  -t, --header               Output the header\n"
      "  -b, --basename             Add basename column\n  -a, --absolute             Add column for absolute path\n"
      "      --adapter=NAME:SEQ     Look for SEQ (1 .. 32 letters of A C G T) and call it NAME; up to eight, and giving any\n"
      "                             replaces the built-in set (Illumina universal and small RNA, Nextera, SOLiD, poly-A, poly-G)\n"
      "      --max-positions=N      One row per position up to N (default: 1000, at most 16777216); what lies beyond\n"
      "                             comes as one last row \">N\"\n"
      "      --counts               The reads whose first occurrence starts at the position, as integers (default: the\n"
      "                             percentage of the reads in which it starts at or before the position); the \">N\" row\n"
      "                             then holds the reads whose first occurrence starts beyond N\n"
      "      --totals               One row per adapter and file instead: adapter sequence reads reads_with percent hits,\n"
      "                             and a row \"any\"\n"
      "  -h, --help                 Show this help\n";
  Columns cols;
  bool counts = false, totals = false;
  uint64_t max_positions = 1000;
  std::vector<std::string> files, names, seqs;
  const std::vector<Opt> table = cols.options({
      opt_flag("counts", 0, &counts),
      opt_flag("totals", 0, &totals),
      opt_number("max-positions", 8, 0, SCFQ_ADAPTERS_MAX_CAP, &max_positions),
      opt_custom("adapter", [&](std::string& v) {
        const size_t colon = v.find(':');
        const std::string name = colon == std::string::npos ? "" : v.substr(0, colon), seq = colon == std::string::npos ? "" : v.substr(colon + 1);
        if (name.empty() || name.find('\t') != std::string::npos || seq.empty() || seq.size() > SCFQ_ADAPTERS_MAX_LEN ||
            seq.find_first_not_of("ACGT") != std::string::npos || names.size() >= SCFQ_ADAPTERS_MAX_PROBES)
          return Reject::bad_value;
        names.push_back(name);
        seqs.push_back(seq);
        return Reject::none;
      }),
  });
  if (!parse_options(params, help, table, &files)) return 0;
  if (names.empty()) {
    const char *name = nullptr, *seq = nullptr;
    for (uint32_t i = 0; scfq_adapters_default(i, &name, &seq) > 0; ++i) { names.push_back(name); seqs.push_back(seq); }
  }
  const uint32_t np = (uint32_t)names.size();
  std::vector<const char*> probes;
  for (const auto& s : seqs) probes.push_back(s.c_str());
  std::string positions_header = "position";
  for (const auto& nm : names) positions_header += "\t" + nm;
  cols.header_or_no_input(totals ? std::string(kAdaptersTotalsHeader) : positions_header + "\tany", files.empty());
  std::vector<scfq_adapter_row> rows;
  for (const auto& fastq : files) {
    require_suffix_room(fastq);
    scfq_adapter_summary s;
    // the table is as long as the file's longest sequence line, not as --max-positions; --totals needs no table
    const int rc = size_then_fill(
        &rows, &s,
        [&](scfq_adapter_row* r, uint64_t n, scfq_adapter_summary* out) { return scfq_adapters_file(fastq.c_str(), nullptr, probes.data(), np, r, n, out); },
        [&](const scfq_adapter_summary& sized) { return totals ? 0 : std::min<uint64_t>(max_positions, sized.max_seq_len); });
    if (rc == SCFQ_EOPEN) quit_unable_to_open(fastq);
    if (rc != SCFQ_OK) quit_error(library_error(rc, scfq_adapters_error_detail()), 1);
    char row[1024];
    if (totals) {
      uint64_t hits = 0;
      for (uint32_t j = 0; j <= np; ++j) {
        const uint64_t with = j < np ? s.total.first[j] : s.total.any;
        const std::string line = (j < np ? names[j] + "\t" + seqs[j] : std::string("any\t*")) + "\t" + std::to_string(s.reads) + "\t" +
                                 std::to_string(with) + "\t" + nim_float(100.0 * (double)with / (double)s.reads) + "\t" +
                                 std::to_string(j < np ? s.hits[j] : hits);
        if (j < np) hits += s.hits[j];
        cols.emit_row(line, fastq);
      }
      continue;
    }
    // the rows as they are with --counts; added up from position 1 otherwise
    scfq_adapter_row acc = scfq_adapter_row();
    for (uint64_t p = 0; p < s.positions; ++p) {
      for (uint32_t j = 0; j < np; ++j) acc.first[j] += rows[p].first[j];
      acc.any += rows[p].any;
      scfq_format_adapter_row_tsv(counts ? &rows[p] : &acc, np, s.reads, counts, row, sizeof row);
      cols.emit_row(std::to_string(p + 1) + "\t" + row, fastq);
    }
    bool tail = s.tail.any != 0;
    for (uint32_t j = 0; j < np; ++j) tail = tail || s.tail.first[j] != 0;
    if (tail) {
      scfq_format_adapter_row_tsv(counts ? &s.tail : &s.total, np, s.reads, counts, row, sizeof row);
      cols.emit_row(">" + std::to_string(max_positions) + "\t" + row, fastq);
    }
  }
  std::fflush(stdout);
  return 0;
}

// command "fa-gc" (sc.nim:84-96, src/fa_gc.nim): --pos <chr:pos | file> <fasta> <window> [<window> ...]
static void warning_msg(const std::string& msg) {                    // helpers.nim:36-37 (colorize fgYellow)
  std::fprintf(stderr, "\x1b[33mWarning: %s\x1b[0m\n", msg.c_str());
}

struct FaPosition {
  std::string chrom;
  long long pos = 0;
};

static bool fa_parse_int(const std::string& s, long long* out) {     // Nim parseInt without the '_' separators
  const size_t d = (!s.empty() && (s[0] == '-' || s[0] == '+')) ? 1 : 0;
  if (s.size() == d || s.size() - d > 18 || s.find_first_not_of("0123456789", d) != std::string::npos) return false;
  *out = std::atoll(s.c_str());
  return true;
}

// The whole positions file; a name that ends in ".gz" goes through the library's host gzip reader.
static bool fa_read_text(const std::string& path, std::string* out) {
  if (path.size() >= 3 && path.compare(path.size() - 3, 3, ".gz") == 0) {
    for (uint64_t cap = 1u << 20;; cap *= 4) {
      out->resize(cap);
      const int64_t got = scfq_debug_read_file(path.c_str(), &(*out)[0], cap, 0);
      if (got >= 0) { out->resize((size_t)got); return true; }
      if (got != SCFQ_EARG || cap > (1ull << 34)) return false;     // (SCFQ_EARG: the text does not fit into cap)
    }
  }
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) return false;
  out->clear();
  char buf[1 << 16];
  size_t got;
  while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) out->append(buf, got);
  std::fclose(f);
  return true;
}

// iter_pos, helpers.nim:88-151: one "chr:pos" string, or a text file with chrom and position as its first two fields
static std::vector<FaPosition> fa_positions(const std::string& pos_in) {
  std::vector<FaPosition> out;
  if (pos_in.find(':') != std::string::npos && pos_in.find('/') == std::string::npos) {
    const size_t c = pos_in.find(':');
    FaPosition p;
    p.chrom = pos_in.substr(0, c);
    if (!fa_parse_int(pos_in.substr(c + 1), &p.pos)) quit_error("Invalid position: " + pos_in, 1);
    out.push_back(p);
    return out;
  }
  std::string lower = pos_in;
  for (char& ch : lower) ch = (char)std::tolower((unsigned char)ch);
  if (lower.size() >= 4 && lower.compare(lower.size() - 4, 4, ".bcf") == 0)
    quit_error("BCF position files are not supported: " + pos_in + " (give chr:pos, or a text file: BED, VCF, TSV)", 1);
  std::string text;
  if (!fa_read_text(pos_in, &text)) quit_unable_to_open(pos_in, 2);
  const char* seps = "\t: ";
  size_t at = 0;
  for (long long n = 1; at < text.size(); ++n) {
    size_t nl = text.find('\n', at);
    if (nl == std::string::npos) nl = text.size();
    std::string line = text.substr(at, nl - at);
    at = nl + 1;
    if (!line.empty() && line.back() == '\r') line.pop_back();
    const size_t first = line.find_first_not_of(seps), last = line.find_last_not_of(seps);
    const std::string cur = first == std::string::npos ? "" : line.substr(first, last - first + 1);
    const size_t e1 = cur.find_first_of(seps);
    FaPosition p;
    bool ok = e1 != std::string::npos;
    if (ok) {
      const size_t s2 = cur.find_first_not_of(seps, e1);
      size_t e2 = cur.find_first_of(seps, s2);
      if (e2 == std::string::npos) e2 = cur.size();
      p.chrom = cur.substr(0, e1);
      ok = fa_parse_int(cur.substr(s2, e2 - s2), &p.pos);
    }
    if (ok) out.push_back(p);
    else if (n != 1 && (line.empty() || line[0] != '#'))
      warning_msg("Invalid line: " + std::to_string(n) + " in \"" + pos_in + "\" > " + line);
  }
  return out;
}

// The order of the rows: names lower-cased and without a leading "chr"; all-digit names first, by value and then position;
// then x, y, m, by that rank and then position; then every other name in byte order, input order kept within a name.  This
// is genome_cmp (helpers.nim:164-193) wherever genome_cmp is a consistent order: it is not for ties among x / y / m (its
// second branch repeats the first, so equal ranks compare as "greater" both ways) nor between one of x / y / m and another
// non-numeric name (x < "i" by name but every x, y, m pair ignores names), where the result of its sort depends on the
// input order.
struct FaSortKey {
  int group = 2;              // 0 digits, 1 x / y / m, 2 other
  std::string name;           // digits without leading zeros / the folded name
  int rank = 0;
  long long pos = 0;
};
static FaSortKey fa_sort_key(const FaPosition& p) {
  FaSortKey k;
  std::string s = p.chrom;
  for (char& ch : s) ch = (char)std::tolower((unsigned char)ch);
  if (s.size() > 3 && s.compare(0, 3, "chr") == 0) s = s.substr(3);
  k.name = s;
  k.pos = p.pos;
  if (s.find_first_not_of("0123456789") == std::string::npos) {   // (an empty name is all digits to the reference's all())
    k.group = 0;
    const size_t nz = s.find_first_not_of('0');
    k.name = nz == std::string::npos ? "" : s.substr(nz);
  } else if (s == "x" || s == "y" || s == "m") {
    k.group = 1;
    k.rank = s == "x" ? 1 : s == "y" ? 2 : 3;
  }
  return k;
}
static bool fa_key_less(const FaSortKey& a, const FaSortKey& b) {
  if (a.group != b.group) return a.group < b.group;
  if (a.group == 0) {
    if (a.name.size() != b.name.size()) return a.name.size() < b.name.size();
    if (a.name != b.name) return a.name < b.name;
    return a.pos < b.pos;
  }
  if (a.group == 1) return a.rank != b.rank ? a.rank < b.rank : a.pos < b.pos;
  return a.name < b.name;
}

static int cmd_fa_gc(const std::vector<std::string>& params) {
  static const char* const help =
      "Calculate GC content surrouding a location\n\nUsage:\n  fa-gc [options] fasta [windows ...]\n\nArguments:\n"
      "  fasta            Input FASTA (plain, .gz or BGZF)\n"
      "  [windows ...]    sequence length up and downstream (50 --> ~100bp window [see docs])\n\nOptions:\n"
      "  -p, --pos=POS              VCF, BED, or string position (e.g. chr1:8675309)\n"
      "  -h, --help                 Show this help\n";
  if (params.size() == 1) { std::fputs(help, stdout); return 0; }
  // the reference's grammar (-p X / -p=X / --pos X / --pos=X: a value in the next argument), so not a table for parse_options()
  std::string pos_in;
  std::vector<std::string> args;
  bool only_positional = false;
  for (size_t i = 1; i < params.size(); ++i) {
    const std::string& a = params[i];
    if (only_positional || a.empty() || a[0] != '-' || a == "-") { args.push_back(a); continue; }
    if (a == "--") { only_positional = true; continue; }
    if (a == "-h" || a == "--help") { std::fputs(help, stdout); return 0; }
    if (a == "-p" || a == "--pos") {
      if (i + 1 >= params.size()) usage_error(help, "Missing value for " + a);
      pos_in = params[++i];
    } else if (a.compare(0, 6, "--pos=") == 0) pos_in = a.substr(6);
    else if (a.compare(0, 3, "-p=") == 0) pos_in = a.substr(3);
    else unknown_option(help, a);
  }
  if (args.empty()) usage_error(help, "Missing FASTA");
  if (pos_in.empty()) quit_error("Must provide --pos: (chr:100 / bed / vcf )", 1);
  if (args.size() < 2) quit_error("Must provide a list of windows: (e.g. 100 200 500)", 1);
  const std::string fasta = args[0];
  std::vector<uint64_t> windows;
  for (size_t i = 1; i < args.size(); ++i) {
    uint64_t w = 0;
    if (scfq_fa_parse_window(args[i].c_str(), &w) != SCFQ_OK) quit_error(scfq_fa_error_detail(), 1);
    windows.push_back(w);
  }
  std::vector<FaPosition> positions = fa_positions(pos_in);
  {
    std::vector<std::pair<FaSortKey, FaPosition>> keyed;
    for (const auto& p : positions) keyed.emplace_back(fa_sort_key(p), p);
    std::stable_sort(keyed.begin(), keyed.end(), [](const auto& a, const auto& b) { return fa_key_less(a.first, b.first); });
    for (size_t i = 0; i < keyed.size(); ++i) positions[i] = keyed[i].second;
  }

  scfq_fa_index* index = nullptr;
  const int rc = scfq_fa_index_file(fasta.c_str(), nullptr, &index, nullptr);
  if (rc == SCFQ_EOPEN) quit_unable_to_open(fasta, 2);
  if (rc != SCFQ_OK) quit_error(library_error(rc, scfq_fa_error_detail()), 1);
  std::string header = "chrom\tpos";
  for (const uint64_t w : windows) header += "\tgc_" + std::to_string(2 * w);
  std::printf("%s\n", header.c_str());

  // every cell of the run in one call
  std::vector<const FaPosition*> rows;
  std::vector<scfq_fa_interval> cells;
  for (const auto& p : positions) {
    uint64_t c = 0;
    scfq_fa_contig contig;
    int out_of_range = 1;
    uint64_t begin = 0, end = 0;
    if (scfq_fa_contig_find(index, p.chrom.c_str(), &c) == SCFQ_OK && scfq_fa_contig_at(index, c, &contig) == SCFQ_OK)
      scfq_fa_gc_interval(p.pos, windows[0], contig.length, &begin, &end, &out_of_range);
    if (out_of_range) {     // (the reference dereferences nil here)
      warning_msg("<" + p.chrom + ":" + std::to_string(p.pos) + "> is out of range");
      continue;
    }
    rows.push_back(&p);
    for (const uint64_t w : windows) {
      scfq_fa_gc_interval(p.pos, w, contig.length, &begin, &end, &out_of_range);
      cells.push_back(scfq_fa_interval{c, begin, end});
    }
  }
  std::vector<scfq_fa_counts> counts(cells.size());
  const int qrc = scfq_fa_count_intervals(index, cells.data(), cells.size(), counts.data());
  if (qrc != SCFQ_OK) quit_error(library_error(qrc, scfq_fa_error_detail()), 1);
  for (size_t r = 0; r < rows.size(); ++r) {
    std::string line = rows[r]->chrom + "\t" + std::to_string(rows[r]->pos);
    for (size_t k = 0; k < windows.size(); ++k) {
      char cell[48];
      const scfq_fa_counts& v = counts[r * windows.size() + k];
      scfq_format_fa_gc_value(v.gc, v.acgt, windows[k], cell, sizeof cell);
      line += "\t";
      line += cell;
    }
    std::printf("%s\n", line.c_str());
  }
  std::fflush(stdout);
  scfq_fa_index_free(index);
  return 0;
}

// command "fq-count" (sc.nim:103-116) and the MI355X additions of its help
static int cmd_fq_count(const std::vector<std::string>& params) {
  Columns cols;
  bool debug = false;      // --debug is accepted and ignored
  int jobs = 0;            // 0: not given
  int shard_rank = -1, shard_world = 0, transport = SCFQ_COMM_RCCL;
  std::string rendezvous;
  std::vector<std::string> files;
  std::vector<int32_t> devices;
  scfq_opts opts = fresh<scfq_opts>();
  // these numbers are read leniently (atoi): what is no number counts as 0
  auto lenient = [](int* out, int at_least = INT_MIN) {
    return [out, at_least](std::string& v) { *out = std::max(at_least, std::atoi(v.c_str())); return Reject::none; };
  };
  const std::vector<Opt> table = cols.options({
      opt_flag("debug", 0, &debug),
      opt_bits("struct-check", &opts.flags, SCFQ_STRUCT_CHECK),
      opt_bits("qual-hist", &opts.flags, SCFQ_QUAL_HIST),
      opt_bits("stats", &opts.flags, SCFQ_TIMING),
      opt_custom("jobs", lenient(&jobs, 1)),
      opt_custom("shard-rank", lenient(&shard_rank)),
      opt_custom("shard-world", lenient(&shard_world)),
      opt_custom("rendezvous", [&](std::string& v) { rendezvous = v; return Reject::none; }),     // (may be empty)
      opt_custom("transport", [&](std::string& v) {
        if (v != "tcp" && v != "rccl") return Reject::unknown_option;
        transport = v == "tcp" ? SCFQ_COMM_TCP : SCFQ_COMM_RCCL;
        return Reject::none;
      }),
      opt_custom("devices", [&](std::string& list) {
        size_t p = 0;
        while (p < list.size()) {
          size_t q = list.find(',', p);
          if (q == std::string::npos) q = list.size();
          devices.push_back(std::atoi(list.substr(p, q - p).c_str()));
          p = q + 1;
        }
        return Reject::none;
      }),
  });
  if (!parse_options(params, kHelpFqCount, table, &files)) return 0;
  opts.n_devices = (int32_t)devices.size();
  opts.device_ids = devices.empty() ? nullptr : devices.data();
  if (const char* e = std::getenv("SC_GPU_CHUNK")) opts.chunk_bytes = std::strtoull(e, nullptr, 10);

  // ---- one process per GPU (addition): byte-range shard per rank, exchange inside the library, rank 0 prints ----------
  if (shard_world > 0 || shard_rank >= 0) {
    if (shard_world <= 0 && std::getenv("WORLD_SIZE")) shard_world = std::atoi(std::getenv("WORLD_SIZE"));
    if (shard_rank < 0 && std::getenv("RANK")) shard_rank = std::atoi(std::getenv("RANK"));
    if (rendezvous.empty() && std::getenv("MASTER_PORT"))
      rendezvous = std::string(std::getenv("MASTER_ADDR") ? std::getenv("MASTER_ADDR") : "127.0.0.1") + ":" + std::getenv("MASTER_PORT");
    const size_t colon = rendezvous.rfind(':');
    if (shard_world < 1 || shard_rank < 0 || shard_rank >= shard_world || colon == std::string::npos)
      quit_error("--shard-rank / --shard-world / --rendezvous=HOST:PORT do not describe a rank", 1);
    const std::string host = rendezvous.substr(0, colon);
    const int port = std::atoi(rendezvous.substr(colon + 1).c_str());
    if (devices.empty()) devices.push_back(shard_rank);
    opts.n_devices = 1;
    opts.device_ids = devices.data();
    scfq_comm* comm = nullptr;
    const int rc = scfq_comm_init_rendezvous(host.c_str(), port, shard_world, shard_rank, devices[0], transport, 0, &comm);
    if (rc) quit_error(std::string(scfq_strerror(rc)) + ": " + scfq_comm_error_detail(), 1);
    if (!cols.header || shard_rank == 0) cols.header_or_no_input(kHeader, files.empty());   // (the header comes from rank 0 alone)
    for (const auto& f : files) {
      const FileResult r = fq_count_compute(f, cols, opts, comm);
      if (r.exit_code || shard_rank == 0) fq_count_emit(r);       // every rank quits with the reference's message on an error
      else if (!r.extra.empty()) std::fputs(r.extra.c_str(), stderr);      // (the additions' stderr lines, e.g. --stats of this rank's share)
    }
    scfq_comm_destroy(comm);
    scfq_shutdown();
    return 0;
  }

  cols.header_or_no_input(kHeader, files.empty());                                       // sc.nim:110-113
  // several devices in one process: their RCCL communicators come up BEFORE the first row (while one is created the library
  // points descriptor 1 at descriptor 2 — RCCL prints a banner on stdout — and a row printed in that window would be lost to
  // stderr); a failure here is reported by the first counting call
  if (devices.size() > 1 && !files.empty()) (void)scfq_prepare(&opts);
  // sc.nim:114-116 takes the files one after the other.  Here two are in flight unless --jobs says otherwise (a file's
  // pipeline — read or copy, inflate, scan — leaves the device idle most of the time; file k + 1's ingest runs under file k's
  // kernels): rows still come out in argv order and the first failing file ends the run where the sequential loop would have.
  if (jobs == 0) jobs = devices.size() > 1 ? 1 : (int)std::min<size_t>(2, std::max<size_t>(1, files.size()));
  if (jobs <= 1 || files.size() <= 1) {
    for (const auto& f : files) fq_count_emit(fq_count_compute(f, cols, opts));   // sc.nim:114-116
  } else {
    // --jobs=N: up to N files in flight (each a session on its own device context: inflate / read of one file overlaps
    // the scans of the others); rows are still emitted strictly in argv order, and the first failing file ends the
    // run with the reference's message and exit code exactly where the sequential loop would have.
    std::vector<FileResult> results(files.size());
    std::vector<char> done(files.size(), 0);
    std::mutex mu;
    std::condition_variable cv;
    std::atomic<size_t> next{0};
    std::vector<std::thread> pool;
    const size_t nthreads = std::min<size_t>((size_t)jobs, files.size());
    for (size_t t = 0; t < nthreads; ++t)
      pool.emplace_back([&] {
        for (;;) {
          const size_t i = next.fetch_add(1);
          if (i >= files.size()) return;
          FileResult r = fq_count_compute(files[i], cols, opts);
          { std::lock_guard<std::mutex> lk(mu); results[i] = std::move(r); done[i] = 1; }
          cv.notify_all();
        }
      });
    for (size_t i = 0; i < files.size(); ++i) {
      { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return done[i] != 0; }); }
      if (results[i].exit_code) {   // stop handing out files, let the in-flight ones finish, then quit like the sequential loop
        next.store(files.size());
        for (auto& th : pool) th.join();
        scfq_shutdown();
      }
      fq_count_emit(results[i]);
    }
    for (auto& th : pool) if (th.joinable()) th.join();
  }
  // A process that is about to end does not give its device memory back piece by piece (scfq_shutdown: 40 - 50 ms of frees and
  // stream destruction after a 10 GB .gz): the rows are out, the driver reclaims everything with the process.  SC_CLEAN_EXIT=1 keeps
  // the orderly shutdown (leak checkers).
  std::fflush(stdout);
  std::fflush(stderr);
  if (std::getenv("SC_CLEAN_EXIT")) { scfq_shutdown(); return 0; }
  _exit(0);
}

int main(int argc, char** argv) {
  scfq_debug_stage_mark("sc: main entered");
  signal(SIGPIPE, SIG_IGN);   // sc.nim:45-46
  std::vector<std::string> params(argv + 1, argv + argc);
  if (stdin_is_fifo())        // sc.nim:274-284
    for (auto& p : params)
      if (p == "-") { p = "STDIN"; break; }
  if (params.empty() || params[0] == "-h" || params[0] == "--help") { help_top(stdout); return 0; }
  if (params[0] == "-v" || params[0] == "--version") { std::printf("%s\n", kVersion); return 0; }
  static const struct { const char* name; int (*run)(const std::vector<std::string>&); } commands[] = {
      {"fq-count", cmd_fq_count},       {"fq-dedup", cmd_fq_dedup},       {"fq-meta", cmd_fq_meta},
      {"fq-readstats", cmd_fq_readstats}, {"fq-cycles", cmd_fq_cycles},   {"fq-kmers", cmd_fq_kmers},
      {"fq-adapters", cmd_fq_adapters}, {"fq-insert-size", cmd_fq_insert_size}, {"fq-merge", cmd_fq_merge},
      {"fq-trim", cmd_fq_trim},         {"fq-screen", cmd_fq_screen},     {"fq-demux", cmd_fq_demux},
      {"fq-kcount", cmd_fq_kcount},     {"fq-normalize", cmd_fq_normalize}, {"fq-complexity", cmd_fq_complexity},
      {"fq-rmdup", cmd_fq_rmdup},       {"fq-repair", cmd_fq_repair},
      {"fa-gc", cmd_fa_gc}};
  for (const auto& c : commands)
    if (params[0] == c.name) return c.run(params);
  help_top(stdout);
  quit_error("Unknown command: " + params[0] + " (this build provides the FASTQ commands only)", 1);
}

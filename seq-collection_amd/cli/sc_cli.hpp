// sc_cli.hpp — what the commands of sc_main.cpp share: the reference's error and filename-column helpers, one option parser
// driven by a per-command table, and the per-file scaffold around a library call.
//
// Reference anchors:
//   src/utils/helpers.nim:29-34    "Error <code>: <msg>" in red on stderr, exit <code>
//   src/utils/helpers.nim:200-224  header / basename / absolute columns
//   sc.nim:294-298                 a usage error prints the help, then the error, exit 1
#pragma once
#include "../../include/sc_fqcount.h"

#include <limits.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

static void error_msg(const std::string& msg, int code) {           // helpers.nim:29-30 (colorize fgRed)
  std::fprintf(stderr, "\x1b[31mError %d: %s\x1b[0m\n", code, msg.c_str());
}
[[noreturn]] static void quit_error(const std::string& msg, int code = 1) {   // helpers.nim:32-34
  error_msg(msg, code);
  std::exit(code);
}
// the UsageError funnel, sc.nim:294-298: the command's help on stdout, then the error
[[noreturn]] static void usage_error(const char* help, const std::string& msg) {
  std::fputs(help, stdout);
  quit_error("Error: " + msg, 1);
}
[[noreturn]] static void unknown_option(const char* help, const std::string& what) { usage_error(help, "Unknown option: " + what); }

static std::string join_nonempty(const std::vector<std::string>& parts) {     // filterIt(it.len > 0).join("\t")
  std::string out;
  for (const auto& p : parts) {
    if (p.empty()) continue;
    if (!out.empty()) out += '\t';
    out += p;
  }
  return out;
}

static std::string output_header(const std::string& header, bool basename, bool absolute) {   // helpers.nim:200-208
  return join_nonempty({header, basename ? "basename" : "", absolute ? "absolute" : ""});
}

static std::string last_path_part(std::string p) {   // Nim os.lastPathPart
  while (p.size() > 1 && p.back() == '/') p.pop_back();
  if (p == "/") return "";
  const size_t k = p.find_last_of('/');
  return k == std::string::npos ? p : p.substr(k + 1);
}

static std::string normalize_join(const std::string& root, const std::string& rel) {   // Nim os.absolutePath/joinPath
  std::vector<std::string> comp;
  auto feed = [&](const std::string& s) {
    size_t i = 0;
    while (i <= s.size()) {
      size_t j = s.find('/', i);
      if (j == std::string::npos) j = s.size();
      std::string c = s.substr(i, j - i);
      if (c == "..") { if (!comp.empty()) comp.pop_back(); }
      else if (!c.empty() && c != ".") comp.push_back(c);
      i = j + 1;
    }
  };
  feed(root);
  feed(rel);
  std::string out;
  for (const auto& c : comp) { out += '/'; out += c; }
  return out.empty() ? "/" : out;
}

static std::string absolute_path(const std::string& p) {
  if (!p.empty() && p[0] == '/') return p;          // absolute inputs are returned verbatim
  char cwd[PATH_MAX];
  if (!getcwd(cwd, sizeof cwd)) return p;
  return normalize_join(cwd, p);
}

static std::string get_absolute(const std::string& path) {   // helpers.nim:210-213
  struct stat sb;
  if (lstat(path.c_str(), &sb) == 0 && S_ISLNK(sb.st_mode)) {
    char buf[PATH_MAX];
    ssize_t n = readlink(path.c_str(), buf, sizeof buf - 1);
    if (n >= 0) { buf[n] = 0; return absolute_path(buf); }   // relative targets resolve against the CWD (reference quirk)
  }
  return absolute_path(path);
}

static std::string output_w_fnames(const std::string& line, const std::string& path, bool basename, bool absolute) {
  return join_nonempty({line, basename ? last_path_part(path) : "", absolute ? get_absolute(path) : ""});   // helpers.nim:215-224
}

// ---- the option table ------------------------------------------------------------------------------------------------------
// A command declares its options as rows and its help as one text; parse_options() walks the arguments.

enum class Reject { none, bad_value, unknown_option };   // what a custom row says about the text after '='

struct Opt {
  enum Kind { FLAG, BITS, NUMBER, TEXT, CUSTOM } kind;   // FLAG and BITS stand alone, the other three take "=value"
  const char* name;                    // the long name, without the dashes
  char letter = 0;                     // the short letter of a FLAG or BITS row, 0: none
  bool* flag = nullptr;                // FLAG: set
  uint32_t* word = nullptr;            // BITS: *word |= bits
  uint32_t bits = 0;
  unsigned digits = 0;                 // NUMBER: all digits and at most this many of them, then lo .. hi
  uint64_t lo = 0, hi = 0;
  uint32_t* u32 = nullptr;             //   (one of the two receives it)
  uint64_t* u64 = nullptr;
  std::string* text = nullptr;         // TEXT: not empty
  std::function<Reject(std::string&)> custom;   // CUSTOM: may replace the text by what the "Bad value" message is to show
  Opt(Kind k, const char* n) : kind(k), name(n) {}
};

static Opt opt_flag(const char* name, char letter, bool* flag) { Opt o(Opt::FLAG, name); o.letter = letter; o.flag = flag; return o; }
static Opt opt_bits(const char* name, uint32_t* word, uint32_t bits) { Opt o(Opt::BITS, name); o.word = word; o.bits = bits; return o; }
static Opt opt_number(const char* name, unsigned digits, uint64_t lo, uint64_t hi, uint32_t* u32, uint64_t* u64 = nullptr) {
  Opt o(Opt::NUMBER, name); o.digits = digits; o.lo = lo; o.hi = hi; o.u32 = u32; o.u64 = u64; return o;
}
static Opt opt_number(const char* name, unsigned digits, uint64_t lo, uint64_t hi, uint64_t* u64) { return opt_number(name, digits, lo, hi, nullptr, u64); }
static Opt opt_text(const char* name, std::string* text) { Opt o(Opt::TEXT, name); o.text = text; return o; }
static Opt opt_custom(const char* name, std::function<Reject(std::string&)> fn) { Opt o(Opt::CUSTOM, name); o.custom = std::move(fn); return o; }

// a NUMBER row's rule, also for the custom rows that add a condition of their own
static bool bounded_number(const std::string& v, unsigned digits, uint64_t lo, uint64_t hi, uint64_t* out) {
  if (v.empty() || v.size() > digits || v.find_first_not_of("0123456789") != std::string::npos) return false;
  *out = std::stoull(v);
  return *out >= lo && *out <= hi;
}

// Walks params[1..] and collects the positionals; false when the help was asked for (it is printed, the command returns 0).
//   "--" ends the options; "-", "" and whatever does not start with '-' is a positional
//   -h, --help, a bare command: the help on stdout
//   -tba: the rows with these letters; a table without letters has no short options at all
//   --name / --name=value: the row of that name and form; anything else is an unknown option
static bool parse_options(const std::vector<std::string>& params, const char* help, const std::vector<Opt>& table,
                          std::vector<std::string>* positionals) {
  auto show_help = [&] { std::fputs(help, stdout); return false; };
  auto set = [](const Opt& o) { if (o.kind == Opt::FLAG) *o.flag = true; else *o.word |= o.bits; };
  if (params.size() == 1) return show_help();          // sc.nim:288-290: len <= 1 -> "-h"
  bool has_letters = false, only_positional = false;
  for (const Opt& o : table) has_letters = has_letters || o.letter;
  for (size_t i = 1; i < params.size(); ++i) {
    const std::string& a = params[i];
    if (only_positional || a.empty() || a[0] != '-' || a == "-") { positionals->push_back(a); continue; }
    if (a == "--") { only_positional = true; continue; }
    if (a == "-h" || a == "--help") return show_help();
    if (a[1] != '-' && has_letters) {                  // combined short flags: -tb
      for (size_t k = 1; k < a.size(); ++k) {
        if (a[k] == 'h') return show_help();
        const Opt* row = nullptr;
        for (const Opt& o : table) if (o.letter == a[k]) row = &o;
        if (!row) unknown_option(help, std::string("-") + a[k]);
        set(*row);
      }
      continue;
    }
    const size_t eq = a.find('=');
    const bool has_value = eq != std::string::npos;
    const std::string name = a[1] == '-' ? a.substr(2, has_value ? eq - 2 : std::string::npos) : "";
    const Opt* row = nullptr;
    for (const Opt& o : table) if (name == o.name && (o.kind >= Opt::NUMBER) == has_value) row = &o;
    if (!row) unknown_option(help, a);
    if (!has_value) { set(*row); continue; }
    std::string v = a.substr(eq + 1);
    Reject r = Reject::none;
    uint64_t n = 0;
    if (row->kind == Opt::NUMBER) {
      if (!bounded_number(v, row->digits, row->lo, row->hi, &n)) r = Reject::bad_value;
      else if (row->u32) *row->u32 = (uint32_t)n;
      else *row->u64 = n;
    } else if (row->kind == Opt::TEXT) {
      if (v.empty()) r = Reject::bad_value;
      else *row->text = v;
    } else {
      r = row->custom(v);
    }
    if (r == Reject::unknown_option) unknown_option(help, a);
    if (r == Reject::bad_value) usage_error(help, std::string("Bad value for --") + row->name + ": " + v);
  }
  return true;
}

// ---- the per-file scaffold -------------------------------------------------------------------------------------------------

// a zeroed struct of the C ABI with its struct_size set
template <class T>
static T fresh() {
  T s;
  std::memset(&s, 0, sizeof s);
  s.struct_size = sizeof s;
  return s;
}

// the message of a library call that failed: the pipeline's own detail if it left one, else the library's last one
static std::string library_error(int rc, const char* own_detail = "") {
  std::string msg = scfq_strerror(rc);
  const char* d = *own_detail ? own_detail : scfq_last_error_detail();
  if (d && *d) { msg += ": "; msg += d; }
  return msg;
}

// plain: stream == nil -> quit_error(..., 2) (fq_count.nim:35-36); .gz: the stream constructor raises -> exit 1 (sc.nim:299-305)
static int unable_to_open_code(const std::string& path) { return path.size() >= 3 && path.compare(path.size() - 3, 3, ".gz") == 0 ? 1 : 2; }
static std::string unable_to_open(const std::string& path) { return "Unable to open file: " + path; }
[[noreturn]] static void quit_unable_to_open(const std::string& path, int code) { quit_error(unable_to_open(path), code); }
[[noreturn]] static void quit_unable_to_open(const std::string& path) { quit_unable_to_open(path, unable_to_open_code(path)); }

// paired input: the first of the two that cannot be opened is the one the library stopped at (r2: NULL for interleaved input)
static const std::string& first_unopenable(const std::string& r1, const std::string* r2) {
  return (r2 && access(r1.c_str(), R_OK) == 0) ? *r2 : r1;
}

static const char* const kIndexOutOfBounds = "index out of bounds";
// fastq[^3 .. ^1] raises on a path shorter than three bytes; sc.nim:299-305 -> exit 1
static void require_suffix_room(const std::string& path) {
  if (path.size() < 3) quit_error(kIndexOutOfBounds, 1);
}

[[noreturn]] static void quit_no_fastq() { quit_error("No FASTQ specified", 3); }   // sc.nim:112-113

// -t / -b / -a: the header line and the filename columns behind every row (helpers.nim:200-224)
struct Columns {
  bool header = false, basename = false, absolute = false;
  // the three rows, behind the command's own
  std::vector<Opt> options(std::vector<Opt> own = {}) {
    own.push_back(opt_flag("header", 't', &header));
    own.push_back(opt_flag("basename", 'b', &basename));
    own.push_back(opt_flag("absolute", 'a', &absolute));
    return own;
  }
  std::string row(const std::string& line, const std::string& path) const { return output_w_fnames(line, path, basename, absolute); }
  void emit_row(const std::string& line, const std::string& path) const { std::printf("%s\n", row(line, path).c_str()); }
  // sc.nim:110-113: the header if asked for; without it, no file is an error
  void header_or_no_input(const std::string& names, bool no_files) const {
    if (header) std::printf("%s\n", output_header(names, basename, absolute).c_str());
    else if (no_files) quit_no_fastq();
  }
};

// A table whose length the file decides: call(rows, n_rows, &summary) once without rows for the sizes, then once more with
// want(summary) rows; no second call when that is 0.  The summary is fresh before each call.
template <class Row, class Summary, class Call, class Want>
static int size_then_fill(std::vector<Row>* rows, Summary* s, Call call, Want want) {
  rows->clear();
  *s = fresh<Summary>();
  int rc = call(static_cast<Row*>(nullptr), (uint64_t)0, s);
  if (rc != SCFQ_OK) return rc;
  rows->assign((size_t)want(*s), Row());
  if (rows->empty()) return rc;
  *s = fresh<Summary>();
  return call(rows->data(), (uint64_t)rows->size(), s);
}

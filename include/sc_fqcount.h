/*
 * sc_fqcount.h — C ABI of libsc_fqcount_hip.so, the MI355X (gfx950) drop-in for the
 * `sc fq-count` hot path of danielecook/seq-collection.
 *
 * What this boundary replaces in the reference (all paths relative to the reference tree):
 *   src/fq_count.nim:30-45   open stream (plain / ".gz"), per-line loop, i mod 4 classifier,
 *                            count("G")+count("C"), count("N"), line.len accumulation
 *   src/fq_count.nim:47-51   the five output fields and their `$` formatting
 *   gzip_stream.nim:13-23    readData == zlib gzread (the host inflate semantics kept here)
 * The reference has no FFI of its own for this path; the seam is the Nim proc
 *   fq_count*(fastq: string, basename: bool, absolute: bool)          (src/fq_count.nim:14)
 * A Nim host keeps that proc and calls scfq_count_file() + scfq_format_tsv() in place of
 * lines :30-51 (binding shown in INTEGRATION.md and seq-collection_amd/nim/fq_count.nim).
 *
 * Plain C: pointers and sizes only, no C++ types, no exceptions cross this boundary, the
 * library never calls exit() and never writes to stdout.
 */
#ifndef SC_FQCOUNT_H
#define SC_FQCOUNT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCFQ_ABI_VERSION 1u

/* ---- return codes (0 = success; negative = error) -------------------------------------- */
#define SCFQ_OK       0
#define SCFQ_EOPEN   (-1)  /* cannot open input: host maps to quit_error("Unable to open file: "&path, 2), src/fq_count.nim:35-36 */
#define SCFQ_EGZ     (-2)  /* zlib reported a corrupt / truncated gzip stream */
#define SCFQ_EHIP    (-3)  /* a HIP runtime call or kernel launch failed (no GPU, OOM, ...) */
#define SCFQ_ERCCL   (-4)  /* collective exchange failed */
#define SCFQ_EARG    (-5)  /* bad argument (NULL pointer, struct_size mismatch, bad flag) */
#define SCFQ_EIO     (-6)  /* read error after a successful open */
#define SCFQ_ENOMEM  (-7)  /* host allocation failed */
#define SCFQ_EPIPE   (-9)  /* the reader of an output descriptor went away (write -> EPIPE): `sc fq-dedup | head` ends quietly with
                              status 0 as the reference does for `errno: 32 Broken pipe` (sc.nim:304); every other write error is SCFQ_EIO */
#define SCFQ_ESPEC   (-8)  /* the speculative quality histogram of a shard backed a class that is not the quality line
                              (malformed input cut into shards): count that shard again with SCFQ_HIST_EXACT.
                              scfq_count_file / scfq_count_buffer do this by themselves and never return it. */

/* ---- option flags ------------------------------------------------------------------------ */
#define SCFQ_QUAL_HIST     0x1u  /* also build the 256-bin histogram of quality-line bytes (K3; not in reference) */
#define SCFQ_STRUCT_CHECK  0x2u  /* also count header lines not starting '@' / separator lines not starting '+' (K4) */
#define SCFQ_TIMING        0x4u  /* bracket the scan kernel with HIP events; read back with scfq_last_timing() */
#define SCFQ_PREV_IN_MEMORY 0x8u /* scfq_partial_buffer: the byte before `ptr` is addressable and is the look-behind halo */
#define SCFQ_WAIT_STREAM   0x20u /* order this call after the work already enqueued on scfq_opts.wait_stream (see there) */
#define SCFQ_HIST_EXACT    0x10u /* with SCFQ_QUAL_HIST: build all four class histograms exactly (slower kernel) instead of the
                                    verified-speculative form that only completes the quality class (scfq_partial.hist_class) */

/* ---- results: the counters of src/fq_count.nim:22-28 plus derivation inputs ------------- */
typedef struct scfq_counts {
  uint64_t struct_size;   /* caller sets to sizeof(scfq_counts) before the call */
  uint64_t abi_version;   /* library writes SCFQ_ABI_VERSION */
  uint64_t reads;         /* n_reads   = #{lines i : i mod 4 == 1}      fq_count.nim:40-41 */
  uint64_t gc_bases;      /* gc_cnt    = count("G")+count("C") on i mod 4 == 2   :43 */
  uint64_t n_bases;       /* n_cnt     = count("N")                              :44 */
  uint64_t bases;         /* total_len = sum line.len (EOL stripped)             :45 */
  uint64_t lines;         /* number of lines the reference's `lines(stream)` yields */
  uint64_t newlines;      /* number of '\n' bytes */
  uint64_t input_bytes;   /* bytes scanned (inflated bytes for .gz) */
  uint64_t bad_at;        /* K4: header lines whose first byte is not '@'   (0 unless SCFQ_STRUCT_CHECK) */
  uint64_t bad_plus;      /* K4: separator lines whose first byte is not '+' (0 unless SCFQ_STRUCT_CHECK) */
  uint64_t qual_hist[256];/* K3: byte histogram of quality lines (i mod 4 == 0), EOL bytes excluded; zeros unless SCFQ_QUAL_HIST */
} scfq_counts;

typedef struct scfq_opts {
  uint64_t struct_size;     /* sizeof(scfq_opts) */
  int32_t  n_devices;       /* 0 = use the current / default device only; >0 = shard byte ranges across device_ids[0..n) */
  const int32_t* device_ids;/* may be NULL when n_devices == 0 */
  uint32_t flags;           /* SCFQ_* option flags */
  uint32_t reserved;
  uint64_t chunk_bytes;     /* host->device staging chunk for file / host-buffer ingest; 0 = default (64 MiB) */
  /* ---- fields below exist when struct_size >= 48 (SCFQ_OPTS_V1_SIZE = 40 is still accepted) ---- */
  void*    wait_stream;     /* hipStream_t of the CALLER, read when SCFQ_WAIT_STREAM is set in flags (NULL then names the legacy
                               default stream). Device-pointer arguments (inputs and outputs) are used on library-private
                               non-blocking streams, which do not order against the stream that produced the input or last
                               used the output buffer. With SCFQ_WAIT_STREAM the library records an event on this stream at
                               entry and makes its own streams wait for it, so work already enqueued there completes first.
                               Without it the caller has synchronised (hipStreamSynchronize / hipDeviceSynchronize) before
                               the call. Every entry point synchronises its own streams before it returns, so results are
                               visible to any stream afterwards. */
} scfq_opts;
#define SCFQ_OPTS_V1_SIZE 40u

/*
 * The shard partial: what a contiguous byte range contributes when its line
 * phase at the first byte is unknown. Index r = (number of '\n' seen so far in THIS range) mod 4.
 * Flat u64 so it can be exchanged with one collective (RCCL uint64 / torch int64).
 *   combine  (A (+) B).nl = A.nl + B.nl ; (A (+) B).x[r] = A.x[r] + B.x[(r - A.nl) mod 4]
 * Associative, NOT commutative. Fold in file order from the identity.
 */
#define SCFQ_PARTIAL_WORDS 32
typedef struct scfq_partial {
  uint64_t nl;            /* '\n' count in range */
  uint64_t gc[4];         /* 'G'|'C' bytes per relative class */
  uint64_t n[4];          /* 'N' bytes per relative class */
  uint64_t len[4];        /* bytes that are not '\n' and not a '\r' directly before '\n' */
  uint64_t starts[4];     /* K4: line-start events (first byte of a line lies in this range) */
  uint64_t first_at[4];   /* K4: ... whose first byte is '@' */
  uint64_t first_plus[4]; /* K4: ... whose first byte is '+' */
  uint64_t bytes;         /* bytes covered */
  uint64_t last_byte;     /* value of the last byte covered (undefined when bytes == 0) */
  uint64_t hist_class;    /* K3 side array: 0 = all four class histograms are complete; k+1 (k = 0..3) = only class k is
                             (the speculative form histograms just the lines it verified to be quality lines);
                             5 = none (shards that disagree were combined: finalize returns SCFQ_ESPEC) */
  uint64_t reserved[4];   /* [0]: status word, OR-ed by the combine (scfq_count_file_sharded: a rank whose shard failed); the rest 0
                             (scfq_count_file_sharded carries a gzip shard's first byte, raw CRC-32 and length in them between its ranks) */
} scfq_partial;

#define SCFQ_HIST_WORDS (4 * 256)  /* optional K3 side array: uint64_t hist[4][256], class-major */

typedef struct scfq_timing {
  uint64_t struct_size;
  double scan_kernel_ms;  /* device time of the last scan launch(es) on the library stream (HIP events) */
  double fold_kernel_ms;  /* device time of the partial fold */
  uint64_t scan_bytes;    /* bytes those scan launches covered */
  uint64_t scan_launches;
  double host_fill_ms;    /* host time spent producing chunks (pread / zlib inflate) during the last ingest */
  double ingest_wall_ms;  /* wall time of the last chunked ingest (fill + copy + scan, overlapped) */
  uint64_t h2d_bytes;     /* bytes moved host -> HBM by the last ingest */
  double h2d_ms;          /* device time of those copies on the copy stream (HIP events) */
} scfq_timing;

/* ---- whole-input entry points (what a host binds) ---------------------------------------- */

/* Opens `path`; last three bytes ".gz" (case-sensitive, src/fq_count.nim:31) selects host zlib
 * inflate (gzread semantics incl. concatenated members, gzip_stream.nim:16-17) overlapped with
 * device scans via pinned buffers on a copy stream; otherwise plain pread. */
int scfq_count_file(const char* path, const scfq_opts* opts, scfq_counts* out);

/* Counts an in-memory FASTQ image. is_device != 0: `ptr` is a device pointer on the current
 * device (bytes already resident in HBM: the roofline configuration). */
int scfq_count_buffer(const void* ptr, uint64_t n, int is_device, const scfq_opts* opts, scfq_counts* out);

/* ---- shard-level entry points (multi-GPU / streaming hosts, tests of shard boundaries) --- */

/* Partial of one contiguous byte range. prev_byte: the byte immediately before the range in the
 * file (0..255), or -1 when the range starts the file. Needed because a '\r' directly before a
 * '\n' is not part of the line (look-behind halo of 1 byte). With SCFQ_PREV_IN_MEMORY set in
 * opts->flags prev_byte is ignored and ptr[-1] is read instead.
 * hist: NULL, or uint64_t[SCFQ_HIST_WORDS] (written only when SCFQ_QUAL_HIST is set). */
int scfq_partial_buffer(const void* ptr, uint64_t n, int is_device, int prev_byte,
                        const scfq_opts* opts, scfq_partial* out, uint64_t* hist);

void scfq_partial_identity(scfq_partial* p, uint64_t* hist);
/* acc = acc (+) b   (hist arrays may be NULL) */
int  scfq_partial_combine(scfq_partial* acc, const scfq_partial* b, uint64_t* hist_acc, const uint64_t* hist_b);
/* Interpret a partial folded from the start of the file: select the sequence class, derive
 * lines and reads (ceil(lines/4), src/fq_count.nim:39-41). */
int  scfq_partial_finalize(const scfq_partial* p, const uint64_t* hist, scfq_counts* out);

/* ---- C1: the cross-rank exchange of shard partials -----------------------------
 * The reference is one process with no collective (one call per file, sc.nim:114-116); the exchange exists because the
 * input is byte-range sharded across the GPUs of a node. Every rank contributes the partial of its shard; all ranks
 * receive the same rank-ordered (+) fold (an all-gather of the 32-word partials over RCCL / xGMI and the ordered combine —
 * NOT a sum-allreduce of counters: (+) is not commutative). librccl is dlopen()ed on first use.
 * A communicator runs its RCCL / HIP calls on its own worker thread; every wait has a deadline (timeout_ms, <= 0 means
 * 300 s) and a missing or stuck rank comes back as SCFQ_ERCCL, never as a hang. scfq_comm_error_detail() has the text.
 * One communicator per (process, device); calls on one communicator come from one host thread at a time. */
typedef struct scfq_comm scfq_comm;
#define SCFQ_COMM_ID_BYTES 128   /* sizeof(ncclUniqueId) */
#define SCFQ_COMM_RCCL 0         /* ncclAllGather of ncclUint64 on a private stream of the rank's device */
#define SCFQ_COMM_TCP  1         /* host sockets through rank 0: explicit opt-in for hosts without a common RCCL fabric and for
                                    CPU-only tests of the multi-process path; needs no device; never chosen by the library itself */

/* STDOUT: RCCL prints a version banner on stdout when a process's first communicator comes up. While any scfq_comm_init_* call
 * is in flight (communicator creation plus one warm-up collective) descriptor 1 of the process points at descriptor 2, and what
 * OTHER threads of the host write to stdout in that window lands on stderr. A host that prints from several threads creates
 * its communicators before its first row: scfq_prepare() below does that for the in-process multi-device path.
 * One process per GPU, the host distributes the id itself (rank 0 creates it, every rank passes the same bytes): */
int scfq_comm_unique_id(void* id, uint64_t cap /* >= SCFQ_COMM_ID_BYTES */);
int scfq_comm_init_rank(const void* id, int world, int rank, int device, int timeout_ms, scfq_comm** out);
/* One process per GPU, the library distributes the id: rank 0 listens on host:port (IPv4 name or address, NULL = 127.0.0.1),
 * the other ranks connect (retrying until the deadline). transport = SCFQ_COMM_RCCL | SCFQ_COMM_TCP. */
int scfq_comm_init_rendezvous(const char* host, int port, int world, int rank, int device, int transport, int timeout_ms,
                              scfq_comm** out);
/* One process, n distinct devices (ncclCommInitAll): out[k] is the communicator of device_ids[k], rank k. */
int scfq_comm_init_all(int n, const int32_t* device_ids, int timeout_ms, scfq_comm** out);
int scfq_comm_world(const scfq_comm* c);
int scfq_comm_rank(const scfq_comm* c);
/* 1 once an exchange on this communicator failed or timed out: every later call fails fast with SCFQ_ERCCL (an answer that
 * arrives after its deadline is dropped, never handed to a later exchange); destroy it and create a new one. */
int scfq_comm_is_broken(const scfq_comm* c);
const char* scfq_comm_transport(const scfq_comm* c);   /* "RCCL 2.x.y" | "tcp"; thread-local static storage */
/* folded = P_0 (+) P_1 (+) ... (+) P_{world-1}, identical on every rank. hist: NULL on every rank, or uint64_t[SCFQ_HIST_WORDS]
 * on every rank (then hist_folded receives the folded class histograms). */
int scfq_comm_exchange(scfq_comm* c, const scfq_partial* mine, const uint64_t* hist, scfq_partial* folded,
                       uint64_t* hist_folded, int timeout_ms);
/* The same in two halves, so that a host can scan shard k+1 while the exchange of shard k is in flight; finishes answer
 * starts in order. */
int scfq_comm_exchange_start(scfq_comm* c, const scfq_partial* mine, const uint64_t* hist, int timeout_ms);
int scfq_comm_exchange_finish(scfq_comm* c, scfq_partial* folded, uint64_t* hist_folded, int timeout_ms);
/* all[r * words + k] = word k of rank r (words <= 1056): barriers and max-over-ranks timings of a non-Python host. */
int scfq_comm_allgather_u64(scfq_comm* c, const uint64_t* mine, uint32_t words, uint64_t* all, int timeout_ms);
int scfq_comm_destroy(scfq_comm* c);
const char* scfq_comm_error_detail(void);   /* static, thread-local */

/* Optional warm-up for a host that is about to call scfq_count_file / scfq_count_buffer with these opts: creates the device
 * context(s) (streams, pinned staging) and, for opts->n_devices > 1 with distinct devices, the in-process RCCL communicators —
 * i.e. everything that would otherwise happen inside the first counting call, including the stdout window described above.
 * `sc fq-count` calls it before its first row. Safe to call more than once; returns SCFQ_OK or what the set-up returned. */
int scfq_prepare(const scfq_opts* opts);

/* fq_count of ONE file by all ranks of a communicator: rank r scans bytes [size*r/world, size*(r+1)/world) of `path` — cut at
 * arbitrary byte offsets, one byte of look-behind — on the current device (or opts->device_ids[0]), the partials are
 * exchanged, every rank receives the counters of the whole file.
 * ".gz" input: a BGZF (bgzip) file shards where its members are — rank r takes the members that start in its byte range (the
 * first cut at or after size*r/world where eight members follow one another; the byte in front of a rank's first inflated byte
 * comes from the member before the cut, inflated on the host), inflates them on its device and scans them; the ranks agree on
 * that with one extra all-gather of a word, and fall back together when any of them saw something else in its range.
 * An ordinary gzip file of SEVERAL members (cat a.gz b.gz, pigz -i, a sequencer's writer) shards where members start: a rank's
 * cut is the first position at or after size*r/world with the magic bytes, a header that parses and deflate data that inflates
 * cleanly; it inflates and scans the members of its stretch as if they began the input, and the byte in front of its first
 * inflated byte — the last byte of the rank before it — is put right when the gathered partials are folded.  A file of ONE member
 * (gzip, pigz) or of a few big ones (every rank finds at most one member start inside its share of the file) is cut where deflate
 * BLOCKS start, a member start being a cut of its own and no stretch crossing a member's end: every rank decodes its stretch to symbols, folds what the stretch does to the
 * 32 KiB window into a map and keeps the symbols; the ranks exchange their maps and compose them in rank order, which gives each
 * the window in front of its stretch; then the symbols become bytes, are checksummed and scanned (SCFQ_SHARD_GZ_KEEP=0: nothing
 * is kept, the stretch is decoded a second time); the member's CRC-32 and ISIZE are checked against the join of the stretches'.  What proves a cut, in both schemes, is the rank before it: its members (its chain of blocks) must end exactly where
 * the next rank began.  Whenever the ranks' findings do not join up — and for damaged files — rank 0 inflates and scans the whole
 * file with the readers scfq_count_file() uses (zlib gzread's bytes and errors), the other ranks contribute the identity.
 * Knobs: SCFQ_SHARD_BGZF / SCFQ_SHARD_GZ / SCFQ_SHARD_GZ_BLOCKS = 0 switch the three schemes off.
 * Collective: every rank must call it. */
int scfq_count_file_sharded(const char* path, const scfq_opts* opts, scfq_comm* comm, scfq_counts* out);

/* ---- K5: line index (record-boundary detection) ---------------------------------------------
 * Lines as the reference's `lines(stream)` yields them (src/fq_count.nim:38, src/fq_dedup.nim:42): record i of a FASTQ
 * is lines 4i .. 4i+3. For a device-resident input writes line_off[j] = offset of the first byte of line j for
 * j = 0 .. lines-1 and the sentinel line_off[lines] = offset one past the (real or implied) final '\n', so that line j
 * is bytes [line_off[j], line_off[j+1] - 1) before "\r\n" stripping. line_off_device: device memory of `cap` entries,
 * or NULL to only count. *lines_out is always set. One pass over the input: entries are written as they are found, so
 * when cap < lines + 1 the first cap entries are valid and the index is incomplete (size from *lines_out, call again). */
int scfq_index_lines(const void* device_ptr, uint64_t n, uint64_t* line_off_device, uint64_t cap, uint64_t* lines_out);

/* ---- `sc fq-dedup` (next row of SURVEY.md §8f): src/fq_dedup.nim:14-84 ------------------------
 * De-duplicate a FASTQ by read ID: every record (lines 4i .. 4i+3) whose header line equals the header line of an
 * earlier record is dropped, everything else is echoed, each line as text + '\n' (so "\r\n" comes out as "\n").
 * Replaces the reference's two streaming passes with Bloom filter + CountTable (:29,42-73) by an exact device
 * pipeline over the HBM-resident input: line index, header hashes, radix sort, exact compare inside equal-hash runs,
 * prefix sum of the kept lengths, gather. */
typedef struct scfq_dedup_stats {
  uint64_t struct_size;      /* caller sets to sizeof(scfq_dedup_stats) */
  uint64_t total_reads;      /* n_reads = lines div 4                             src/fq_dedup.nim:49 */
  uint64_t duplicates;       /* n_dups: records dropped                           :65 */
  uint64_t false_positive;   /* the reference's Bloom-filter diagnostic (:76-80); always 0 here: no Bloom filter */
  uint64_t records_out;      /* records echoed */
  uint64_t bytes_out;        /* bytes echoed */
  uint64_t hash_collisions;  /* header pairs with equal 64-bit hash and different text (resolved by the exact compare) */
} scfq_dedup_stats;

/* Input in host (is_device = 0) or device memory; the de-duplicated FASTQ is written to out (host or device memory of
 * out_cap bytes). *out_bytes is always set to the size of the result: out = NULL only sizes (returns SCFQ_OK), a too
 * small out returns SCFQ_EARG. */
int scfq_dedup_buffer(const void* ptr, uint64_t n, int is_device, void* out, uint64_t out_cap, int out_is_device,
                      uint64_t* out_bytes, scfq_dedup_stats* stats);
/* Stages the whole input (".gz" by suffix as src/fq_dedup.nim:32: zlib / BGZF inflate on the host) into HBM,
 * de-duplicates, writes the result to out_fd (what the reference echoes to stdout); out_fd < 0: statistics only. */
int scfq_dedup_file(const char* path, const scfq_opts* opts, int out_fd, scfq_dedup_stats* stats);
const char* scfq_dedup_error_detail(void);

/* ---- `sc fq-readstats` (addition; not in the reference): per-read length, G+C, N and quality ------------------
 * Lines are those of K5 above; record i is lines 4i .. 4i+3, reads = ceil(lines / 4) as scfq_counts.reads, a line a
 * truncated last record does not have is empty. All values are integers and exact. Device pipeline over the
 * HBM-resident input: line index (K5), R1 — a reduction segmented by record whose work is partitioned by BYTES (a
 * block per 32 KiB tile, so a 150-byte record and a 100 kB record cost the same per byte; a record inside one tile is
 * stored, a record that crosses a tile border is added to by every tile it touches) — and R2, the summary. */
typedef struct scfq_read_rec {
  uint64_t seq_len;       /* text length of line 4i+1 (EOL stripped as K5 does) */
  uint64_t gc_bases;      /* bytes 'G' or 'C' in it (case-sensitive, as scfq_counts.gc_bases) */
  uint64_t n_bases;       /* bytes 'N' in it */
  uint64_t qual_len;      /* text length of line 4i+3 */
  uint64_t qual_sum;      /* sum of its byte values (raw bytes, no Phred offset subtracted) */
} scfq_read_rec;

#define SCFQ_LEN_HIST_BINS   65
#define SCFQ_GC_HIST_BINS    102
#define SCFQ_MEANQ_HIST_BINS 256
typedef struct scfq_read_summary {
  uint64_t struct_size;   /* caller sets to sizeof(scfq_read_summary) before the call */
  uint64_t abi_version;   /* library writes SCFQ_ABI_VERSION */
  uint64_t reads;         /* ceil(lines / 4) */
  uint64_t lines;
  uint64_t input_bytes;   /* bytes scanned (inflated bytes for .gz) */
  uint64_t bases;         /* sum of seq_len */
  uint64_t gc_bases;
  uint64_t n_bases;
  uint64_t qual_bytes;    /* sum of qual_len */
  uint64_t qual_sum;
  uint64_t min_len;       /* over seq_len; 0 when reads == 0 */
  uint64_t max_len;
  /* seq_len in descending order, accumulated: Nx = the length of the read at which acc * 100 >= bases * x first holds,
   * Lx = how many reads were taken, that one included; all four 0 when bases == 0 */
  uint64_t n50, l50, n90, l90;
  uint64_t len_hist[SCFQ_LEN_HIST_BINS];     /* bin k: reads whose seq_len has bit length k (0 | 1 | 2-3 | 4-7 | ...) */
  uint64_t gc_hist[SCFQ_GC_HIST_BINS];       /* bin floor(100 * gc_bases / (seq_len - n_bases)); bin 101: denominator 0 */
  uint64_t meanq_hist[SCFQ_MEANQ_HIST_BINS]; /* bin floor(qual_sum / qual_len) of the reads with qual_len > 0 */
  uint64_t no_qual;       /* reads with qual_len == 0 (in no bin of meanq_hist) */
} scfq_read_summary;

/* Input in host (is_device = 0) or device memory. records_device: device memory for `cap` records that receives the
 * per-read table, or NULL for the summary only. A table with cap < reads returns SCFQ_EARG with out->reads (and lines,
 * input_bytes) set: size with NULL, call again. Device pointers follow the scfq_set_wait_stream contract of
 * scfq_index_lines. One device, the whole input resident, fewer than 2^31 records (SCFQ_EARG beyond, the text in
 * scfq_read_stats_error_detail()). */
int scfq_read_stats_buffer(const void* ptr, uint64_t n, int is_device, scfq_read_rec* records_device, uint64_t cap,
                           scfq_read_summary* out);
/* Stages the whole (inflated) input with scfq_stage_file, ".gz" and BGZF by suffix as everywhere else. */
int scfq_read_stats_file(const char* path, const scfq_opts* opts, scfq_read_summary* out);
/* "<reads>\t<bases>\t<min_len>\t<max_len>\t<mean_len>\t<n50>\t<l50>\t<n90>\t<l90>\t<mean_qual>" without trailing newline;
 * mean_len = bases / reads and mean_qual = qual_sum / qual_bytes as IEEE doubles printed by the rule of scfq_format_tsv
 * ("nan" for 0/0). Returns the number of bytes needed (excluding NUL); writes at most cap bytes incl. NUL. */
int scfq_format_read_stats_tsv(const scfq_read_summary* s, char* buf, uint64_t cap);
const char* scfq_read_stats_error_detail(void);   /* static, thread-local */

/* ---- `sc fq-cycles` (addition; not in the reference): base composition and quality position by position ---------
 * Lines and records are those of fq-readstats above. Every text byte b at 0-based position p of a sequence line (4i+1)
 * adds 1 to bases[p] and to exactly one of a, c, g, t, n at p when b is that upper-case letter (case-sensitive, as
 * scfq_counts.gc_bases); other = bases - a - c - g - t - n is not stored. Every text byte q at position p of a quality
 * line (4i+3) adds 1 to quals[p] and its raw value to qual_sum[p] (no Phred offset, as scfq_read_rec.qual_sum). All
 * values are integers and exact. Device pipeline over the HBM-resident input: line index (K5), a pass over its offsets
 * (line lengths), C1 — the counting kernel, partitioned by line group and position window, 32-bit counters in LDS per
 * block, flushed to 64-bit global counters — and a pass that turns the counters into rows, tail and total. */
typedef struct scfq_cycle_row {       /* 64 bytes */
  uint64_t bases, a, c, g, t, n;      /* sequence lines that have a byte at this position, and which byte */
  uint64_t quals, qual_sum;           /* quality lines that have a byte here, and the sum of those bytes */
} scfq_cycle_row;

typedef struct scfq_cycle_summary {
  uint64_t struct_size;   /* caller sets to sizeof(scfq_cycle_summary) before the call */
  uint64_t abi_version;   /* library writes SCFQ_ABI_VERSION */
  uint64_t reads;         /* ceil(lines / 4) */
  uint64_t lines;
  uint64_t input_bytes;   /* bytes scanned (inflated bytes for .gz) */
  uint64_t max_seq_len, max_qual_len; /* longest text of a line 4i+1 / 4i+3; 0 without one */
  uint64_t cycles;                    /* rows written: min(cap, max(max_seq_len, max_qual_len)) */
  scfq_cycle_row tail;                /* everything at positions >= cap, added up */
  scfq_cycle_row total;               /* every position added up: does not depend on cap */
} scfq_cycle_summary;

#define SCFQ_CYCLES_MAX_CAP (1ull << 24)
/* Input in host (is_device = 0) or device memory. rows_host: HOST memory for `cap` rows (may be NULL when cap is 0);
 * rows [0, cycles) are written, every field, rows [cycles, cap) are not touched. cap = 0 is the sizing call: everything
 * lands in tail, read max_seq_len / max_qual_len and call again. total, reads, lines, input_bytes and the two maxima do
 * not depend on cap, and rows[p] is the same for every cap > p. cap above SCFQ_CYCLES_MAX_CAP returns SCFQ_EARG (text in
 * scfq_cycles_error_detail()). Device pointers follow the scfq_set_wait_stream contract of scfq_index_lines. One
 * device, the whole input resident, fewer than 2^31 records, as scfq_read_stats_buffer. */
int scfq_cycles_buffer(const void* ptr, uint64_t n, int is_device, scfq_cycle_row* rows_host, uint64_t cap,
                       scfq_cycle_summary* out);
/* Stages the whole (inflated) input with scfq_stage_file, ".gz" and BGZF by suffix as everywhere else. */
int scfq_cycles_file(const char* path, const scfq_opts* opts, scfq_cycle_row* rows_host, uint64_t cap,
                     scfq_cycle_summary* out);
/* "<bases>\t<A>\t<C>\t<G>\t<T>\t<N>\t<other>\t<quals>\t<mean_qual>" without trailing newline; mean_qual = qual_sum /
 * quals as an IEEE double printed by the rule of scfq_format_tsv ("nan" for 0/0). Returns the number of bytes needed
 * (excluding NUL); writes at most cap bytes incl. NUL. */
int scfq_format_cycle_row_tsv(const scfq_cycle_row* r, char* buf, uint64_t cap);
const char* scfq_cycles_error_detail(void);   /* static, thread-local */

/* ---- `sc fq-kmers` (addition; not in the reference): the k-mer spectrum of the sequence lines ------------------------
 * Lines and records are those of fq-readstats above. For 1 <= k <= SCFQ_KMERS_MAX_K a window is k consecutive text bytes
 * of one sequence line (4i+1): a line of length L has max(0, L - k + 1) of them, and counts in short_lines when L < k. A
 * window is a k-mer iff every byte is exactly 'A', 'C', 'G' or 'T' (case-sensitive, as scfq_counts.gc_bases); any other
 * byte ('N', lower case, an interior '\r', high bytes) makes it skipped: windows = kmers + skipped. With the codes A = 0,
 * C = 1, G = 2, T = 3 and the first base most significant, index = sum of code[i] * 4^(k-1-i): index order is
 * lexicographic order, the table has 4^k entries. SCFQ_KMERS_CANONICAL counts a k-mer at min(index, rc(index)), rc being
 * the reverse complement (3 - code, reversed); a palindrome is counted once per occurrence, entries that are not their
 * own minimum stay 0. All values are integers and exact. Device pipeline over the HBM-resident input: line index (K5),
 * M1 — the counting kernel, partitioned by BYTES (a block owns a run of aligned 8 KiB steps and follows the lines through
 * the newlines it sees), 32-bit counters in LDS for k <= 7, 64-bit atomic adds on the table in HBM for k >= 8 — and M2,
 * a pass over the table for distinct and max_count. */
#define SCFQ_KMERS_MAX_K     12
#define SCFQ_KMERS_CANONICAL 0x1u
typedef struct scfq_kmer_summary {
  uint64_t struct_size;   /* caller sets to sizeof(scfq_kmer_summary) before the call */
  uint64_t abi_version;   /* library writes SCFQ_ABI_VERSION */
  uint64_t reads;         /* ceil(lines / 4) */
  uint64_t lines;
  uint64_t input_bytes;   /* bytes scanned (inflated bytes for .gz) */
  uint64_t k;
  uint64_t flags;
  uint64_t windows;       /* kmers + skipped */
  uint64_t kmers;         /* the sum of the table */
  uint64_t skipped;       /* windows with a byte that is not A C G T */
  uint64_t short_lines;   /* sequence lines shorter than k */
  uint64_t distinct;      /* non-zero entries of the table */
  uint64_t max_count;     /* the largest entry */
  uint64_t table_entries; /* 4^k */
} scfq_kmer_summary;

/* Input in host (is_device = 0) or device memory. table_host: HOST memory for `cap` entries. cap = 0 is the sizing and
 * summary call: the whole summary is filled (distinct and max_count included), table_host is not touched and may be NULL.
 * With cap >= 4^k entries [0, 4^k) are written and entries [4^k, cap) are not touched. The summary does not depend on cap.
 * SCFQ_EARG with text in scfq_kmers_error_detail(): 0 < cap < 4^k, k = 0 or k > SCFQ_KMERS_MAX_K, unknown flag bits;
 * SCFQ_EARG also for a NULL out or a wrong struct_size, NULL ptr with n > 0, NULL table_host with cap > 0. Device pointers
 * follow the scfq_set_wait_stream contract of scfq_index_lines. One device, the whole input resident, fewer than 2^31
 * records, as scfq_cycles_buffer; there is no CPU fallback (SCFQ_EHIP without a device). */
int scfq_kmers_buffer(const void* ptr, uint64_t n, int is_device, uint32_t k, uint32_t flags, uint64_t* table_host,
                      uint64_t cap, scfq_kmer_summary* out);
/* Stages the whole (inflated) input with scfq_stage_file, ".gz" and BGZF by suffix as everywhere else. */
int scfq_kmers_file(const char* path, const scfq_opts* opts, uint32_t k, uint32_t flags, uint64_t* table_host,
                    uint64_t cap, scfq_kmer_summary* out);
/* "<kmer>\t<count>" without trailing newline, e.g. "ACGT\t12": the k letters of `index`, first base first. Returns the
 * number of bytes needed (excluding NUL); writes at most cap bytes incl. NUL, as scfq_format_cycle_row_tsv. SCFQ_EARG for
 * k = 0, k > SCFQ_KMERS_MAX_K or index >= 4^k. */
int scfq_format_kmer_tsv(uint32_t k, uint64_t index, uint64_t count, char* buf, uint64_t cap);
const char* scfq_kmers_error_detail(void);    /* static, thread-local */

/* ---- `sc fq-adapters` (addition; not in the reference): adapter content by read position --------------------------------
 * Lines and records are those of fq-readstats above. A probe is 1 .. SCFQ_ADAPTERS_MAX_LEN letters, each exactly 'A',
 * 'C', 'G' or 'T'; a call takes 1 .. SCFQ_ADAPTERS_MAX_PROBES of them. Probe j of length m occurs at 0-based position p of
 * sequence line 4i+1 when the m text bytes from p are all inside that line's text and equal the probe byte for byte
 * (case-sensitive, as everywhere else; occurrences may overlap). A probe never occurs in a header, separator or quality
 * line, whatever those hold. hits[j] counts all occurrences of probe j; first(i, j) is the smallest position at which probe
 * j occurs in read i, or none; any(i) is the minimum of first(i, j) over the probes, or none. All values are integers and
 * exact. Device pipeline over the HBM-resident input: line index (K5), A1 — the matching kernel, partitioned by BYTES as
 * M1 of fq-kmers, with a 32-bit atomic minimum per (read, probe) —, A2, a pass over the reads that counts the first
 * positions into rows, and A3, their sum. Positions are kept in 32 bits: a sequence line of 2^32 - 1 bytes or more returns
 * SCFQ_EARG (text in scfq_adapters_error_detail()), nothing wraps. */
#define SCFQ_ADAPTERS_MAX_PROBES 8
#define SCFQ_ADAPTERS_MAX_LEN    32
#define SCFQ_ADAPTERS_MAX_CAP    (1ull << 24)
typedef struct scfq_adapter_row {                 /* 72 bytes */
  uint64_t first[SCFQ_ADAPTERS_MAX_PROBES];       /* reads whose first occurrence of probe j starts here */
  uint64_t any;                                   /* reads whose earliest occurrence of any probe starts here */
} scfq_adapter_row;

typedef struct scfq_adapter_summary {             /* 42 x 8 bytes */
  uint64_t struct_size;   /* caller sets to sizeof(scfq_adapter_summary) before the call */
  uint64_t abi_version;   /* library writes SCFQ_ABI_VERSION */
  uint64_t reads;         /* ceil(lines / 4) */
  uint64_t lines;
  uint64_t input_bytes;   /* bytes scanned (inflated bytes for .gz) */
  uint64_t n_probes;
  uint64_t max_seq_len;   /* longest text of a line 4i+1; 0 without one */
  uint64_t positions;     /* rows written: min(cap, max_seq_len) */
  uint64_t probe_len[SCFQ_ADAPTERS_MAX_PROBES];
  uint64_t hits[SCFQ_ADAPTERS_MAX_PROBES];
  scfq_adapter_row tail;  /* first occurrences at positions >= cap, added up */
  scfq_adapter_row total; /* every position added up: total.first[j] = reads that hold probe j, total.any = reads that hold one */
} scfq_adapter_summary;

/* Input in host (is_device = 0) or device memory. probes: n_probes NUL-terminated strings. rows_host: HOST memory for
 * `cap` rows (may be NULL when cap is 0); rows [0, positions) are written, every field, rows [positions, cap) are not
 * touched. cap = 0 is the sizing call: everything lands in tail, read max_seq_len and call again. total, hits, reads,
 * lines, input_bytes, max_seq_len and probe_len do not depend on cap, and rows[p] is the same for every cap > p. Slots
 * j >= n_probes are 0 everywhere. The same probe given twice is allowed: both columns are equal. SCFQ_EARG with text in
 * scfq_adapters_error_detail(): n_probes of 0 or above SCFQ_ADAPTERS_MAX_PROBES, a NULL or empty probe, a probe longer
 * than SCFQ_ADAPTERS_MAX_LEN, a probe byte that is not A C G T, cap above SCFQ_ADAPTERS_MAX_CAP, a sequence line too long
 * for 32-bit positions; SCFQ_EARG also for a NULL out or a wrong struct_size, NULL ptr with n > 0, NULL rows_host with
 * cap > 0, NULL probes. Device pointers follow the scfq_set_wait_stream contract of scfq_index_lines. One device, the
 * whole input resident, fewer than 2^31 records, as scfq_kmers_buffer; there is no CPU fallback (SCFQ_EHIP without a
 * device). */
int scfq_adapters_buffer(const void* ptr, uint64_t n, int is_device, const char* const* probes, uint32_t n_probes,
                         scfq_adapter_row* rows_host, uint64_t cap, scfq_adapter_summary* out);
/* Stages the whole (inflated) input with scfq_stage_file, ".gz" and BGZF by suffix as everywhere else. */
int scfq_adapters_file(const char* path, const scfq_opts* opts, const char* const* probes, uint32_t n_probes,
                       scfq_adapter_row* rows_host, uint64_t cap, scfq_adapter_summary* out);
/* Entry i of the built-in set (the 12-mers the common QC tools look for): *name and *seq point to static strings (either
 * may be NULL). Returns the size of the set; SCFQ_EARG for i beyond it. */
int scfq_adapters_default(uint32_t i, const char** name, const char** seq);
/* n_probes + 1 tab-separated fields (first[0 .. n_probes), any) without trailing newline: with counts != 0 the integers of
 * r, otherwise 100 * r->x / reads as IEEE doubles printed by the rule of scfq_format_tsv ("nan" for 0/0). Returns the
 * number of bytes needed (excluding NUL); writes at most cap bytes incl. NUL, as scfq_format_cycle_row_tsv. SCFQ_EARG for
 * a NULL r, n_probes of 0 or above SCFQ_ADAPTERS_MAX_PROBES. */
int scfq_format_adapter_row_tsv(const scfq_adapter_row* r, uint32_t n_probes, uint64_t reads, int counts, char* buf, uint64_t cap);
const char* scfq_adapters_error_detail(void); /* static, thread-local */

/* ---- `sc fq-insert-size` (addition; the reference reads insert sizes from an aligned BAM): read-pair overlap -------------
 * Inputs are two FASTQs, record i of each being pair i (pairs = min(reads1, reads2), unpaired = |reads1 - reads2|), or one
 * interleaved FASTQ, records 2i and 2i+1 being pair i (pairs = reads / 2, unpaired = reads & 1). Lines, records and line
 * ends are those of fq-readstats above: reads = ceil(lines / 4), a '\r' before a real '\n' is stripped, a sequence line the
 * input does not have is a text of length 0.
 * For pair i let A be the text of mate 1's sequence line (length La), B that of mate 2's (length Lb) and
 * C[y] = comp(B[Lb-1-y]), comp exchanging 'A' <-> 'T' and 'C' <-> 'G': the reverse complement of mate 2. A byte that is not
 * exactly one of A C G T never agrees with anything (case-sensitive, as everywhere else). For an offset d in
 * [-(Lb-1), La-1], C[y] faces A[y+d]: the overlap is the y in [max(0,-d), min(Lb, La-d)), ov(d) its size, mm(d) the number
 * of overlap positions at which A[y+d] and C[y] do not agree, and insert(d) = d + Lb, in 1 .. La+Lb-1 (d < 0: the mates
 * read through the insert into the adapters). An offset is accepted iff ov(d) >= min_overlap, mm(d) <= max_mismatches and
 * 100 * mm(d) <= max_mismatch_pct * ov(d). The pair's offset d* is the accepted offset with the largest ov; ties go to the
 * smallest mm, then to the largest d. Defaults 30 / 5 / 20; allowed min_overlap 1 .. 512, max_mismatches 0 .. 65535,
 * max_mismatch_pct 0 .. 100 (anything else: SCFQ_EARG, text in scfq_insert_size_error_detail()). A pair with La or Lb above
 * SCFQ_INSERT_MAX_LEN counts in too_long and is not analysed; of such a line only the bytes that tell its length are read.
 * The method sees inserts up to La + Lb - min_overlap only: a longer fragment's mates do not overlap (not_overlapped).
 * All values are integers and exact. Device pipeline over the HBM-resident inputs: line index (K5) of each, P1 — a wave per
 * pair: both reads as bit planes (two code bits and a valid bit per base, 64 bases per word), a lane per offset, shifts and
 * population counts, one packed-key minimum per wave; histogram in 32-bit LDS counters per block, flushed to 64-bit global
 * ones — and P2, a pass over the bins for min, max, mode and median. */
#define SCFQ_INSERT_MAX_LEN     512
#define SCFQ_INSERT_HIST_BINS   1024
#define SCFQ_INSERT_INTERLEAVED 0x1u
typedef struct scfq_overlap_rec {   /* 8 bytes; {0, 0, 0}: no accepted offset; {0, 0, 0xFFFF}: a too-long pair */
  int32_t  offset;                  /* d* */
  uint16_t overlap;                 /* ov(d*) */
  uint16_t mismatches;              /* mm(d*) */
} scfq_overlap_rec;

typedef struct scfq_insert_opts {
  uint64_t struct_size;             /* sizeof(scfq_insert_opts) */
  uint32_t flags;                   /* SCFQ_INSERT_INTERLEAVED */
  uint32_t min_overlap;
  uint32_t max_mismatches;
  uint32_t max_mismatch_pct;
} scfq_insert_opts;

typedef struct scfq_insert_summary {   /* 25 x 8 bytes */
  uint64_t struct_size;   /* caller sets to sizeof(scfq_insert_summary) before the call */
  uint64_t abi_version;   /* library writes SCFQ_ABI_VERSION */
  uint64_t reads1, reads2;             /* ceil(lines / 4) of each input (reads2 = lines2 = input_bytes2 = 0 for interleaved input) */
  uint64_t lines1, lines2;
  uint64_t input_bytes1, input_bytes2; /* bytes scanned (inflated bytes for .gz) */
  uint64_t pairs, unpaired;
  uint64_t overlapped, not_overlapped, too_long;   /* pairs = overlapped + not_overlapped + too_long */
  uint64_t read_through;               /* overlapped pairs with insert < max(La, Lb) */
  uint64_t overlap_bases, mismatches;  /* sums of ov(d*) and mm(d*) */
  uint64_t insert_sum, insert_sq_sum;  /* sums of insert(d*) and its square */
  uint64_t min_insert, max_insert;     /* 0 without an overlapped pair, as the next two */
  uint64_t mode_insert;                /* the smallest s with the largest count */
  uint64_t median_insert;              /* the smallest s with 2 * cum(s) >= overlapped */
  uint64_t min_overlap, max_mismatches, max_mismatch_pct;   /* the parameters as used */
} scfq_insert_summary;

/* r1 / r2 in host (is_device = 0) or device memory, both of one kind. opts = NULL: the defaults; with
 * SCFQ_INSERT_INTERLEAVED r1 is the interleaved input and r2 must be NULL with n2 = 0. recs_device: DEVICE memory for
 * rec_cap records that receives the per-pair table, entries [0, pairs), or NULL; rec_cap < pairs returns SCFQ_EARG with
 * out->pairs (and reads, lines, input_bytes) set, as scfq_read_stats_buffer. hist_host: HOST memory for exactly
 * SCFQ_INSERT_HIST_BINS entries, or NULL: entry s = pairs with insert s, entry 0 is always 0. SCFQ_EARG for a NULL out or
 * a wrong struct_size (out's or opts'), a NULL pointer with n > 0, NULL recs_device with rec_cap > 0; with text: unknown
 * flag bits, a parameter out of range, a second buffer with interleaved input. Device pointers follow the
 * scfq_set_wait_stream contract of scfq_index_lines. One device, both inputs whole and resident, fewer than 2^31 records
 * per input, as scfq_adapters_buffer; there is no CPU fallback (SCFQ_EHIP without a device). */
int scfq_insert_size_buffers(const void* r1, uint64_t n1, const void* r2, uint64_t n2, int is_device,
                             const scfq_insert_opts* opts, scfq_overlap_rec* recs_device, uint64_t rec_cap,
                             uint64_t* hist_host, scfq_insert_summary* out);
/* path2 = NULL: path1 is interleaved (SCFQ_INSERT_INTERLEAVED in iopts is then implied, and SCFQ_EARG with a path2). Stages
 * the whole (inflated) inputs with scfq_stage_file, ".gz" and BGZF by suffix as everywhere else. */
int scfq_insert_size_files(const char* path1, const char* path2, const scfq_opts* opts, const scfq_insert_opts* iopts,
                           scfq_overlap_rec* recs_device, uint64_t rec_cap, uint64_t* hist_host, scfq_insert_summary* out);
/* "<pairs>\t<overlapped>\t<percent_overlapped>\t<min>\t<median>\t<mean>\t<std_dev>\t<mode>\t<max>\t<read_through>\t
 * <mismatch_rate>" without trailing newline. percent_overlapped = 100 * overlapped / pairs, mean = insert_sum / overlapped,
 * std_dev = sqrt((double)(overlapped * insert_sq_sum - insert_sum^2)) / overlapped with the difference formed as an exact
 * 128-bit integer and converted once, mismatch_rate = mismatches / overlap_bases; IEEE doubles printed by the rule of
 * scfq_format_tsv ("nan" for 0/0). Returns the number of bytes needed (excluding NUL); writes at most cap bytes incl. NUL. */
int scfq_format_insert_size_tsv(const scfq_insert_summary* s, char* buf, uint64_t cap);
const char* scfq_insert_size_error_detail(void); /* static, thread-local */

/* ---- `sc fq-merge` (addition, not in the reference): overlapping read pairs become single reads -----------------------
 * Inputs, lines, records, pairs and `unpaired`; A, B, C = revcomp(B), La, Lb, d, ov, mm; the acceptance of an offset by
 * min_overlap / max_mismatches / max_mismatch_pct (defaults 30 / 5 / 20, the same ranges), the choice of d* and
 * SCFQ_INSERT_MAX_LEN are those of fq-insert-size above. One more parameter: phred_offset Q0, 33 (the default) or 64.
 * QA and QB are the texts of the two quality lines (line 4r+3). A quality byte the line does not have counts as the byte
 * Q0 (a line shorter than the sequence line, a record cut short); bytes of a quality line beyond the sequence length are
 * ignored. comp() maps A <-> T and C <-> G and leaves every other byte as it is; valid(b) holds when b is exactly one of
 * A C G T.
 * A pair with an accepted offset is MERGED. Its merged read has length s = d* + Lb, the insert: mate 1 starts the fragment
 * and C ends it. For x in [0, s): A covers x iff x < La; C covers x iff x >= d*, at y = x - d*, its source byte being
 * B[Lb-1-y] with quality QB[Lb-1-y]. At least one covers x; what lies outside [0, s) is read-through into adapter and is
 * dropped. Base and quality byte at x (qa, qc: the quality bytes of A and C there):
 *   only A covers                       A[x]                                           QA[x]
 *   only C covers                       comp(B[..])                                    QB[..]
 *   both cover, both valid, equal       that base                                      max(qa, qc)
 *   both cover, both valid, different   the one with the larger quality byte, mate 1   min(Q0 + max(2, |qa - qc|), 126)
 *                                       on a tie
 *   both cover, exactly one valid       the valid one                                  its own quality byte
 *   both cover, neither valid           A[x]                                           min(qa, qc)
 * (the two "both valid" rows are FLASH's rule). The merged record is the text of mate 1's header line, '\n', the merged
 * bases, '\n', "+\n", the merged quality bytes, '\n': len(header) + 2 s + 5 bytes; merged records appear in pair order.
 * A pair without an accepted offset, or a too-long pair, is UNMERGED: mate 1's record is echoed to the first unmerged
 * output and mate 2's to the second, exactly as fq-dedup echoes a kept record (each line the record has as text + '\n':
 * "\r\n" comes out as '\n', a last line without a newline gains one). With interleaved input both records go to the first
 * unmerged output, mate 1 then mate 2, and there is no second one. Records counted in `unpaired` go nowhere.
 * All values are integers and exact. Device pipeline over the HBM-resident inputs: line index (K5) of each, P1 of
 * fq-insert-size (the same kernel) into a table in pool memory, M1 — a thread per pair: the three output lengths, summed
 * per group of 32 pairs, and the sums of the statistics —, three exclusive scans over the groups, and M2 — a wave per
 * group: unmerged records are copied, merged ones built four positions per lane and stored as words. */
#define SCFQ_MERGE_INTERLEAVED 0x1u
typedef struct scfq_merge_opts {
  uint64_t struct_size;             /* sizeof(scfq_merge_opts) */
  uint32_t flags;                   /* SCFQ_MERGE_INTERLEAVED */
  uint32_t min_overlap;
  uint32_t max_mismatches;
  uint32_t max_mismatch_pct;
  uint32_t phred_offset;            /* 33 or 64 */
  uint32_t reserved;                /* 0 */
} scfq_merge_opts;

typedef struct scfq_merge_stats {      /* 26 x 8 bytes */
  uint64_t struct_size;   /* caller sets to sizeof(scfq_merge_stats) before the call */
  uint64_t abi_version;   /* library writes SCFQ_ABI_VERSION */
  uint64_t reads1, reads2;             /* as scfq_insert_summary, down to `unpaired` */
  uint64_t lines1, lines2;
  uint64_t input_bytes1, input_bytes2;
  uint64_t pairs, unpaired;
  uint64_t merged, not_overlapped, too_long;   /* pairs = merged + not_overlapped + too_long */
  uint64_t merged_bases;               /* sum of s */
  uint64_t overlap_bases, mismatches;  /* sums of ov(d*) and mm(d*): fq-insert-size's values on the same input */
  uint64_t took_mate1, took_mate2;     /* positions of the row "both valid, different" won by each mate */
  uint64_t neither_valid;              /* positions of the last row */
  uint64_t merged_bytes, unmerged1_bytes, unmerged2_bytes;   /* sizes of the three outputs, written or not */
  uint64_t min_overlap, max_mismatches, max_mismatch_pct, phred_offset;   /* the parameters as used */
} scfq_merge_stats;

/* r1 / r2 in host (is_device = 0) or device memory, both of one kind; with SCFQ_MERGE_INTERLEAVED r1 is the interleaved
 * input and r2 must be NULL with n2 = 0. opts = NULL: the defaults. The three outputs are all host (out_is_device = 0) or
 * all device memory. An output pointer of NULL with capacity 0 is not written; its size is reported in stats all the same,
 * so a call with three NULLs is the sizing call. An output that is too small returns SCFQ_EARG with text naming the output
 * and both sizes: stats is filled, every field, and NO byte is written to ANY output (M2 compares the scanned totals with
 * the capacities before it stores). un2 with interleaved input is SCFQ_EARG, with text. SCFQ_EARG for a NULL stats or a
 * wrong struct_size (stats' or opts'), a NULL input with n > 0, a NULL output with a capacity; with text in
 * scfq_merge_error_detail(): unknown flag bits, a parameter out of range, phred_offset other than 33 or 64, reserved not
 * 0, a second buffer with interleaved input. Device pointers follow the scfq_set_wait_stream contract of
 * scfq_index_lines. One device, inputs and outputs whole and resident, fewer than 2^31 records per input, as
 * scfq_insert_size_buffers; there is no CPU fallback (SCFQ_EHIP without a device). */
int scfq_merge_buffers(const void* r1, uint64_t n1, const void* r2, uint64_t n2, int is_device,
                       const scfq_merge_opts* opts, void* merged, uint64_t merged_cap, void* un1, uint64_t un1_cap,
                       void* un2, uint64_t un2_cap, int out_is_device, scfq_merge_stats* stats);
/* path2 = NULL: path1 is interleaved (SCFQ_MERGE_INTERLEAVED is then implied, and SCFQ_EARG with a path2; a un2_fd >= 0
 * is SCFQ_EARG then). Stages the whole (inflated) inputs with scfq_stage_file, ".gz" and BGZF by suffix as everywhere
 * else. A descriptor below 0: that output is not produced (its size is still in stats). The outputs are written one after
 * another, each in full: merged, then un1, then un2 — three pipes that one reader drains in lock-step would stall, give
 * each its own reader or use files. A reader that has gone away is SCFQ_EPIPE and any other failing write SCFQ_EIO, text
 * in scfq_merge_error_detail(), as scfq_dedup_file; stats is complete then. */
int scfq_merge_files(const char* path1, const char* path2, const scfq_opts* opts, const scfq_merge_opts* mopts,
                     int merged_fd, int un1_fd, int un2_fd, scfq_merge_stats* stats);
/* "<pairs>\t<merged>\t<percent_merged>\t<not_overlapped>\t<too_long>\t<unpaired>\t<merged_bases>\t<overlap_bases>\t
 * <mismatches>\t<took_mate1>\t<took_mate2>\t<neither_valid>\t<merged_bytes>\t<unmerged1_bytes>\t<unmerged2_bytes>" without
 * trailing newline; percent_merged = 100 * merged / pairs, an IEEE double printed by the rule of scfq_format_tsv ("nan" for
 * 0/0). Returns the number of bytes needed (excluding NUL); writes at most cap bytes incl. NUL. SCFQ_EARG for a NULL s. */
int scfq_format_merge_stats_tsv(const scfq_merge_stats* s, char* buf, uint64_t cap);
const char* scfq_merge_error_detail(void);       /* static, thread-local */

/* ---- `sc fq-trim` (addition, not in the reference): adapter, poly-G, quality and overlap trimming of the 3' ends ---------
 * Inputs are one FASTQ (single-end), two FASTQs (record i of each is pair i, pairs = min(reads1, reads2), unpaired the
 * difference) or, with SCFQ_TRIM_INTERLEAVED, one interleaved FASTQ (records 2i and 2i+1). Lines, records and texts are
 * those of fq-readstats above; a line the input does not have is empty. For a read, S is the text of its sequence line
 * (length L), Q that of its quality line (length LQ), q(i) = Q[i] - Q0 as a SIGNED integer and 0 for i >= LQ, Q0 being
 * phred_offset, 33 or 64.
 * A read with L > SCFQ_TRIM_MAX_LEN is too_long: no step looks at it and its record is echoed as fq-dedup echoes a kept
 * record (each line the record has as text + '\n'). Every other read gets ONE cut point e, starting at e = L; the steps
 * lower it in this order and each sees the read as S[0, e):
 *  1 Overlap (paired input, unless SCFQ_TRIM_NO_OVERLAP). The offset d* of fq-insert-size above is looked for with
 *    min_overlap / max_mismatches / max_mismatch_pct (defaults 30 / 5 / 20, the same ranges). A pair with an accepted
 *    offset has the insert s = d* + Lb, and both mates get e = min(L, s). A pair with a too-long mate has no offset.
 *  2 Adapters. 0 .. SCFQ_TRIM_MAX_PROBES probes of 1 .. 32 letters, each exactly 'A', 'C', 'G' or 'T' (the default set:
 *    scfq_adapters_default without the entries whose names begin with "poly", five probes). Probe j of length m matches
 *    at p in [0, e) iff t = min(m, e - p) >= min_adapter_overlap (1 .. 32, default 5) and, mm being the number of k in
 *    [0, t) with S[p+k] != probe[k] (byte for byte: 'N' and lower case are mismatches), 100 * mm <= adapter_mismatch_pct
 *    * t (0 .. 100, default 10). e becomes the smallest p at which a probe matches; adapter_reads[j] counts the read
 *    for the lowest j that matches there.
 *  3 Poly-G tail (poly_g, 0 = off, the default; 1 .. 512). g is the length of the longest suffix of S[0, e) that is all
 *    'G'; if g >= poly_g then e -= g.
 *  4 Quality window (window 1 .. 32, default 4; window_quality 0 .. 93, 0 = off, the default). p is the smallest
 *    position with p + window <= e and q(p) + .. + q(p + window - 1) < window_quality * window; if there is one, e = p.
 *  5 Minimum length (min_length 0 .. 512, default 15). A read with e < min_length is short. A short single-end read is
 *    dropped; a pair is dropped when either mate is short. A too-long read is never short.
 * The record of a kept read that is not too long: the header text, '\n', S[0, e), '\n', the text of the separator line,
 * '\n', Q[0, min(LQ, e)), '\n' — always four lines ("\r\n" comes out as '\n', a last line without a newline gains one).
 * Records keep their input order. Two inputs give out1 and out2, interleaved input one output (mate 1, then mate 2),
 * single-end input one output. Records counted in `unpaired` go nowhere and are counted nowhere else.
 * All values are integers and exact. Device pipeline over the HBM-resident inputs: line index (K5) of each, P1 of
 * fq-insert-size (the same kernel) for paired input, T1 — a wave per read: the read as bit planes, the probes against
 * every position by shifts and population counts, poly-G from the planes, the window sums from a wave prefix sum; 8 bytes
 * per read —, T2 — a thread per read or pair: output lengths per group of 32 and the statistics —, one exclusive scan per
 * output, and T3 — a wave per group: the records copied or written as their four pieces. */
#define SCFQ_TRIM_MAX_LEN      SCFQ_INSERT_MAX_LEN
#define SCFQ_TRIM_MAX_PROBES   8
#define SCFQ_TRIM_INTERLEAVED  0x1u
#define SCFQ_TRIM_NO_OVERLAP   0x2u
#define SCFQ_TRIM_NO_ADAPTERS  0x4u
typedef struct scfq_trim_opts {     /* 128 bytes */
  uint64_t struct_size;             /* sizeof(scfq_trim_opts) */
  uint32_t flags;                   /* SCFQ_TRIM_INTERLEAVED | SCFQ_TRIM_NO_OVERLAP | SCFQ_TRIM_NO_ADAPTERS */
  uint32_t min_overlap;
  uint32_t max_mismatches;
  uint32_t max_mismatch_pct;
  uint32_t min_adapter_overlap;
  uint32_t adapter_mismatch_pct;
  uint32_t poly_g;
  uint32_t window;
  uint32_t window_quality;
  uint32_t min_length;
  uint32_t phred_offset;            /* 33 or 64 */
  uint32_t n_probes;                /* 0 without SCFQ_TRIM_NO_ADAPTERS: the default set; with it: must be 0 */
  uint32_t reserved[2];             /* 0 */
  const char* probes[SCFQ_TRIM_MAX_PROBES];   /* entries [0, n_probes), NUL-terminated; the rest is not looked at */
} scfq_trim_opts;

typedef struct scfq_trim_stats {       /* 49 x 8 bytes */
  uint64_t struct_size;   /* caller sets to sizeof(scfq_trim_stats) before the call */
  uint64_t abi_version;   /* library writes SCFQ_ABI_VERSION */
  uint64_t reads1, reads2;             /* as scfq_insert_summary, down to `unpaired`; single-end: reads2 = pairs = unpaired = 0 */
  uint64_t lines1, lines2;
  uint64_t input_bytes1, input_bytes2;
  uint64_t pairs, unpaired;
  uint64_t reads_in, reads_out;        /* reads_in: reads1, or 2 * pairs; reads_in = reads_out + dropped_reads */
  uint64_t too_long;                   /* reads */
  uint64_t short_reads;                /* reads with e < min_length */
  uint64_t dropped_reads;              /* paired input: every read of a dropped pair */
  uint64_t bases_in, bases_out;        /* sums of L over reads_in and of e over reads_out */
  uint64_t cut_overlap, cut_adapter, cut_polyg, cut_quality;          /* reads the step lowered */
  uint64_t bases_overlap, bases_adapter, bases_polyg, bases_quality;  /* bases the step removed */
  uint64_t adapter_reads[SCFQ_TRIM_MAX_PROBES];   /* sum = cut_adapter */
  uint64_t bases_dropped;              /* sum of e over dropped reads (L for a too-long one) */
  uint64_t overlapped_pairs;           /* pairs with an accepted offset */
  uint64_t out1_bytes, out2_bytes;     /* sizes of the outputs, written or not */
  uint64_t flags, min_overlap, max_mismatches, max_mismatch_pct, min_adapter_overlap, adapter_mismatch_pct, poly_g, window,
      window_quality, min_length, phred_offset, n_probes;   /* the parameters as used */
} scfq_trim_stats;

/* r1 / r2 in host (is_device = 0) or device memory, both of one kind; r2 = NULL with n2 = 0: single-end input or, with
 * SCFQ_TRIM_INTERLEAVED, the interleaved one (the flag with a second buffer is SCFQ_EARG). opts = NULL: the defaults. The
 * outputs are both host (out_is_device = 0) or both device memory. An output pointer of NULL with capacity 0 is not
 * written; its size is reported in stats all the same, so a call with two NULLs is the sizing call. An output that is too
 * small returns SCFQ_EARG with text naming the output and both sizes: stats is filled, every field, and NO byte is written
 * to ANY output (T3 compares the scanned totals with the capacities before it stores). out2 without a second input is
 * SCFQ_EARG, with text. SCFQ_EARG for a NULL stats or a wrong struct_size (stats' or opts'), a NULL input with n > 0, a
 * NULL output with a capacity; with text in scfq_trim_error_detail(): unknown flag bits, a parameter out of range,
 * phred_offset other than 33 or 64, reserved not 0, more than SCFQ_TRIM_MAX_PROBES probes, probes together with
 * SCFQ_TRIM_NO_ADAPTERS, a NULL, empty or too long probe, a probe byte that is not A C G T. Device pointers follow the
 * scfq_set_wait_stream contract of scfq_index_lines. One device, inputs and outputs whole and resident, fewer than 2^31
 * records per input, as scfq_merge_buffers; there is no CPU fallback (SCFQ_EHIP without a device). */
int scfq_trim_buffers(const void* r1, uint64_t n1, const void* r2, uint64_t n2, int is_device, const scfq_trim_opts* opts,
                      void* out1, uint64_t cap1, void* out2, uint64_t cap2, int out_is_device, scfq_trim_stats* stats);
/* path2 = NULL: path1 is single-end or, with SCFQ_TRIM_INTERLEAVED in topts, interleaved (the flag with a path2 is
 * SCFQ_EARG; so is an out2_fd >= 0 without a path2). Stages the whole (inflated) inputs with scfq_stage_file, ".gz" and
 * BGZF by suffix as everywhere else. A descriptor below 0: that output is not produced (its size is still in stats). The
 * outputs are written one after another, each in full: out1, then out2. A reader that has gone away is SCFQ_EPIPE and any
 * other failing write SCFQ_EIO, text in scfq_trim_error_detail(), as scfq_merge_files; stats is complete then. */
int scfq_trim_files(const char* path1, const char* path2, const scfq_opts* opts, const scfq_trim_opts* topts, int out1_fd,
                    int out2_fd, scfq_trim_stats* stats);
/* "<reads_in>\t<reads_out>\t<dropped_reads>\t<short_reads>\t<too_long>\t<pairs>\t<unpaired>\t<overlapped_pairs>\t
 * <bases_in>\t<bases_out>\t<bases_dropped>\t<cut_overlap>\t<bases_overlap>\t<cut_adapter>\t<bases_adapter>\t<cut_polyg>\t
 * <bases_polyg>\t<cut_quality>\t<bases_quality>\t<adapter_reads>\t<out1_bytes>\t<out2_bytes>" without trailing newline,
 * all integers; <adapter_reads> is adapter_reads[0 .. n_probes) joined by ',', or "-" without a probe. Returns the number
 * of bytes needed (excluding NUL); writes at most cap bytes incl. NUL. SCFQ_EARG for a NULL s or n_probes above
 * SCFQ_TRIM_MAX_PROBES. */
int scfq_format_trim_stats_tsv(const scfq_trim_stats* s, char* buf, uint64_t cap);
const char* scfq_trim_error_detail(void);        /* static, thread-local */

/* ---- `sc fq-screen` (addition, not in the reference): k-mer contaminant screen and filter ----------------------------------
 * Which reads share k-mers with one of up to SCFQ_SCREEN_MAX_REFS named references, and optionally the reads that match
 * none of them (or, with SCFQ_SCREEN_KEEP_MATCHED, only those that match). Pairs stay in step.
 * References. 1 .. 16 references, reference r with a name of 1 .. 63 bytes without tab, newline or ':'; two references
 *  may not share a name. A reference is FASTA text by the fa-gc rule below: a header line is a line whose first byte is
 *  '>', every other line is a sequence line. A sequence byte is a byte 0x21 .. 0x7E of a sequence line (fa-gc's base: '\r'
 *  and blanks are none); 'a' .. 'z' are upper-cased. A contig is the sequence bytes between two header lines (or an end of
 *  the text); the bytes before the first header line are a contig of their own when there are any. A window is k
 *  consecutive sequence bytes of one contig: line ends do not break it, a header line does. A window is a k-mer iff every
 *  byte is then one of A C G T. Its key is the canonical index of fq-kmers above in 64 bits: codes A=0 C=1 G=2 T=3, first
 *  base most significant, key = min(index, index of the reverse complement); k = 8 .. SCFQ_SCREEN_MAX_K, default 31. The
 *  index is the set of keys, each with a 16-bit mask of the references that contain it. The sequence bytes of all
 *  references together are at most SCFQ_SCREEN_MAX_REF_BASES; a reference without a sequence byte is an error, one with
 *  fewer than k is not (it has no k-mer).
 * Reads. Lines, records and texts are those of fq-readstats above; S is the text of the sequence line, L its length (below
 *  2^32, otherwise unlimited). A read has max(0, L - k + 1) windows; a window is a k-mer iff every byte is EXACTLY 'A', 'C',
 *  'G' or 'T' (lower case and 'N' are not, as in fq-kmers and fq-trim), otherwise it is skipped. hits[r] is the number of
 *  the read's k-mers whose key is in the index with bit r. Reference r MATCHES the read iff hits[r] >= max(1, min_hits)
 *  (1 .. 65535, default 1) and 100 * hits[r] >= min_hit_pct * kmers (0 .. 100, default 0), kmers being the read's own number
 *  of k-mers. The read's mask is the set of matching references; best is the matching reference with the most hits, the
 *  lowest index on a tie, 0xFF without one (best_hits is then 0). A read with L < k has mask 0 and is a short read. A
 *  pair is matched iff either mate's mask is not 0; a single-end read iff its own is.
 * Outputs. out1 / out2 receive the records of the reads or pairs that are NOT matched (with SCFQ_SCREEN_KEEP_MATCHED: that
 *  are), in input order, each echoed as fq-dedup echoes a kept record: each line the record has as text + '\n'. Input
 *  forms and pairing are fq-trim's: one FASTQ; two (pairs = min(reads1, reads2), the rest `unpaired`, counted nowhere
 *  else); one interleaved FASTQ with SCFQ_SCREEN_INTERLEAVED (both mates to out1, no out2).
 * All values are integers and exact. Device pipeline: S0 on the host (the references into one upper-cased byte string with
 *  a separator between contigs), S1 — a thread per run of positions rolls both strands and inserts min(fwd, rc) into an
 *  open-addressing table of 64-bit keys (compare-and-swap, linear probing) and ORs the reference's bit into the slot's mask
 *  word —, a counting pass over the slots; per call: line index (K5), S2 — a wave per read: the read as 2-bit codes and an
 *  invalid-bit plane in LDS, every lane its windows by a funnel shift, a bit prefilter in LDS in front of the table probe;
 *  16 bytes per read —, S3 — a thread per read or pair: keep or not, output lengths per group of 32, the statistics —, one
 *  exclusive scan per output, S4 — a wave per group copies the kept records. Every probe loop is bounded by the number of
 *  slots and the table always has an empty slot. */
#define SCFQ_SCREEN_MAX_REFS       16
#define SCFQ_SCREEN_MAX_K          32
#define SCFQ_SCREEN_MAX_REF_BASES  (1ull << 27)
#define SCFQ_SCREEN_INTERLEAVED    0x1u
#define SCFQ_SCREEN_KEEP_MATCHED   0x2u
typedef struct scfq_screen_index scfq_screen_index;   /* opaque: the table on the device, names and per-reference numbers on the host */
typedef struct scfq_screen_ref {
  const char* name;      /* NUL-terminated */
  const void* text;      /* host memory: the FASTA text */
  uint64_t n;
} scfq_screen_ref;
typedef struct scfq_screen_ref_summary {
  uint64_t contigs, bases, windows, kmers;
  uint64_t distinct;     /* slots with bit r */
  uint64_t shared;       /* slots with bit r and another bit */
} scfq_screen_ref_summary;
typedef struct scfq_screen_summary {   /* 6 + 16 x 6 words */
  uint64_t struct_size;   /* caller sets to sizeof(scfq_screen_summary) before the call */
  uint64_t abi_version;   /* library writes SCFQ_ABI_VERSION */
  uint64_t n_refs, k;
  uint64_t distinct;      /* keys of the index */
  uint64_t slots;         /* of the table: a power of two, >= 1024, > the windows of all references */
  scfq_screen_ref_summary ref[SCFQ_SCREEN_MAX_REFS];
} scfq_screen_summary;
typedef struct scfq_screen_opts {
  uint64_t struct_size;   /* sizeof(scfq_screen_opts) */
  uint32_t flags;         /* SCFQ_SCREEN_INTERLEAVED | SCFQ_SCREEN_KEEP_MATCHED */
  uint32_t min_hits;      /* 1 .. 65535 */
  uint32_t min_hit_pct;   /* 0 .. 100 */
  uint32_t reserved;      /* 0 */
} scfq_screen_opts;
typedef struct scfq_screen_rec {   /* the per-read table: 16 bytes per read; paired input: mate m of pair p is entry 2p + m */
  uint32_t kmers;         /* k-mers of the read */
  uint32_t hit_kmers;     /* of them, those whose key is in the index at all */
  uint32_t best_hits;     /* hits[best], 0 without a match */
  uint16_t mask;
  uint8_t best;           /* 0xFF without a match */
  uint8_t reserved;       /* 0 */
} scfq_screen_rec;
typedef struct scfq_screen_stats {     /* 94 x 8 bytes */
  uint64_t struct_size;   /* caller sets to sizeof(scfq_screen_stats) before the call */
  uint64_t abi_version;   /* library writes SCFQ_ABI_VERSION */
  uint64_t reads1, reads2;             /* as scfq_trim_stats, down to `unpaired` */
  uint64_t lines1, lines2;
  uint64_t input_bytes1, input_bytes2;
  uint64_t pairs, unpaired;
  uint64_t reads_in, reads_out;        /* reads_in: reads1, or 2 * pairs; reads_in = reads_out + dropped_reads */
  uint64_t dropped_reads;              /* paired input: every read of a pair that is not written */
  uint64_t matched_reads;              /* reads with a mask other than 0 */
  uint64_t matched_pairs;              /* pairs with such a mate; single-end input: 0 */
  uint64_t multi_reads;                /* reads whose mask has two or more bits */
  uint64_t short_reads;                /* L < k */
  uint64_t bases_in, bases_out;        /* sums of L */
  uint64_t windows, kmers, skipped;    /* windows = kmers + skipped */
  uint64_t hit_kmers;
  uint64_t ref_reads[SCFQ_SCREEN_MAX_REFS];        /* reads with bit r */
  uint64_t ref_only_reads[SCFQ_SCREEN_MAX_REFS];   /* reads whose mask is exactly bit r: sum + multi_reads = matched_reads */
  uint64_t ref_best_reads[SCFQ_SCREEN_MAX_REFS];   /* sum = matched_reads */
  uint64_t ref_kmer_hits[SCFQ_SCREEN_MAX_REFS];    /* sum of hits[r] over reads_in */
  uint64_t out1_bytes, out2_bytes;     /* sizes of the outputs, written or not */
  uint64_t flags, min_hits, min_hit_pct, k, n_refs;   /* the parameters as used */
} scfq_screen_stats;

/* Builds the index of n_refs references in HOST memory; sum may be NULL. SCFQ_EARG with text in
 * scfq_screen_error_detail(), decided before any device call: k outside 8 .. 32, n_refs outside 1 .. 16, a NULL, empty,
 * too long or repeated name or one with a tab, newline or ':', a NULL text, a reference without a sequence byte, more than
 * SCFQ_SCREEN_MAX_REF_BASES sequence bytes, a forced table (SCFQ_SCREEN_TABLE_BITS) with no more slots than the
 * references have windows. SCFQ_EARG without text for a NULL out or a wrong sum->struct_size. *out is NULL after every
 * failure. The index lives on the device that is current at the call. */
int scfq_screen_index_buffers(const scfq_screen_ref* refs, uint32_t n_refs, uint32_t k, scfq_screen_index** out,
                              scfq_screen_summary* sum);
/* The same from files: ".gz" and BGZF by suffix (the library's readers inflate them), SCFQ_EOPEN for a file that cannot be
 * opened. names[i] = NULL: the file's base name up to its first '.'. */
int scfq_screen_index_files(const char* const* names, const char* const* paths, uint32_t n_refs, uint32_t k,
                            const scfq_opts* opts, scfq_screen_index** out, scfq_screen_summary* sum);
void scfq_screen_index_free(scfq_screen_index* index);   /* NULL is fine */
int scfq_screen_index_summary(const scfq_screen_index* index, scfq_screen_summary* sum);
/* the name of reference r, owned by the index; NULL for a NULL index or r >= n_refs */
const char* scfq_screen_ref_name(const scfq_screen_index* index, uint32_t r);
/* r1 / r2, the outputs, the sizing call, a too-small output (SCFQ_EARG naming it, stats complete, NO byte written to ANY
 * output: S4 compares the scanned totals with the capacities before it stores) and the device-pointer rules are those of
 * scfq_trim_buffers. recs_device: NULL, or DEVICE memory for rec_cap entries of the per-read table; fewer than reads_in is
 * SCFQ_EARG with text and nothing is written. SCFQ_EARG with text, before any launch: a NULL index, unknown flag bits,
 * min_hits or min_hit_pct out of range, reserved not 0, out2 without a second input, a second buffer with
 * SCFQ_SCREEN_INTERLEAVED. opts = NULL: the defaults. There is no CPU fallback (SCFQ_EHIP without a device). */
int scfq_screen_buffers(const scfq_screen_index* index, const void* r1, uint64_t n1, const void* r2, uint64_t n2,
                        int is_device, const scfq_screen_opts* opts, scfq_screen_rec* recs_device, uint64_t rec_cap,
                        void* out1, uint64_t cap1, void* out2, uint64_t cap2, int out_is_device, scfq_screen_stats* stats);
/* As scfq_trim_files: staged inputs, descriptors below 0 are not produced, out1 then out2, SCFQ_EPIPE / SCFQ_EIO.
 * recs_host: NULL, or HOST memory for rec_cap entries of the per-read table. */
int scfq_screen_files(const scfq_screen_index* index, const char* path1, const char* path2, const scfq_opts* opts,
                      const scfq_screen_opts* sopts, int out1_fd, int out2_fd, scfq_screen_rec* recs_host, uint64_t rec_cap,
                      scfq_screen_stats* stats);
/* One report row, without trailing newline. r < n_refs: "<name>\t<ref_bases>\t<ref_kmers>\t<reads_in>\t<ref_reads[r]>\t
 * <pct_reads>\t<ref_only_reads[r]>\t<ref_best_reads[r]>\t<ref_kmer_hits[r]>"; r = n_refs, the row "*": "*", the sums of
 * bases and kmers over the references, reads_in, matched_reads, its percentage, matched_reads - multi_reads, multi_reads,
 * hit_kmers. pct_reads = 10000 * reads / reads_in in integers (0 for reads_in = 0), printed with two decimals. Returns
 * the number of bytes needed (excluding NUL); writes at most cap bytes incl. NUL. SCFQ_EARG for a NULL argument, r >
 * n_refs, or stats of another index (n_refs or k differ). */
int scfq_format_screen_row_tsv(const scfq_screen_stats* s, const scfq_screen_index* index, uint32_t r, char* buf, uint64_t cap);
const char* scfq_screen_error_detail(void);      /* static, thread-local */

/* ---- `sc fq-demux` (addition, not in the reference): split reads by sample barcode ---------------------------------------
 * Inputs and units are fq-trim's: one FASTQ (a unit is a read), two FASTQs (unit i is record i of each, pairs =
 * min(reads1, reads2), the surplus is counted in `unpaired` and goes nowhere) or, with SCFQ_DEMUX_INTERLEAVED, one
 * interleaved FASTQ (records 2i and 2i+1). Lines, records and texts are those of fq-readstats above; a line the input does
 * not have is empty. There is no length limit on reads or headers.
 * Sheet. N = 1 .. SCFQ_DEMUX_MAX_SAMPLES samples, sample s with a name and one or two barcodes b1, b2 of 1 ..
 *  SCFQ_DEMUX_MAX_BARCODE letters, each exactly 'A', 'C', 'G' or 'T'; either every sample has a second barcode (a dual
 *  sheet) or none has. A name is 1 .. 63 bytes of [A-Za-z0-9._-], does not start with '.' and is not "undetermined". Two
 *  samples may share neither their name nor their (b1, b2) pair.
 * Where the barcode is read. Inline (the default): X1 is the sequence text S of the read, or of mate 1, X2 is S of mate 2;
 *  a dual sheet with single-end input is SCFQ_EARG. With SCFQ_DEMUX_HEADER: H is the header text of the read, or of mate 1
 *  (mate 2 is not consulted). Without a ':' in H both X1 and X2 are empty. Otherwise the tail is H behind its last ':'; if
 *  the tail holds a '+', X1 is the tail before its first '+' and X2 the tail behind it, if not, X1 is the tail and X2 is
 *  empty (CASAVA 1.8: "@... 1:N:0:ACGTACGT+TGCATGCA").
 * Assignment, in integers. m1 = |b1|, m2 = |b2| (0 on a single-index sheet). Sample s is ELIGIBLE iff |X1| >= m1 and
 *  |X2| >= m2; mmk(s) is the number of i < mk with Xk[i] != bk[i], byte for byte ('N' and lower case are mismatches); s
 *  MATCHES iff it is eligible and mm1 <= M and mm2 <= M, M = mismatches (0 .. 3, default 1); t(s) = mm1 + mm2. The unit
 *  goes to the matching sample with the smallest t and, among equal t, the larger m1 + m2 ("ACGTAA" wins over "ACGT").
 *  Two or more matching samples that share the best (t, m1 + m2): the unit is AMBIGUOUS. No eligible sample: NO_BARCODE.
 *  Eligible samples but no matching one: UNMATCHED. These three kinds are UNDETERMINED, which is destination N.
 * Records. Every written record has four lines, as fq-trim's: the header text, '\n', the sequence, '\n', the text of the
 *  separator line, '\n', the quality, '\n' ("\r\n" comes out as '\n', a last line without a newline gains one). Inline
 *  mode without SCFQ_DEMUX_KEEP_BARCODE: mate k (k = 1, 2) of a unit assigned to s, with mk > 0, is written with
 *  S[mk, L) and Q[min(LQ, mk), LQ) — L = mk gives an empty sequence line. Everything else is written unclipped:
 *  undetermined units, header mode, mate 2 under a single-index sheet.
 * Layout. out1 (and out2 for two inputs) holds the records of destination 0, then 1, .., N - 1, then the undetermined
 *  ones; each destination in input order. Interleaved input gives one output, mate 1 then mate 2 of each pair. The mates
 *  of unit u have the same rank within the same destination of out1 and out2.
 * All values are integers and exact. Device pipeline over the HBM-resident inputs: line index (K5) of each, X1 — a lane
 *  per unit: the candidate's first 32 bytes as 2-bit codes and a plane of bytes that are not A C G T, every sample of the
 *  sheet against them by XOR, fold and population count; 8 bytes and a sort key per unit —, a stable radix sort of (key,
 *  unit) over the key's bits, X2 — a thread per sorted position: record lengths per group of 32 and the rows —, one
 *  exclusive scan per output, X3 — a wave per group gathers the records from where they lie in the input and writes them
 *  one behind the other. */
#define SCFQ_DEMUX_MAX_SAMPLES   1024
#define SCFQ_DEMUX_MAX_BARCODE   32
#define SCFQ_DEMUX_INTERLEAVED   0x1u
#define SCFQ_DEMUX_HEADER        0x2u
#define SCFQ_DEMUX_KEEP_BARCODE  0x4u
#define SCFQ_DEMUX_ASSIGNED      0
#define SCFQ_DEMUX_UNMATCHED     1
#define SCFQ_DEMUX_AMBIGUOUS     2
#define SCFQ_DEMUX_NO_BARCODE    3
typedef struct scfq_demux_sheet scfq_demux_sheet;   /* opaque, host memory only: names, barcodes and their packed form */
typedef struct scfq_demux_sample {
  const char* name;        /* NUL-terminated */
  const char* barcode1;    /* NUL-terminated */
  const char* barcode2;    /* NUL-terminated, or NULL: no second barcode */
} scfq_demux_sample;
typedef struct scfq_demux_opts {       /* 24 bytes */
  uint64_t struct_size;   /* sizeof(scfq_demux_opts) */
  uint32_t flags;         /* SCFQ_DEMUX_INTERLEAVED | SCFQ_DEMUX_HEADER | SCFQ_DEMUX_KEEP_BARCODE */
  uint32_t mismatches;    /* M: 0 .. 3 (opts = NULL: 1) */
  uint32_t reserved[2];   /* 0 */
} scfq_demux_opts;
typedef struct scfq_demux_row {        /* one destination: 64 bytes; entry N is the undetermined one */
  uint64_t units;
  uint64_t perfect;       /* units with t = 0; 0 for the undetermined row */
  uint64_t mismatched;    /* units with t > 0: units = perfect + mismatched for a sample */
  uint64_t bases_out;     /* sequence bytes written, both mates */
  uint64_t bytes1, bytes2;   /* the destination's bytes in out1 and out2 */
  uint64_t off1, off2;    /* where they begin: destination d is out1[off1, off1 + bytes1) and out2[off2, off2 + bytes2) */
} scfq_demux_row;
typedef struct scfq_demux_rec {        /* the per-unit table: 8 bytes per unit */
  uint16_t sample;        /* 0xFFFF when undetermined */
  uint8_t mm1, mm2;       /* of that sample; 0xFF when undetermined */
  uint8_t state;          /* SCFQ_DEMUX_ASSIGNED, _UNMATCHED, _AMBIGUOUS or _NO_BARCODE */
  uint8_t reserved[3];    /* 0 */
} scfq_demux_rec;
typedef struct scfq_demux_stats {      /* 29 x 8 bytes */
  uint64_t struct_size;   /* caller sets to sizeof(scfq_demux_stats) before the call */
  uint64_t abi_version;   /* library writes SCFQ_ABI_VERSION */
  uint64_t reads1, reads2;             /* as scfq_trim_stats, down to `unpaired` */
  uint64_t lines1, lines2;
  uint64_t input_bytes1, input_bytes2;
  uint64_t pairs, unpaired;
  uint64_t units_in;                   /* reads1, or pairs: units_in = assigned + undetermined */
  uint64_t assigned, undetermined;
  uint64_t no_barcode, unmatched, ambiguous;   /* sum = undetermined */
  uint64_t perfect, mismatched;        /* sum = assigned */
  uint64_t reads_in, reads_out;        /* reads1, or 2 * pairs; equal: nothing is dropped */
  uint64_t bases_in, bases_out, bases_clipped;   /* sums of L over reads_in; bases_in = bases_out + bases_clipped */
  uint64_t out1_bytes, out2_bytes;     /* sizes of the outputs, written or not */
  uint64_t flags, mismatches, n_samples, dual;   /* the parameters as used */
} scfq_demux_stats;

/* The sheet of n samples. SCFQ_EARG with text in scfq_demux_error_detail(), all decided on the host: n outside 1 ..
 * SCFQ_DEMUX_MAX_SAMPLES, a NULL, empty, too long, reserved or repeated name or one with another byte, a NULL, empty or too
 * long barcode1, a barcode byte that is not A C G T, a second barcode on some samples only, a repeated (barcode1, barcode2)
 * pair. SCFQ_EARG without text for a NULL out. *out is NULL after every failure. No device is touched. */
int scfq_demux_sheet_new(const scfq_demux_sample* samples, uint32_t n, scfq_demux_sheet** out);
void scfq_demux_sheet_free(scfq_demux_sheet* sheet);   /* NULL is fine */
uint32_t scfq_demux_sheet_samples(const scfq_demux_sheet* sheet);   /* N; 0 for a NULL sheet */
/* the name of sample s, owned by the sheet; "undetermined" for s = N; NULL for a NULL sheet or s > N */
const char* scfq_demux_sheet_name(const scfq_demux_sheet* sheet, uint32_t s);
/* r1 / r2, the outputs, the sizing call (both outputs NULL), a too-small output (SCFQ_EARG naming it, stats and rows
 * complete, NO byte written to ANY output: the host compares the scanned totals with the capacities before X3 is launched)
 * and the device-pointer rules are those of scfq_trim_buffers. rows_host: HOST memory for row_cap entries, N + 1 of which are
 * written; row_cap < N + 1 is SCFQ_EARG with text before any launch. recs_device: NULL, or DEVICE memory for rec_cap entries
 * of the per-unit table; fewer than units_in is SCFQ_EARG with text and nothing is written. SCFQ_EARG with text, before any
 * device call: a NULL sheet, unknown flag bits, mismatches above 3, reserved not 0, out2 without a second input, a second
 * buffer with SCFQ_DEMUX_INTERLEAVED, a dual sheet with single-end input in inline mode. opts = NULL: the defaults. One
 * device, inputs and outputs whole and resident, fewer than 2^31 records per input; there is no CPU fallback (SCFQ_EHIP
 * without a device). */
int scfq_demux_buffers(const scfq_demux_sheet* sheet, const void* r1, uint64_t n1, const void* r2, uint64_t n2, int is_device,
                       const scfq_demux_opts* opts, scfq_demux_rec* recs_device, uint64_t rec_cap, scfq_demux_row* rows_host,
                       uint64_t row_cap, void* out1, uint64_t cap1, void* out2, uint64_t cap2, int out_is_device,
                       scfq_demux_stats* stats);
/* path2 = NULL: path1 is single-end or, with SCFQ_DEMUX_INTERLEAVED in dopts, interleaved (the flag with a path2 is
 * SCFQ_EARG). Stages the whole (inflated) inputs with scfq_stage_file, ".gz" and BGZF by suffix as everywhere else.
 * out_dir = NULL: report only. Otherwise the directory has to exist, and every destination gets a file in it, created or
 * truncated, empty for a destination without a unit: <out_dir>/<name>.fq for one input, <out_dir>/<name>_R1.fq and
 * <out_dir>/<name>_R2.fq for two, the undetermined units under the name "undetermined". One descriptor is open at a time
 * (2050 files are more than a common `ulimit -n`). A file that cannot be created is SCFQ_EIO with text; a failing write is
 * SCFQ_EPIPE / SCFQ_EIO as scfq_merge_files; stats and rows are complete then. recs_host: NULL, or HOST memory for rec_cap
 * entries of the per-unit table. */
int scfq_demux_files(const scfq_demux_sheet* sheet, const char* path1, const char* path2, const scfq_opts* opts,
                     const scfq_demux_opts* dopts, const char* out_dir, scfq_demux_rec* recs_host, uint64_t rec_cap,
                     scfq_demux_row* rows_host, uint64_t row_cap, scfq_demux_stats* stats);
/* One report row, without trailing newline, of destination d = 0 .. N with its row of the call that filled s:
 * "<sample>\t<barcode>\t<units>\t<pct_units>\t<perfect>\t<mismatched>\t<bases_out>\t<bytes1>\t<bytes2>". <barcode> is
 * barcode1, or barcode1 + '+' + barcode2; the row of d = N is named "undetermined" with the barcode "-". pct_units = 10000 *
 * units / units_in in integers (0 for units_in = 0), printed with two decimals, as fq-screen's. Returns the number of bytes
 * needed (excluding NUL); writes at most cap bytes incl. NUL. SCFQ_EARG for a NULL argument, d > N, or stats of another
 * sheet (n_samples differs). */
int scfq_format_demux_row_tsv(const scfq_demux_stats* s, const scfq_demux_sheet* sheet, uint32_t d, const scfq_demux_row* row,
                              char* buf, uint64_t cap);
const char* scfq_demux_error_detail(void);       /* static, thread-local */

/* ---- `sc fq-kcount` (addition; not in the reference): k-mer counts for k = 13 .. 32 in a hash table on the device -----
 * Lines, records, windows, k-mers, skipped and short_lines are exactly those of fq-kmers above; so is the key (codes A = 0,
 * C = 1, G = 2, T = 3, first base most significant, here in 64 bits) and the canonical mode (a k-mer is counted at
 * min(key, rc(key)); a palindrome once per occurrence). Where fq-kmers holds 4^k counters, this one holds the keys that
 * occur: an open-addressing table of (key, count) slots, linear probing, a power of two of slots. Every value is an
 * integer and exact; counts are 64 bits.
 *   Inputs.  One input (r2 = NULL, n2 = 0) or two, which are counted into ONE table: reads, lines, windows and the rest are
 *            the sums over both. The two are not paired and their lengths may differ.
 *   Sizing.  opts->table_bits = 0: the table starts at the power of two >= 2 * (n1 + n2) slots (at least 2^10, at most
 *            2^30; SCFQ_KCOUNT_START_BITS in the environment lowers it) and grows fourfold per failed pass while it fits
 *            into half of the free device memory. table_bits = 10 .. 32: that size and no growth. A pass fails when a key
 *            found no slot within the probe bound (512 slots with automatic sizing, min(slots, 4096) with table_bits;
 *            SCFQ_KCOUNT_MAX_PROBE overrides both); a failed pass is thrown away whole and the input, which is resident,
 *            is counted again: no count is ever applied twice. SCFQ_EFULL: the table named by table_bits could not hold
 *            the keys (or could not be allocated), or growth ran out of device memory; the detail names the slot count.
 *   Summary. Every field but slots and passes is independent of table_bits. kmers is the sum of the counts in the table,
 *            windows and skipped are counted by the lanes that see the windows: windows = kmers + skipped compares two
 *            counts made in different ways. slots and passes are diagnostics: the size of the table of the last pass
 *            and the number of passes over the input (one with a table that is large enough). */
#define SCFQ_KCOUNT_MIN_K     13
#define SCFQ_KCOUNT_MAX_K     32
#define SCFQ_KCOUNT_CANONICAL 0x1u
#define SCFQ_EFULL   (-10) /* fq-kcount: the hash table could not hold the keys (see Sizing above) */
typedef struct scfq_kcount scfq_kcount;          /* opaque: the table on the device */
typedef struct scfq_kcount_opts {
  uint64_t struct_size;   /* caller sets to sizeof(scfq_kcount_opts) */
  uint32_t k;             /* SCFQ_KCOUNT_MIN_K .. SCFQ_KCOUNT_MAX_K */
  uint32_t flags;         /* SCFQ_KCOUNT_CANONICAL */
  uint32_t table_bits;    /* 0: automatic; 10 .. 32: 2^table_bits slots, no growth */
  uint32_t reserved;      /* 0 */
} scfq_kcount_opts;
typedef struct scfq_kcount_summary {
  uint64_t struct_size;   /* caller sets to sizeof(scfq_kcount_summary) before the call */
  uint64_t abi_version;   /* library writes SCFQ_ABI_VERSION */
  uint64_t reads;         /* (lines + 3) / 4 per input, summed */
  uint64_t lines;
  uint64_t input_bytes;
  uint64_t k;
  uint64_t flags;
  uint64_t windows;       /* kmers + skipped */
  uint64_t kmers;         /* the sum of the counts in the table */
  uint64_t skipped;       /* windows with a byte that is not A C G T */
  uint64_t short_lines;   /* sequence lines with fewer than k text bytes */
  uint64_t distinct;      /* keys in the table */
  uint64_t unique;        /* keys whose count is 1 */
  uint64_t max_count;
  uint64_t slots;         /* diagnostic: slots of the table of the last pass */
  uint64_t passes;        /* diagnostic: passes over the input */
} scfq_kcount_summary;
typedef struct scfq_kmer_count { uint64_t key, count; } scfq_kmer_count;

/* Counts the k-mers of one or two inputs in host (is_device = 0) or device memory. out: receives the table, to be freed
 * with scfq_kcount_free, or NULL for the summary only; sum: the whole summary either way, or NULL. At least one of the two
 * is given. *out is NULL after every failure. SCFQ_EARG with text in scfq_kcount_error_detail(), found before any HIP call:
 * k outside 13 .. 32, unknown flag bits, table_bits not 0 and outside 10 .. 32, a non-zero reserved, a wrong struct_size
 * (opts' or sum's), a NULL opts, a NULL input with n > 0, a second input without a first. Device pointers follow the
 * scfq_set_wait_stream contract of scfq_index_lines and may have any alignment. One device, the whole input resident,
 * fewer than 2^31 records per input; there is no CPU fallback (SCFQ_EHIP without a device). */
int scfq_kcount_buffers(const void* r1, uint64_t n1, const void* r2, uint64_t n2, int is_device, const scfq_kcount_opts* opts,
                        scfq_kcount** out, scfq_kcount_summary* sum);
/* The same from files (path2 may be NULL): the whole (inflated) inputs are staged with scfq_stage_file, ".gz" and BGZF by
 * suffix as everywhere else; SCFQ_EOPEN for a file that cannot be opened. */
int scfq_kcount_files(const char* path1, const char* path2, const scfq_opts* opts, const scfq_kcount_opts* kopts,
                      scfq_kcount** out, scfq_kcount_summary* sum);
/* The multiplicity histogram, 2 <= bins <= 2^20 entries of HOST memory: hist[0] = 0, hist[c] for 1 <= c <= bins - 2 is the
 * number of keys with count c, hist[bins - 1] the number of keys with count >= bins - 1: the sum is `distinct`. SCFQ_EARG
 * for a NULL argument or bins out of range. hist, dump and query work in device memory that belongs to the table (8 MiB
 * behind its slots, allocated with it; they take none of their own), so the calls on one table run one after the other:
 * a second thread's call waits. Calls on different tables do not wait for each other. */
int scfq_kcount_hist(const scfq_kcount* t, uint64_t* hist_host, uint64_t bins);
/* The keys with min_count <= count (and count <= max_count unless that is 0) in ascending key order, sorted on the host
 * (the table is read in pieces of 2^19 slots, each piece's rows copied behind the last one's).
 * *total is always the number of keys that qualify; with cap < *total nothing is written and the call still returns 0 (as
 * snprintf sizes); entries behind *total are not touched. out_host may be NULL with cap = 0. */
int scfq_kcount_dump(const scfq_kcount* t, uint64_t min_count, uint64_t max_count, scfq_kmer_count* out_host, uint64_t cap,
                     uint64_t* total);
/* counts_host[i] = the count of keys_host[i], 0 for a key that is absent. The keys are plain indices; in canonical mode the
 * library takes the minimum with the reverse complement itself. A key >= 4^k: SCFQ_EARG, the text names it, nothing is
 * written. n = 0 is valid. */
int scfq_kcount_query(const scfq_kcount* t, const uint64_t* keys_host, uint64_t n, uint64_t* counts_host);
void scfq_kcount_free(scfq_kcount* t);           /* NULL is fine */
/* "<kmer>\t<count>" without trailing newline: the k letters of `key`, first base first. Returns the number of bytes needed
 * (excluding NUL); writes at most cap bytes incl. NUL, as scfq_format_kmer_tsv. SCFQ_EARG for k outside 13 .. 32 or
 * key >= 4^k. */
int scfq_format_kcount_tsv(uint32_t k, uint64_t key, uint64_t count, char* buf, uint64_t cap);
const char* scfq_kcount_error_detail(void);      /* static, thread-local */

/* ---- `sc fq-normalize` (addition; not in the reference): k-mer depth normalization of reads against an fq-kcount table ----
 * For every read, how often its k-mers occur in a table of scfq_kcount; reads of over-covered regions are thinned to a target
 * depth, reads whose k-mers are almost all rare are dropped (BBNorm, khmer's normalize-by-median, in one pass over resident
 * input). Every value is an integer and exact.
 *   Taken over. Lines, records, texts, read forms and pairing are fq-trim's / fq-screen's: one FASTQ (a unit is a read); two
 *            (unit p is record p of each, pairs = min(reads1, reads2), the rest `unpaired`, counted nowhere else); one
 *            interleaved FASTQ with SCFQ_NORM_INTERLEAVED (records 2p and 2p + 1). Windows, k-mers (every byte EXACTLY
 *            A C G T), skipped, the 64-bit key and the canonical mode are fq-kcount's. k and plain / canonical are the
 *            table's own: the handle carries them.
 *   Count.   c(w) is the table's count of the window's key, 0 when the key is absent; the key of 32 x 'T' in plain mode has
 *            the counter of its own that fq-kcount keeps for it. c(w) is saturated at SCFQ_NORM_MAX_DEPTH = 2^32 - 2 (2^32 - 1
 *            is the kernels' marker for "no k-mer here"). The lookup is scfq_kcount_query's: 16-byte loads, linear probing, at
 *            most the table's probe bound of slots, ending at the key or at an empty slot; every key that was inserted lies
 *            within that bound of its home slot, so the bound loses nothing.
 *   Per read (scfq_norm_rec, 16 bytes; paired input: mate m of pair p is entry 2p + m). kmers: the read's number of k-mers;
 *            depth: the LOWER MEDIAN of their counts, sorted[(kmers - 1) / 2], 0 when kmers = 0; min_count: the smallest
 *            count, 0 when kmers = 0; weak: the k-mers with c < weak_below (0: none are counted).
 *   Per unit, u its 0-based number in input order. D = the smaller depth among the mates with kmers > 0 ("use the lower
 *            depth"). A unit without such a mate is `no_kmers`: dropped, or kept with SCFQ_NORM_KEEP_NO_KMERS. Otherwise it is
 *            dropped as `low` iff D < min_depth. Otherwise, with target > 0 and D > target, it is dropped as `high` iff
 *            ((r * D) >> 32) >= target, r = mix64(seed ^ (u * 0x9E3779B97F4A7C15 mod 2^64)) >> 32 and mix64 MurmurHash3's
 *            64-bit finalizer (r and D are below 2^32: the product fits 64 bits). Otherwise it is kept. target = 0 switches
 *            the thinning off. The decision depends on u, the seed and the counts only — not on launch geometry, on
 *            SCFQ_NORM_LDS_WINDOWS or on host vs device input.
 *   Outputs. out1 / out2 receive the kept units' records in input order, echoed as fq-screen echoes them, pairs in step;
 *            interleaved input sends both mates to out1. The sizing call, a too-small output (SCFQ_EARG naming it, statistics
 *            complete, NO byte written to ANY output) and a too-small rec_cap (SCFQ_EARG with text before any write) are
 *            scfq_screen_buffers'. hist_host: NULL (bins = 0), or 2 * bins words of HOST memory, 2 <= bins <= 2^20:
 *            hist[2d] = units with D = d, hist[2d + 1] = those of them that are kept; the last bin gathers D >= bins - 1;
 *            no_kmers units are in neither column.
 *   Two-pass form. table = NULL: the library counts the SAME inputs first (opts->k, opts->table_flags, opts->table_bits; growth
 *            and SCFQ_EFULL are fq-kcount's), normalizes against that table and frees it; one staging and one line index per
 *            input serve both passes. With a table given opts->k is 0 or the table's k and table_flags / table_bits are not
 *            looked at.
 *   Limits.  One device, everything resident, fewer than 2^31 records per input, L < 2^32. The two-pass form needs fq-kcount's
 *            table next to the inputs: 32 bytes per input byte at automatic sizing (2 slots of 16 bytes per byte).
 *   Device pipeline. K5 line index per input; N1 — a wave per read, four per block, persistent blocks: the read through LDS
 *            as 2-bit codes and an invalid-bit plane in chunks of 512 window starts, lane l the windows l, l + 64, ..., each
 *            valid one probes the table, its saturated count (or the marker) goes to the wave's array of 2048 words in LDS,
 *            minimum, weak, kmers and the maximum are wave reductions, the median a radix select (a ballot and a population
 *            count per 64 entries and bit, from the maximum's top bit down); a read with more windows than the array keeps its
 *            counts in device memory (4 bytes per window of such reads, sized by a pass over the line index before N1) and
 *            selects from there; SCFQ_NORM_LDS_WINDOWS = 64 .. 2048 in the environment lowers the threshold and changes no
 *            result — N2, a thread per unit: the rule, output lengths per group of 32, statistics, histogram columns — one
 *            exclusive scan per output — N3, a wave per group echoes the kept records. Every loop is bounded: probes by the
 *            probe bound, select rounds by 32, chunk loops by the line's length. There is no CPU fallback. */
#define SCFQ_NORM_MAX_DEPTH      0xFFFFFFFEu
#define SCFQ_NORM_INTERLEAVED    0x1u
#define SCFQ_NORM_KEEP_NO_KMERS  0x2u
#define SCFQ_NORM_MAX_BINS       (1ull << 20)
typedef struct scfq_norm_opts {        /* 48 bytes */
  uint64_t struct_size;   /* sizeof(scfq_norm_opts) */
  uint32_t flags;         /* SCFQ_NORM_INTERLEAVED | SCFQ_NORM_KEEP_NO_KMERS */
  uint32_t k;             /* table = NULL: 13 .. 32; otherwise 0 or the table's k */
  uint32_t table_flags;   /* table = NULL: SCFQ_KCOUNT_CANONICAL or 0 */
  uint32_t table_bits;    /* table = NULL: scfq_kcount_opts.table_bits */
  uint32_t target;        /* 0: no thinning */
  uint32_t min_depth;
  uint32_t weak_below;    /* 0: count none */
  uint32_t reserved;      /* 0 */
  uint64_t seed;
} scfq_norm_opts;
typedef struct scfq_norm_rec { uint32_t kmers, depth, min_count, weak; } scfq_norm_rec;
typedef struct scfq_norm_stats {       /* 37 x 8 bytes */
  uint64_t struct_size;   /* caller sets to sizeof(scfq_norm_stats) before the call */
  uint64_t abi_version;   /* library writes SCFQ_ABI_VERSION */
  uint64_t reads1, reads2;             /* as scfq_screen_stats, down to `unpaired` */
  uint64_t lines1, lines2;
  uint64_t input_bytes1, input_bytes2;
  uint64_t pairs, unpaired;
  uint64_t units_in, units_out;        /* units_in = units_out + dropped_no_kmers + dropped_low + dropped_high */
  uint64_t reads_in, reads_out;        /* reads_in: reads1, or 2 * pairs */
  uint64_t dropped_no_kmers, dropped_low, dropped_high;   /* units */
  uint64_t short_reads;                /* L < k */
  uint64_t bases_in, bases_out;        /* sums of L */
  uint64_t windows, kmers, skipped;    /* windows = kmers + skipped */
  uint64_t weak_kmers;                 /* c < weak_below */
  uint64_t absent_kmers;               /* c = 0: only a table made from other data has any */
  uint64_t out1_bytes, out2_bytes;     /* sizes of the outputs, written or not */
  uint64_t flags, k, table_flags, target, min_depth, weak_below, seed;   /* the parameters as used */
  uint64_t distinct, slots, passes;    /* the table's */
} scfq_norm_stats;

/* r1 / r2, the outputs and the device-pointer rules are those of scfq_screen_buffers. opts = NULL: the defaults (no flags,
 * target 0, min_depth 0, weak_below 2, seed 0), which need a table. recs_device: NULL, or DEVICE memory for rec_cap entries.
 * SCFQ_EARG with text in scfq_norm_error_detail(), decided before any HIP call: unknown flag bits, a non-zero reserved, a wrong
 * struct_size (opts' or stats'), bins outside 2 .. 2^20 with a histogram (or not 0 without one), out2 without a second input
 * or with interleaved input, a second input without a first or with interleaved input, a k that is not the table's, and with
 * table = NULL whatever scfq_kcount_buffers refuses in k, table_flags and table_bits. */
int scfq_norm_buffers(const scfq_kcount* table, const void* r1, uint64_t n1, const void* r2, uint64_t n2, int is_device,
                      const scfq_norm_opts* opts, scfq_norm_rec* recs_device, uint64_t rec_cap, void* out1, uint64_t cap1,
                      void* out2, uint64_t cap2, int out_is_device, uint64_t* hist_host, uint64_t bins, scfq_norm_stats* stats);
/* As scfq_screen_files: staged inputs, descriptors below 0 are not produced, out1 then out2, SCFQ_EPIPE / SCFQ_EIO.
 * recs_host: NULL, or HOST memory for rec_cap entries of the per-read table. */
int scfq_norm_files(const scfq_kcount* table, const char* path1, const char* path2, const scfq_opts* opts,
                    const scfq_norm_opts* nopts, int out1_fd, int out2_fd, scfq_norm_rec* recs_host, uint64_t rec_cap,
                    uint64_t* hist_host, uint64_t bins, scfq_norm_stats* stats);
/* The one-row report without trailing newline; header != 0: the names of its columns instead. The columns: units_in units_out
 * reads_in reads_out dropped_no_kmers dropped_low dropped_high bases_in bases_out kmers skipped weak_kmers absent_kmers k target
 * min_depth. Returns the number of bytes needed (excluding NUL); writes at most cap bytes incl. NUL. */
int scfq_format_norm_row_tsv(const scfq_norm_stats* s, int header, char* buf, uint64_t cap);
/* "<depth>\t<units_in>\t<units_out>" of one bin, without trailing newline; the same return rule. */
int scfq_format_norm_hist_tsv(uint64_t depth, uint64_t units_in, uint64_t units_out, char* buf, uint64_t cap);
const char* scfq_norm_error_detail(void);        /* static, thread-local */

/* ---- `sc fq-complexity` (addition; not in the reference): symmetric DUST masking and filtering of low-complexity reads ----
 * Inputs, lines, records, texts, pairing (`pairs`, `unpaired`), interleaving and too_long are fq-trim's, word for word. A read
 * whose sequence text S has L > SCFQ_CPLX_MAX_LEN bytes is too long: nothing looks at it, it is never masked, never low, and
 * its record is echoed as fq-trim echoes one.
 * Triplets. Position i in [0, L-2) is VALID iff S[i], S[i+1], S[i+2] are each exactly 'A', 'C', 'G' or 'T' (byte-exact: lower
 *  case and 'N' are no bases, as in fq-kmers); t(i) is its 6-bit code.
 * Intervals. [i, j] with 0 <= i < j <= L-3 and l = j-i+1 <= window - 2; window is in bases, 8 .. 64, default 64 (sdust's W,
 *  so l <= 62). c(i,j) is the number of pairs a < b in [i, j], both valid, with t(a) == t(b). The score of the interval is
 *  the fraction c / (l-1); fractions are only ever compared by cross-multiplication (c <= 1891, l-1 <= 61).
 * High. 10 * c > threshold * (l-1); threshold is 1 .. 310, default 20 (sdust's T). At 310 nothing is high; equality is not.
 * Perfect. The interval is high and no sub-interval [i', j'], i <= i' < j' <= j, has a strictly larger score:
 *  c(i',j') * (l-1) <= c(i,j) * (l'-1) for all of them (the symmetric DUST of Morgulis et al. 2006). Agreement with
 *  dustmasker or sdust is not claimed: they restart the window at an 'N', here an invalid triplet simply matches nothing.
 * Masked positions. The union of [i, j+2] over all perfect intervals.
 * Per read. masked: the number of masked positions; intervals: the number of perfect intervals; first: the smallest masked
 *  position, 0xFFFF without one; score: floor(10 * c / (l-1)) of the interval with the largest fraction over ALL intervals,
 *  high or not, 0 for L < 4.
 * Low read. L >= 1 and 100 * masked > max_masked_pct * L; max_masked_pct is 0 .. 100, default 100 (nothing is low). A low
 *  single-end read is dropped; a pair is dropped when either mate is low.
 * Output record of a kept read that is not too long, always four lines: header text, '\n', S', '\n', separator text, '\n',
 *  the WHOLE quality text unchanged, '\n'. S' by `mask`: SCFQ_CPLX_MASK_NONE: S; SCFQ_CPLX_MASK_LOWER (the default): a masked
 *  byte in 'A' .. 'Z' gets | 0x20, any other byte stays; SCFQ_CPLX_MASK_N: every masked byte becomes 'N'.
 * All values are integers and exact. Device pipeline: line index (K5), D1 — a wave per read: the triplet codes and, per
 *  position, a 64-bit word "equal to the triplet d in front" in LDS; lane i of a round owns start 64 w + i and walks its
 *  interval one triplet at a time, best(i, j) = max(c / (l-1), best(i, j-1), best(i+1, j)) with the neighbour lane's value of
 *  the step before; 8 bytes and 8 mask words per read —, D2 — a thread per read or pair: low or not, output lengths per group
 *  of 32, the statistics and the score histogram —, one exclusive scan per output, D3 — a wave per group writes the records. */
#define SCFQ_CPLX_MAX_LEN       SCFQ_INSERT_MAX_LEN
#define SCFQ_CPLX_INTERLEAVED   0x1u
#define SCFQ_CPLX_MASK_NONE     0u
#define SCFQ_CPLX_MASK_LOWER    1u
#define SCFQ_CPLX_MASK_N        2u
#define SCFQ_CPLX_SCORE_BINS    312   /* reads_in by score 0 .. 310; the last bin: too long */
typedef struct scfq_cplx_opts {
  uint64_t struct_size;   /* sizeof(scfq_cplx_opts) */
  uint32_t flags;         /* SCFQ_CPLX_INTERLEAVED */
  uint32_t window;        /* 8 .. 64 */
  uint32_t threshold;     /* 1 .. 310 */
  uint32_t mask;          /* SCFQ_CPLX_MASK_* */
  uint32_t max_masked_pct;   /* 0 .. 100 */
  uint32_t reserved[3];   /* 0 */
} scfq_cplx_opts;
typedef struct scfq_cplx_rec {     /* the per-read table: 8 bytes per read; paired input: mate m of pair p is entry 2p + m */
  uint16_t score, masked, first, intervals;   /* a too-long read: {0xFFFF, 0, 0xFFFF, 0} */
} scfq_cplx_rec;
typedef struct scfq_cplx_stats {   /* 29 x 8 bytes */
  uint64_t struct_size;   /* caller sets to sizeof(scfq_cplx_stats) before the call */
  uint64_t abi_version;   /* library writes SCFQ_ABI_VERSION */
  uint64_t reads1, reads2;             /* as scfq_trim_stats, down to `unpaired` */
  uint64_t lines1, lines2;
  uint64_t input_bytes1, input_bytes2;
  uint64_t pairs, unpaired;
  uint64_t reads_in, reads_out;        /* reads_in: reads1, or 2 * pairs; reads_in = reads_out + dropped_reads */
  uint64_t too_long;
  uint64_t low_reads;                  /* reads that are low themselves */
  uint64_t dropped_reads;              /* paired input: both reads of a pair with a low mate */
  uint64_t masked_reads;               /* reads with masked > 0 */
  uint64_t perfect_intervals;          /* sum of `intervals` */
  uint64_t bases_in, bases_out;        /* sums of L over reads_in and reads_out */
  uint64_t masked_bases;               /* sum of `masked` over reads_in */
  uint64_t masked_bases_out;           /* the same over reads_out */
  uint64_t max_score;                  /* over the reads that are not too long */
  uint64_t out1_bytes, out2_bytes;     /* sizes of the outputs, written or not */
  uint64_t flags, window, threshold, mask, max_masked_pct;   /* the parameters as used */
} scfq_cplx_stats;

/* r1 / r2, the outputs, the sizing call, a too-small output (SCFQ_EARG naming it, stats complete, NO byte written to ANY
 * output: D3 compares the scanned totals with the capacities before it stores) and the device-pointer rules are those of
 * scfq_trim_buffers. recs: NULL, or memory of the outputs' kind (host with out_is_device = 0, device otherwise) for
 * recs_cap entries of the per-read table; fewer than reads_in is SCFQ_EARG with text: stats is complete and nothing is
 * written to the table or to an output. hist_host: NULL, or HOST memory for SCFQ_CPLX_SCORE_BINS words. SCFQ_EARG with
 * text in scfq_cplx_error_detail(), before any launch: unknown flag bits, window, threshold, mask or max_masked_pct out of
 * range, reserved not 0, out2 without a second input, a second buffer with SCFQ_CPLX_INTERLEAVED; without text: a NULL stats
 * or a wrong struct_size (stats' or opts'), a NULL pointer with a size or capacity. opts = NULL: the defaults. There is no
 * CPU fallback (SCFQ_EHIP without a device). */
int scfq_cplx_buffers(const void* r1, uint64_t n1, const void* r2, uint64_t n2, int is_device, const scfq_cplx_opts* opts,
                      scfq_cplx_rec* recs, uint64_t recs_cap, uint64_t* hist_host, void* out1, uint64_t cap1, void* out2,
                      uint64_t cap2, int out_is_device, scfq_cplx_stats* stats);
/* As scfq_trim_files: staged inputs, descriptors below 0 are not produced, out1 then out2, SCFQ_EPIPE / SCFQ_EIO.
 * per_read_fd >= 0: the per-read table as rows of scfq_format_cplx_rec_tsv, each with a '\n', written before the outputs. */
int scfq_cplx_files(const char* path1, const char* path2, const scfq_opts* opts, const scfq_cplx_opts* copts, int out1_fd,
                    int out2_fd, int per_read_fd, uint64_t* hist_host, scfq_cplx_stats* stats);
/* The one-row report without trailing newline; header != 0: the names of its columns instead. The columns: reads_in reads_out
 * dropped_reads low_reads too_long pairs unpaired masked_reads perfect_intervals bases_in bases_out masked_bases
 * masked_bases_out max_score out1_bytes out2_bytes. Returns the number of bytes needed (excluding NUL); writes at most cap
 * bytes incl. NUL. */
int scfq_format_cplx_stats_tsv(const scfq_cplx_stats* s, int header, char* buf, uint64_t cap);
/* "<read>\t<length>\t<score>\t<masked>\t<first>\t<intervals>" without trailing newline; r = NULL: the names of the columns.
 * score is "-" for a too-long read, first is "-" without a masked position. The same return rule. */
int scfq_format_cplx_rec_tsv(uint64_t read, const scfq_cplx_rec* r, uint64_t length, char* buf, uint64_t cap);
const char* scfq_cplx_error_detail(void);        /* static, thread-local */

/* ---- `sc fq-rmdup` (addition; not in the reference): duplicate reads and pairs removed by SEQUENCE --------------------
 * (scfq_dedup_* above is the reference's fq-dedup: it drops records whose HEADER repeats. This one finds two reads of the
 * same molecule, which carry different names.)
 * Inputs, lines, records, texts, pairing (`pairs`, `unpaired`) and interleaving are fq-trim's, word for word. A UNIT is a
 * read (single-end input) or a pair; units_in is reads1, or pairs.
 * No length limit. There is no too_long: a sequence text of any length is hashed and compared, in loops over its words.
 * Key of a read with sequence text S of L bytes: the bytes S[0, min(L, prefix)) together with that length. prefix is 0 (the
 *  whole text, the default) or 1 .. 65535. The comparison is byte-exact: 'N', lower case and anything else are bytes like any
 *  other, so two reads that fq-complexity soft-masked alike stay equal. An empty text is a key like any other.
 * Equality of units. Single-end: equal keys. Paired: key1 = key1' and key2 = key2'; with SCFQ_RMDUP_SWAPPED also
 *  (key1 = key2' and key2 = key1'): the same fragment read from the other strand. Both relations are equivalences (the
 *  second compares unordered pairs of keys). The flag with single-end input is SCFQ_EARG with text.
 * Classes. The REPRESENTATIVE of a class is its unit with the smallest index in input order; every other member is a
 *  DUPLICATE and is not written. The kept units are echoed in input order exactly as fq-screen echoes a kept unit: each line
 *  the record has, as text plus '\n'. Two inputs give out1 / out2, interleaved input one output (mate 1, then mate 2). Units
 *  counted in `unpaired` go nowhere.
 * Per-unit table: scfq_rmdup_rec, 8 bytes per unit. rep: the index of the representative (the unit's own index when it is
 *  kept); copies: the class size for a representative, 0 for a duplicate.
 * Histogram: SCFQ_RMDUP_HIST_BINS words. Bin c, 1 <= c <= 1023: the classes of size c; bin 1024: the classes of size >= 1024;
 *  bin 0 is 0. The bins add up to units_out.
 * collisions and rounds are the only two values that depend on the hash: collisions is the number of (unit, round)
 *  comparisons that found a unit different from the head of its equal-hash run, rounds the number of compare rounds that had
 *  a candidate. No other field and no output byte depends on the hash or on hash_bits.
 * All values are integers and exact. Device pipeline: line index (K5); U1 — eight lanes per unit hash its keys in 8-byte
 *  words; a radix sort of (hash, unit); per round U2 — run starts, the head of every run by a max-scan, the candidates
 *  compacted — and U3 — eight lanes per candidate compare it with the HEAD of its run, the unequal ones form the next
 *  round's list in sorted order —; the class sizes; U4 — a thread per unit: the table, output lengths per group of 32, the
 *  statistics and the histogram —, one exclusive scan per output, U5 — a wave per group echoes the kept records. */
#define SCFQ_RMDUP_INTERLEAVED  0x1u
#define SCFQ_RMDUP_SWAPPED      0x2u
#define SCFQ_RMDUP_HIST_BINS    1025
#define SCFQ_RMDUP_MAX_PREFIX   65535
typedef struct scfq_rmdup_opts {
  uint64_t struct_size;   /* sizeof(scfq_rmdup_opts) */
  uint32_t flags;         /* SCFQ_RMDUP_INTERLEAVED | SCFQ_RMDUP_SWAPPED */
  uint32_t prefix;        /* 0: the whole text; 1 .. SCFQ_RMDUP_MAX_PREFIX */
  uint32_t hash_bits;     /* 0: the library's default (40); 1 .. 64: the bits of the hash that are sorted. Fewer bits make
                             equal-hash runs of different units (the tests force collisions with it); no result but
                             `collisions` and `rounds` depends on it */
  uint32_t reserved[3];   /* 0 */
} scfq_rmdup_opts;
typedef struct scfq_rmdup_rec {    /* the per-unit table: 8 bytes per unit */
  uint32_t rep;           /* the unit's representative */
  uint32_t copies;        /* a representative: the size of its class; a duplicate: 0 */
} scfq_rmdup_rec;
typedef struct scfq_rmdup_stats {  /* 26 x 8 bytes */
  uint64_t struct_size;   /* caller sets to sizeof(scfq_rmdup_stats) before the call */
  uint64_t abi_version;   /* library writes SCFQ_ABI_VERSION */
  uint64_t reads1, reads2;             /* as scfq_trim_stats, down to `unpaired` */
  uint64_t lines1, lines2;
  uint64_t input_bytes1, input_bytes2;
  uint64_t pairs, unpaired;
  uint64_t units_in, units_out;        /* units_in: reads1, or pairs; units_out: the classes */
  uint64_t reads_in, reads_out;        /* reads1, or 2 * pairs; the reads of the kept units */
  uint64_t duplicate_units;            /* units_in - units_out */
  uint64_t duplicated_classes;         /* classes with copies >= 2 */
  uint64_t max_copies;                 /* the largest class; 0 without units */
  uint64_t bases_in, bases_out;        /* sums of L over reads_in and reads_out */
  uint64_t collisions, rounds;         /* the two that depend on the hash (above) */
  uint64_t out1_bytes, out2_bytes;     /* sizes of the outputs, written or not */
  uint64_t flags, prefix, hash_bits;   /* the parameters as used (hash_bits: 40 for 0) */
} scfq_rmdup_stats;

/* r1 / r2, the outputs, the sizing call, a too-small output (SCFQ_EARG naming it, stats complete, NO byte written to ANY
 * output: U5 compares the scanned totals with the capacities before it stores) and the device-pointer rules are those of
 * scfq_trim_buffers. recs: NULL, or memory of the outputs' kind (host with out_is_device = 0, device otherwise) for
 * recs_cap entries of the per-unit table; fewer than units_in is SCFQ_EARG with text: stats is complete and nothing is
 * written to the table or to an output. hist_host: NULL, or HOST memory for SCFQ_RMDUP_HIST_BINS words. SCFQ_EARG with
 * text in scfq_rmdup_error_detail(), before any HIP call: unknown flag bits, prefix or hash_bits out of range, reserved not
 * 0, SCFQ_RMDUP_SWAPPED with single-end input, out2 without a second input, a second buffer with SCFQ_RMDUP_INTERLEAVED;
 * without text: a NULL stats or a wrong struct_size (stats' or opts'), a NULL pointer with a size or capacity. opts = NULL:
 * the defaults. Fewer than 2^31 records per input. There is no CPU fallback (SCFQ_EHIP without a device). */
int scfq_rmdup_buffers(const void* r1, uint64_t n1, const void* r2, uint64_t n2, int is_device, const scfq_rmdup_opts* opts,
                       scfq_rmdup_rec* recs, uint64_t recs_cap, uint64_t* hist_host, void* out1, uint64_t cap1, void* out2,
                       uint64_t cap2, int out_is_device, scfq_rmdup_stats* stats);
/* As scfq_trim_files: staged inputs, descriptors below 0 are not produced, out1 then out2, SCFQ_EPIPE / SCFQ_EIO.
 * per_read_fd >= 0: the per-unit table as rows of scfq_format_rmdup_rec_tsv, each with a '\n', written before the outputs. */
int scfq_rmdup_files(const char* path1, const char* path2, const scfq_rmdup_opts* opts, const scfq_opts* ropts, int out1_fd,
                     int out2_fd, int per_read_fd, uint64_t* hist_host, scfq_rmdup_stats* stats);
/* The one-row report without trailing newline; header != 0: the names of its columns instead. The columns: units_in units_out
 * duplicate_units duplicate_pct duplicated_classes max_copies reads_in reads_out pairs unpaired bases_in bases_out out1_bytes
 * out2_bytes. duplicate_pct is floor(10000 * duplicate_units / units_in) printed as X.YY ("0.00" for no units), in integers
 * only. Returns the number of bytes needed (excluding NUL); writes at most cap bytes incl. NUL. */
int scfq_format_rmdup_stats_tsv(const scfq_rmdup_stats* s, int header, char* buf, uint64_t cap);
/* "<unit>\t<rep>\t<copies>" without trailing newline; rec = NULL: the names of the columns. The same return rule. */
int scfq_format_rmdup_rec_tsv(uint64_t unit, const scfq_rmdup_rec* rec, char* buf, uint64_t cap);
const char* scfq_rmdup_error_detail(void);       /* static, thread-local */

/* ---- `sc fq-repair` (addition; not in the reference): R1 and R2 re-paired by READ NAME ---------------------------------
 * Every paired command above pairs record i of R1 with record i of R2 and looks at no name. This one joins the records of
 * two FASTQs by name: the mates that find each other leave in step, the others as singles.
 * Inputs, lines, records, texts and the echo of a record are fq-trim's and fq-screen's, word for word: a record is four lines,
 * reads = (lines + 3) / 4, a text has no "\r\n" or '\n' end, a record is echoed as each line it has, as text plus '\n'.
 * Exactly two inputs; reads1 < 2^31 and reads2 < 2^31 (so reads1 + reads2 < 2^32 - 1); beyond that SCFQ_EARG with text.
 * Name of a record, from the text H of its header line, in this order: (1) H's first byte is dropped, whatever it is (an
 *  empty H gives the empty name); (2) what is left is cut at its first space (0x20) or tab (0x09), exclusive; (3) if what is
 *  left has at least two bytes and ends in "/1" or "/2", those two bytes are dropped — once, and in either input. The
 *  comparison is byte-exact, there is no length limit, and the empty name is a name like any other.
 * Matching. The r-th record in input order that carries a name in R1 is the mate of the r-th record that carries that name
 *  in R2; records of a name beyond the other input's count are singles. Without repeated names this is the plain join; with
 *  them it is deterministic, and an input that is in step maps onto itself.
 * Outputs. out1: the matched R1 records in R1's order, echoed. out2: their mates in that same order (a gather from R2).
 *  singles1 / singles2: the unmatched records of each input in that input's order. Any subset may be left out.
 * Per-record table: reads1 + reads2 words of uint32_t. Entry i < reads1 is the R2 index of R1 record i's mate; entry
 *  reads1 + j is the R1 index of R2 record j's mate; SCFQ_REPAIR_SINGLE for a single.
 * No field other than collisions, rounds and path, and no output byte, depends on the hash, on hash_bits or on the fast path
 * (reads1 == reads2: name i of R1 is compared with name i of R2 first, and when none differs the table is the identity and
 * no join runs; SCFQ_REPAIR_FAST=0 in the environment, read per call, turns that off). All values are integers and exact.
 * Device pipeline: DESIGN.md §fq-repair. */
#define SCFQ_REPAIR_SINGLE 0xFFFFFFFFu
typedef struct scfq_repair_opts {
  uint64_t struct_size;   /* sizeof(scfq_repair_opts) */
  uint32_t flags;         /* every bit is reserved: an unknown bit is SCFQ_EARG */
  uint32_t hash_bits;     /* 0: the library's default (40); 1 .. 64: the bits of the name hash that are sorted */
  uint32_t reserved[4];   /* 0 */
} scfq_repair_opts;
typedef struct scfq_repair_stats {  /* 24 x 8 bytes */
  uint64_t struct_size;   /* caller sets to sizeof(scfq_repair_stats) before the call */
  uint64_t abi_version;   /* library writes SCFQ_ABI_VERSION */
  uint64_t reads1, reads2;
  uint64_t lines1, lines2;
  uint64_t input_bytes1, input_bytes2;
  uint64_t pairs;                      /* matched pairs; not min(reads1, reads2) */
  uint64_t singles1, singles2;         /* unmatched records of each input */
  uint64_t moved;                      /* pairs (i, j) with i != j */
  uint64_t in_step;                    /* 1 iff reads1 == reads2, singles1 == singles2 == 0 and moved == 0 */
  uint64_t repeated1, repeated2;       /* records whose name occurred earlier in their own input */
  uint64_t collisions, rounds;         /* as fq-rmdup's: they depend on the hash only */
  uint64_t path;                       /* 0: the positional check answered; 1: the full join ran */
  uint64_t out1_bytes, out2_bytes, singles1_bytes, singles2_bytes;   /* sizes of the outputs, written or not */
  uint64_t flags, hash_bits;           /* the parameters as used (hash_bits: 40 for 0) */
} scfq_repair_stats;

/* r1 / r2: host (is_device = 0) or device memory, both needed (a NULL pointer goes with a size of 0: an empty input). The four
 * outputs (NULL: not wanted), the sizing call (no output: the four *_bytes say what to bring), a too-small output (SCFQ_EARG
 * naming it, stats complete, NO byte written to ANY output: both writers compare the scanned totals with the capacities
 * before they store) and the device-pointer rules are those of scfq_trim_buffers. table: NULL, or memory of the outputs' kind
 * for table_cap words; fewer than reads1 + reads2 is SCFQ_EARG with text: stats is complete and nothing is written to the
 * table or to an output. SCFQ_EARG with text in scfq_repair_error_detail(), before any HIP call: flag bits, hash_bits above
 * 64, reserved not 0; without text: a NULL stats or a wrong struct_size (stats' or opts'), a NULL pointer with a size or
 * capacity. opts = NULL: the defaults. There is no CPU fallback (SCFQ_EHIP without a device). */
int scfq_repair_buffers(const void* r1, uint64_t n1, const void* r2, uint64_t n2, int is_device, const scfq_repair_opts* opts,
                        uint32_t* table, uint64_t table_cap, void* out1, uint64_t cap1, void* out2, uint64_t cap2, void* singles1,
                        uint64_t cap_s1, void* singles2, uint64_t cap_s2, int out_is_device, scfq_repair_stats* stats);
/* As scfq_merge_files: staged inputs (".gz" / BGZF by suffix), descriptors below 0 are not produced, out1, out2, singles1,
 * singles2 in that order, SCFQ_EPIPE / SCFQ_EIO. per_read_fd >= 0: the table as rows of scfq_format_repair_rec_tsv, each with
 * a '\n', R1's records and then R2's, written before the outputs. Both paths are needed (SCFQ_EARG). */
int scfq_repair_files(const char* path1, const char* path2, const scfq_repair_opts* opts, const scfq_opts* ropts, int out1_fd,
                      int out2_fd, int singles1_fd, int singles2_fd, int per_read_fd, scfq_repair_stats* stats);
/* The one-row report without trailing newline; header != 0: the names of its columns instead. The columns: reads1 reads2 pairs
 * singles1 singles2 moved in_step repeated1 repeated2 out1_bytes out2_bytes singles1_bytes singles2_bytes. Returns the number
 * of bytes needed (excluding NUL); writes at most cap bytes incl. NUL. */
int scfq_format_repair_stats_tsv(const scfq_repair_stats* s, int header, char* buf, uint64_t cap);
/* "<input>\t<record>\t<mate>" without trailing newline: input 1 or 2, the record's index in it, its mate's index in the other
 * input or "-" for a single; input = 0: the names of the columns. The same return rule. */
int scfq_format_repair_rec_tsv(uint32_t input, uint64_t record, uint32_t mate, char* buf, uint64_t cap);
const char* scfq_repair_error_detail(void);      /* static, thread-local */

/* ---- `sc fa-gc` (FASTA group): src/fa_gc.nim, docs/fa-gc.md, sc.nim:84-96 --------------------------------------------
 * GC content of the windows [pos - w, pos + w] around 1-based positions of a FASTA. The contract:
 *   Lines.   A header line is a line whose first byte is '>' (a line that starts at byte 0 of the input included); every
 *            other line is a sequence line.
 *   Bases.   A base is a byte 0x21 .. 0x7E on a sequence line: htslib's faidx rule (isgraph), so '\r', blanks and tabs are
 *            not bases and a CRLF file has the coordinates of its LF form.
 *   Contigs. A contig starts at a header line; its name is the header text after '>' up to the first byte <= 0x20; its
 *            bases are those of the sequence lines up to the next header line, numbered from 0. A name has at most 255
 *            bytes (a longer one: SCFQ_EARG, text in scfq_fa_error_detail()). Of two contigs with one name the first is
 *            found by name, both stay in the table. Bases before the first header line belong to no contig
 *            (orphan_bases). Line lengths need not be uniform: for every file faidx accepts the coordinates are faidx's.
 *            No .fai file is read or written.
 *   Classes. gc = base in {G, C, g, c}; acgt = base in {A, C, G, T, a, c, g, t} (calc_gc, fa_gc.nim:26-27); everything
 *            else ('N', IUPAC codes, a '>' that does not start a line) is a base in neither class.
 * Where the reference reloads a chromosome and re-counts 2w + 1 bases per (position, window) pair, the index holds prefix
 * tables per 4 KiB tile of the input, built in one pass, and an interval costs two tile reads whatever its length. All
 * values are integers and exact. Limits: one device, the whole (inflated) input resident in its memory, names of at most
 * 255 bytes; there is no CPU fallback (SCFQ_EHIP without a device), as scfq_kmers_buffer. */
typedef struct scfq_fa_index scfq_fa_index;   /* opaque: tile tables on the device, contig table on the host */
typedef struct scfq_fa_summary {
  uint64_t struct_size;   /* caller sets to sizeof(scfq_fa_summary) before the call */
  uint64_t abi_version;   /* library writes SCFQ_ABI_VERSION */
  uint64_t input_bytes;   /* bytes scanned (inflated bytes for .gz) */
  uint64_t tiles;
  uint64_t contigs;
  uint64_t bases;         /* of all sequence lines, orphan_bases included */
  uint64_t gc_bases;
  uint64_t acgt_bases;
  uint64_t orphan_bases;  /* bases before the first header line */
} scfq_fa_summary;
typedef struct scfq_fa_contig {
  const char* name;       /* NUL-terminated, owned by the index */
  uint64_t name_len;
  uint64_t header_offset; /* byte offset of the '>' */
  uint64_t length;        /* bases */
} scfq_fa_contig;
typedef struct scfq_fa_interval { uint64_t contig, begin, end; } scfq_fa_interval;   /* 0-based, half-open, end <= length */
typedef struct scfq_fa_counts { uint64_t gc, acgt, bases; } scfq_fa_counts;

/* Builds the index of a FASTA in host (is_device = 0) or device memory. A host buffer is staged and the staged copy is
 * owned by the index; a DEVICE buffer stays the caller's, is read again by every scfq_fa_count_intervals and must outlive
 * the index (device pointers follow the scfq_set_wait_stream contract of scfq_index_lines; any alignment). sum may be
 * NULL. SCFQ_EARG for a NULL out, a wrong sum->struct_size or a NULL ptr with n > 0; *out is NULL after every failure. */
int scfq_fa_index_buffer(const void* ptr, uint64_t n, int is_device, scfq_fa_index** out, scfq_fa_summary* sum);
/* Stages the whole (inflated) input with scfq_stage_file, ".gz" and BGZF by suffix as everywhere else; the index owns it. */
int scfq_fa_index_file(const char* path, const scfq_opts* opts, scfq_fa_index** out, scfq_fa_summary* sum);
/* Contig i in file order; SCFQ_EARG for i >= contigs. */
int scfq_fa_contig_at(const scfq_fa_index* index, uint64_t i, scfq_fa_contig* out);
/* The first contig named `name` (NUL-terminated); SCFQ_EARG when absent. */
int scfq_fa_contig_find(const scfq_fa_index* index, const char* name, uint64_t* i_out);
/* out[i] = (gc, acgt, bases) of the bases [begin, end) of contig q[i].contig; q and out are HOST arrays of nq entries, and
 * all of them go to the device in one call. An interval with begin > end, end > length or contig >= contigs: SCFQ_EARG,
 * the index of the first such interval in scfq_fa_error_detail(), and nothing is written. nq = 0 is valid. One call at a
 * time per index (the index works on one stream of its own); two indexes are independent. */
int scfq_fa_count_intervals(scfq_fa_index* index, const scfq_fa_interval* q, uint64_t nq, scfq_fa_counts* out);
void scfq_fa_index_free(scfq_fa_index* index);   /* NULL is fine */
const char* scfq_fa_error_detail(void);          /* static, thread-local */

/* Host-only helpers of the command (no device is touched).
 * scfq_fa_parse_window restates sci_parse_int (helpers.nim:230-237) literally: without an 'e' the commas are removed and
 * the rest is a decimal integer ("3,200" is 3200); with an 'e' the value is pow(coeff * 10.0, exponent) truncated, so
 * "1e3" is 1000 and "5e5" is 312500000 (50^5, not 500000), as in the reference. SCFQ_EARG for text that is neither and
 * for a window < 1 ("Window lengths must be >= 1", fa_gc.nim:70-71), the text in scfq_fa_error_detail(). */
int scfq_fa_parse_window(const char* text, uint64_t* window_out);
/* The bases a window covers (sub_seq, fa_gc.nim:29-37) for a 1-based pos: pos0 = pos - 1; *out_of_range iff pos < 1 or
 * pos0 >= length (then begin = end = 0); begin = max(0, pos0 - w), end = min(length, pos0 + w + 1). */
int scfq_fa_gc_interval(int64_t pos, uint64_t window, uint64_t length, uint64_t* begin, uint64_t* end, int* out_of_range);
/* The cell text: x = gc / acgt as an IEEE double, round(x * 10^d) / 10^d with C round() and d = the number of decimal
 * digits of `window` + 2 (fa_gc.nim:54), printed as the shortest text that reads back as the same double, laid out the way
 * Python's repr(float) does: "0.5", "1.0", "0.0", "5e-05"; "nan" for acgt = 0. Returns the number of bytes needed
 * (excluding NUL); writes at most cap bytes incl. NUL. */
int scfq_format_fa_gc_value(uint64_t gc, uint64_t acgt, uint64_t window, char* buf, uint64_t cap);

/* Whole (inflated) input of `path` into a device buffer the caller frees with scfq_device_free(). */
int scfq_stage_file(const char* path, const scfq_opts* opts, void** device_ptr_out, uint64_t* n_out);
int scfq_device_free(void* device_ptr);

/* ---- `sc fq-meta` (next row of SURVEY.md §8f): src/fq_meta.nim:197-278 -------------------------
 * One 16-column TSV row (scfq_meta_header() names them, fq_meta.nim:11-26) from the first sample_n records of a FASTQ:
 * machine / flowcell / run / lane parsed from the first header, sequencer guess from the instrument and flow-cell tables,
 * most frequent index, quality range and format guess. Host-side string work over a few hundred lines, as in the
 * reference. SCFQ_META_WHOLE_FILE (addition): min_qual / max_qual and the format columns use the quality-line histogram
 * of the whole file (K3 on the device) instead of the sampled records. Returns the row length (bytes needed excluding NUL)
 * or a negative code; SCFQ_EARG also when the first header has too few ':' fields (IndexError in the reference). */
#define SCFQ_META_WHOLE_FILE 0x1u
const char* scfq_meta_header(void);
int scfq_meta_file_tsv(const char* path, uint32_t sample_n, uint32_t flags, char* out, uint64_t cap);

/* ---- formatting: src/fq_count.nim:47-51 ---------------------------------------------------
 * "<reads>\t<gc_content>\t<gc_bases>\t<n_bases>\t<bases>" without trailing newline;
 * gc_content = gc/(bases-n) as IEEE double printed the way Nim 1.0.6 `$float` does: C "%.16g",
 * then ".0" appended when the text has no '.', no letter; NaN prints "nan".
 * Returns the number of bytes needed (excluding NUL); writes at most cap bytes incl. NUL. */
int scfq_format_tsv(const scfq_counts* c, char* buf, uint64_t cap);

const char* scfq_strerror(int rc);   /* static storage */
const char* scfq_last_error_detail(void); /* static, thread-local: e.g. the failing HIP call */
int  scfq_last_timing(scfq_timing* t);
/* Device memory the library's ingest paths hold in this process (staging, inflate buffers, symbol pools): now, and the most
 * they ever held. The buffers are kept between calls and given back by scfq_shutdown(). */
uint64_t scfq_device_bytes_now(void);
uint64_t scfq_device_bytes_high_water(void);
int  scfq_device_count(void);        /* number of visible HIP devices, or negative on error */
/* Default caller stream of THIS host thread for the entry points that take device pointers but no scfq_opts
 * (scfq_index_lines, scfq_dedup_buffer) and for calls without SCFQ_WAIT_STREAM: same contract as scfq_opts.wait_stream.
 * enable = 0 (the initial state): the caller synchronises before calling. hip_stream = NULL with enable != 0 names the
 * legacy default stream. scfq_get_wait_stream returns the stream, *enabled (may be NULL) whether one is set. */
int   scfq_set_wait_stream(void* hip_stream, int enable);
void* scfq_get_wait_stream(int* enabled);
int  scfq_shutdown(void);            /* frees streams, pinned and device scratch; safe to call twice */

/* Diagnostic entry points (scfq_debug_*: a second device implementation for the parity tests, host-only readers, the
 * stream-ceiling probe) are declared in sc_fqcount_debug.h; a reference-side binding needs none of them. */

/* ---- synthetic workloads of SURVEY.md §8(d) / BASELINE.json configs ------------------------
 * Counter-based generator: record i of a workload is a pure function of (seed, i), so host and
 * device produce identical bytes and any shard can be produced independently.
 * kind: 0 = Illumina 150 bp (config 2/3), 1 = Nanopore-style 500 bp..50 kb (config 5). */
#define SCFQ_SYNTH_ILLUMINA 0
#define SCFQ_SYNTH_NANOPORE 1
typedef struct scfq_synth_info {
  uint64_t struct_size;
  uint64_t records;      /* records generated */
  uint64_t bytes;        /* exact byte length of those records */
  uint64_t gc_bases, n_bases, bases;  /* tallied by the generator itself, independent of the scan */
} scfq_synth_info;

/* Smallest record count whose total length is >= min_bytes (and its exact length). */
int scfq_synth_plan(int kind, uint64_t seed, uint64_t first_record, uint64_t min_bytes, scfq_synth_info* info);
/* Locate byte `offset` of the record stream that starts at record 0: writes the index of the record
 * containing that byte and the stream offset at which that record starts. */
int scfq_synth_locate(int kind, uint64_t seed, uint64_t offset, uint64_t* record, uint64_t* record_start);
/* Generate records [first_record, first_record+records) into host memory (cap >= info->bytes). */
int scfq_synth_host(int kind, uint64_t seed, uint64_t first_record, uint64_t records,
                    void* dst, uint64_t cap, scfq_synth_info* info);
/* Same bytes, produced by a HIP kernel directly in HBM (dst is a device pointer). */
int scfq_synth_device(int kind, uint64_t seed, uint64_t first_record, uint64_t records,
                      void* dst_device, uint64_t cap, scfq_synth_info* info);

#ifdef __cplusplus
}
#endif
#endif /* SC_FQCOUNT_H */

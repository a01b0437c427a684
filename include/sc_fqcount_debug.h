/*
 * sc_fqcount_debug.h — diagnostic entry points of libsc_fqcount_hip.so. NOT part of the drop-in boundary
 * (include/sc_fqcount.h): nothing here is needed by a reference-side binding of `sc fq-count`
 * (src/fq_count.nim:14-53); the parity tests, bench.py's stream-ceiling probe and the measurement scripts use them.
 * No counting entry point calls any of these.
 */
#ifndef SC_FQCOUNT_DEBUG_H
#define SC_FQCOUNT_DEBUG_H

#include "sc_fqcount.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostic: ranges of this thread's last histogram session that the speculative K3 form served / that were (re)done
 * by the exact kernel (no guess, or a guess that did not verify). */
int  scfq_debug_hist_stats(uint64_t* fast_ranges, uint64_t* redone_ranges);
/* Diagnostic only (used by the parity tests as a second, independent device implementation):
 * byte-serial HIP kernel, one thread per 256 bytes. Never called by the counting entry points. */
int  scfq_debug_partial_simple(const void* device_ptr, uint64_t n, int prev_byte, scfq_partial* out);
/* Diagnostic only: the byte stream scfq_count_file() would scan for `path` (plain pread, BGZF block-parallel
 * inflate, or serial gzread), produced on the host without any device. Returns bytes written or a negative code. */
int64_t scfq_debug_read_file(const char* path, void* dst, uint64_t cap, uint64_t chunk_bytes);
/* host only: the same bytes with the first member read in two halves — the serial decoder up to the first block boundary at or after
 * `after_bytes` of output, then the decoder that takes a stream over in the middle of a member (exact bit, window, CRC-32 and length
 * so far): the hand-over of the device gzip path when a batch has no room */
int64_t scfq_debug_gz_resume(const char* path, uint64_t after_bytes, void* dst, uint64_t cap, uint64_t chunk_bytes);
/* Diagnostic only: inflate a whole BGZF image (host memory) with the device-side inflate kernel, result to host memory.
 * Returns the inflated size, SCFQ_EARG when the image is not pure BGZF or does not fit into cap, SCFQ_EGZ for a corrupt
 * member (deflate data, ISIZE or CRC-32). */
int64_t scfq_debug_bgzf_inflate(const void* image, uint64_t n, void* out, uint64_t cap);
/* Diagnostic only: milliseconds (best of `reps`) the scan kernel's LOAD STRUCTURE alone (same ranges, same non-temporal
 * LDS-DMA ring, no classification / accounting) needs for the whole tiles of a 4 KiB-aligned device buffer: the
 * practical read-stream ceiling on this device, reported next to the roofline by bench.py. Negative on error. */
double scfq_debug_stream_ms(const void* device_ptr, uint64_t n, int reps);

/* Host only — the two rules scfq_count_file_sharded cuts an ordinary (non-BGZF) .gz file of several members by, for the CPU tests.
 * scfq_debug_gz_member_boundary: the first position at or after `from` where a gzip member demonstrably starts (magic, no reserved
 * flag bit, a header that parses, deflate data that inflates cleanly for its first 64 KiB); the file's size when there is none, a
 * negative code on error.  *first_byte: the first byte the members from there inflate to (-1: none).
 * scfq_debug_gz_shard_fix: a shard's partial (+ histogram) that was scanned as if it began the input (prev_byte -1), put right for the
 * byte that really lies in front of it (true_prev 0..255; -1: it does begin the input) given the shard's first byte; flags: the
 * SCFQ_* flags of the scan (the line-start words are only touched with SCFQ_STRUCT_CHECK). */
int64_t scfq_debug_gz_member_boundary(const char* path, uint64_t from, int* first_byte);
int scfq_debug_gz_shard_fix(scfq_partial* p, uint64_t* hist, int true_prev, int first_byte, uint32_t flags);
/* Diagnostic only: where this process's time went so far.  The library marks its stages (first device call returned, context up,
 * buffers allocated, first copy queued, first kernel queued, session folded ...) with the milliseconds since it was loaded;
 * scfq_debug_stages writes them as one JSON array of [name, ms] pairs and returns its length (the length needed, with nothing
 * written, when cap is too small); scfq_debug_stage_mark lets the host add marks of its own (`sc`: main entered, rows out).
 * `sc fq-count --stats` prints the array; bench.py's cold-process legs carry it. */
int64_t scfq_debug_stages(char* buf, uint64_t cap);
void scfq_debug_stage_mark(const char* what);
/* The scan kernel instance and range geometry of the calling thread's last scan launch, e.g.
 * "fq_scan_tiles<false, 0, 2, true, false> tiles_per_range=100/50/25/12": the range size of every segment of the launch, one number
 * for a uniform launch (same contract as scfq_debug_stages: returns the length, writes when it fits). */
int64_t scfq_debug_last_scan_kernel(char* buf, uint64_t cap);
/* Host only, no device needed: the ranges a scan launch over `n` bytes would use when its first byte lies `ptr_offset` (0..4095) bytes
 * past a 4 KiB boundary, on a device of n_cu compute units (0: 256), under the SCFQ_* flags of the scan and the SCFQ_TILES_PER_RANGE /
 * SCFQ_TAPER_WAVES of the environment.  Range r of segment s covers the 4 KiB tiles first_tile[s] + (r - first_range[s]) *
 * tiles_per_range[s] up to + tiles_per_range[s], clipped to the next segment's first tile (n_tiles for the last).  Set struct_size. */
typedef struct scfq_scan_geometry {
  uint32_t struct_size;
  uint32_t n_segments;          /* 1..6; 1 = uniform ranges */
  uint64_t n_tiles, n_ranges;
  uint64_t first_range[6], first_tile[6], tiles_per_range[6];
} scfq_scan_geometry;
int scfq_debug_scan_geometry(uint64_t n, uint32_t ptr_offset, uint32_t flags, int n_cu, scfq_scan_geometry* out);
/* Stage times of the calling thread's last scfq_read_stats_buffer / scfq_read_stats_file, in milliseconds:
 * ms[0] line index (host clock around the synchronous index call), ms[1] R1 with its border pass, ms[2] R2 first pass
 * (sums and histograms), ms[3] R2 N50 / N90 (sort, scan, search; 0 when every read has the same length) — [1..3] are HIP-event
 * times, taken only while SCFQ_READSTATS_TIMING=1 is in the environment (zeros otherwise). Writes min(cap, 4) values, returns 4. */
int scfq_debug_read_stats_stages(double* ms, uint32_t cap);
/* Stage times of the calling thread's last scfq_cycles_buffer / scfq_cycles_file, in milliseconds: ms[0] line index (host
 * clock around the synchronous index call), ms[1] line pass (lengths, maxima, block plan), ms[2] C1, the counting kernel,
 * ms[3] finish (rows, tail, total; without the copy to the host) — [1..3] are HIP-event times, taken only while
 * SCFQ_CYCLES_TIMING=1 is in the environment (zeros otherwise). Writes min(cap, 4) values, returns 4. */
int scfq_debug_cycles_stages(double* ms, uint32_t cap);
/* Stage times of the calling thread's last scfq_kmers_buffer / scfq_kmers_file, in milliseconds: ms[0] line index (host
 * clock around the synchronous index call), ms[1] M1, the counting kernel, ms[2] finish (distinct, max_count, sum), ms[3] the
 * copies to the host (table and summary) — [1..3] are HIP-event times, taken only while SCFQ_KMERS_TIMING=1 is in the
 * environment (zeros otherwise). Writes min(cap, 4) values, returns 4. */
int scfq_debug_kmers_stages(double* ms, uint32_t cap);
/* Stage times of the calling thread's last scfq_adapters_buffer / scfq_adapters_file, in milliseconds: ms[0] line index (host
 * clock around the synchronous index call), ms[1] A1, the matching kernel, ms[2] A2, first positions into rows, ms[3] A3, the
 * sum of the rows (without the copies to the host) — [1..3] are HIP-event times, taken only while SCFQ_ADAPTERS_TIMING=1 is in
 * the environment (zeros otherwise). Writes min(cap, 4) values, returns 4. */
int scfq_debug_adapters_stages(double* ms, uint32_t cap);
/* Stage times of the calling thread's last scfq_insert_size_buffers / scfq_insert_size_files, in milliseconds: ms[0] the line
 * indexes (host clock around the synchronous index calls), ms[1] P1, the overlap kernel, ms[2] P2, the pass over the bins,
 * ms[3] the copy of bins and sums to the host — [1..3] are HIP-event times, taken only while SCFQ_INSERT_TIMING=1 is in the
 * environment (zeros otherwise). Writes min(cap, 4) values, returns 4. */
int scfq_debug_insert_size_stages(double* ms, uint32_t cap);
/* Stage times of the calling thread's last scfq_merge_buffers / scfq_merge_files, in milliseconds: ms[0] the line indexes (host
 * clock around the synchronous index calls), ms[1] P1, the overlap kernel, ms[2] M1 with the three scans, ms[3] M2, the write
 * kernel — [1..3] are HIP-event times, taken only while SCFQ_MERGE_TIMING=1 is in the environment (zeros otherwise). Writes
 * min(cap, 4) values, returns 4. */
int scfq_debug_merge_stages(double* ms, uint32_t cap);
/* Stage times of the calling thread's last scfq_trim_buffers / scfq_trim_files, in milliseconds: ms[0] P1, the overlap kernel (0
 * for single-end input), ms[1] T1, the decision kernel, ms[2] T2 with its scans, ms[3] T3, the write kernel — HIP-event times,
 * taken only while SCFQ_TRIM_TIMING=1 is in the environment (zeros otherwise). Writes min(cap, 4) values, returns 4. */
int scfq_debug_trim_stages(double* ms, uint32_t cap);
/* Stage times of the calling thread's last scfq_screen_buffers / scfq_screen_files, in milliseconds: ms[0] the line indexes of
 * paired input (host clock, 0 for single-end input), ms[1] S2, the lookup kernel, ms[2] S3 with its scans, ms[3] S4, the write
 * kernel — the last three HIP-event times, taken only while SCFQ_SCREEN_TIMING=1 is in the environment (zeros otherwise). Writes
 * min(cap, 4) values, returns 4. */
int scfq_debug_screen_stages(double* ms, uint32_t cap);
/* S1, the build kernel of that index, in milliseconds by HIP events; 0 for a NULL index. */
double scfq_debug_screen_build_ms(const scfq_screen_index* index);
/* Stage times of the calling thread's last scfq_demux_buffers / scfq_demux_files, in milliseconds: ms[0] X1, the assignment
 * kernel, ms[1] the radix sort, ms[2] X2 with its scans, ms[3] X3, the gather-write kernel — HIP-event times, taken only while
 * SCFQ_DEMUX_TIMING=1 is in the environment (zeros otherwise). Writes min(cap, 4) values, returns 4. */
int scfq_debug_demux_stages(double* ms, uint32_t cap);
/* Stage times of the calling thread's last fq-kcount calls, in milliseconds: ms[0] the line indexes of scfq_kcount_buffers /
 * scfq_kcount_files (host clock around the synchronous index calls), ms[1] H1, the counting kernel over every input in the
 * LAST pass (the clear of the table not included), ms[2] H2, the finish, ms[3] H3 of the last scfq_kcount_hist — [1..3] are
 * HIP-event times, taken only while SCFQ_KCOUNT_TIMING=1 is in the environment (zeros otherwise). Writes min(cap, 4) values,
 * returns 4. */
int scfq_debug_kcount_stages(double* ms, uint32_t cap);
/* Stage times of the calling thread's last scfq_norm_buffers / scfq_norm_files, in milliseconds: ms[0] the line indexes (host
 * clock around the synchronous index calls), ms[1] N1, the depth kernel (reads that keep their counts in device memory
 * included), ms[2] N2 with its scans, ms[3] N3, the write kernel — the last three HIP-event times, taken only while
 * SCFQ_NORM_TIMING=1 is in the environment (zeros otherwise). The counting pass of the two-pass form is read with
 * scfq_debug_kcount_stages. Writes min(cap, 4) values, returns 4. */
int scfq_debug_norm_stages(double* ms, uint32_t cap);
/* Stage times of the calling thread's last scfq_cplx_buffers / scfq_cplx_files, in milliseconds: ms[0] the line indexes of
 * paired input (host clock, 0 for single-end input), ms[1] D1, the interval kernel, ms[2] D2 with its scans, ms[3] D3, the write
 * kernel — the last three HIP-event times, taken only while SCFQ_CPLX_TIMING=1 is in the environment (zeros otherwise). Writes
 * min(cap, 4) values, returns 4. */
int scfq_debug_cplx_stages(double* ms, uint32_t cap);
/* Stage times of the calling thread's last scfq_rmdup_buffers / scfq_rmdup_files, in milliseconds: ms[0] the line indexes of
 * paired input (host clock, 0 for single-end input), ms[1] U1, the key hash, ms[2] the radix sort, ms[3] the rounds of U2 + U3,
 * ms[4] the class sizes, ms[5] U4 with its scans, ms[6] U5, the write kernel — the last six HIP-event times, taken only while
 * SCFQ_RMDUP_TIMING=1 is in the environment (zeros otherwise). Writes min(cap, 7) values, returns 7. */
int scfq_debug_rmdup_stages(double* ms, uint32_t cap);
/* Stage times of the calling thread's last scfq_repair_buffers / scfq_repair_files, in milliseconds: ms[0] the two line indexes
 * (host clock), ms[1] P1, the name spans, ms[2] the positional check with its readback, ms[3] P2, the name hash, ms[4] the radix
 * sort, ms[5] the rounds, ms[6] the mates (second sort, scans, kernel), ms[7] the pair list and the lengths with their scans,
 * ms[8] W1 and W2, the writers — all but the first HIP-event times, taken only while SCFQ_REPAIR_TIMING=1 is in the environment
 * (zeros otherwise). Writes min(cap, 9) values, returns 9. */
int scfq_debug_repair_stages(double* ms, uint32_t cap);
/* Stage times of the calling thread's last scfq_fa_index_buffer / scfq_fa_index_file, in milliseconds: ms[0] F1, the tile scan,
 * ms[1] F2, the scan over the tile records, ms[2] F3, the contig table's kernel, ms[3] unused (0) — HIP-event times, taken only
 * while SCFQ_FA_TIMING=1 is in the environment (zeros otherwise). Writes min(cap, 4) values, returns 4. */
int scfq_debug_fa_stages(double* ms, uint32_t cap);

#ifdef __cplusplus
}
#endif
#endif /* SC_FQCOUNT_DEBUG_H */

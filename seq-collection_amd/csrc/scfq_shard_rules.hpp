// scfq_shard_rules.hpp — where scfq_count_file_sharded may cut a compressed file, and what a cut costs the rank behind it: pure host code
// over the file's bytes (no device, nothing from HIP: a host compiler alone builds it, and the CPU tests reach it through
// scfq_debug_gz_member_boundary / scfq_debug_gz_shard_fix).  Every rank computes the same cuts from the bytes alone; what PROVES a cut is
// the rank in front of it (scfq_sharded.hpp).
#pragma once
#include "../../include/sc_fqcount.h"
#include "scfq_bgzf.hpp"
#include "scfq_gzfast.hpp"
#include "scfq_pgz.hpp"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

namespace scfq_shard {
namespace {      // (internal linkage: the library exports none of these)

// BGZF shards.  A BGZF file is cut where its members are: the first position at or after `from` where eight members follow one
// another (or a shorter run that ends exactly with the file) — every rank finds the SAME positions with this rule, from the bytes
// alone.  n when there is none.
inline uint64_t bgzf_boundary(const uint8_t* img, uint64_t n, uint64_t from) {
  for (uint64_t p = from; p + 18 <= n;) {
    const void* hit = std::memchr(img + p, 0x1f, (size_t)(n - 17 - p));
    if (!hit) break;
    p = (uint64_t)(static_cast<const uint8_t*>(hit) - img);
    uint64_t q = p;
    int k = 0;
    while (k < 8 && q < n) {
      uint32_t hl = 0;
      const uint32_t bs = scfq_bgzf::block_size(img + q, n - q, &hl);
      if (!bs || q + bs > n || scfq_bgzf::rd32(img + q + bs - 4) > (1u << 16)) break;
      q += bs;
      ++k;
    }
    if (k == 8 || (k > 0 && q == n)) return p;
    ++p;
  }
  return n;
}
// Where rank r's members start (r > 0) and the byte in front of its first inflated byte: the boundary rule gives a member; the rank's
// range starts BEHIND the first non-empty member from there, which the rank inflates on the host (one member of at most 64 KiB)
// for its last byte.  Both neighbours compute the same cut.  false: a member that does not inflate (the file is damaged).
inline bool bgzf_cut(const uint8_t* img, uint64_t n, uint64_t from, uint64_t* cut, int* prev) {
  uint64_t p = bgzf_boundary(img, n, from);
  *prev = -1;
  while (p < n) {
    uint32_t hl = 0;
    const uint32_t bs = scfq_bgzf::block_size(img + p, n - p, &hl);
    if (!bs || p + bs > n) { *cut = n; return false; }
    const uint32_t isize = scfq_bgzf::rd32(img + p + bs - 4);
    if (isize == 0) { p += bs; continue; }               // (an empty member — the end-of-file marker — has no last byte)
    if (isize > (1u << 16)) { *cut = n; return false; }
    std::vector<scfq_bgzf::Block> one{{p, bs, hl, isize, scfq_bgzf::rd32(img + p + bs - 8), 0}};
    std::vector<uint8_t> out(isize);
    if (scfq_bgzf::inflate_blocks(img, one, 0, 1, out.data())) { *cut = n; return false; }
    *prev = out[isize - 1];
    *cut = p + bs;
    return true;
  }
  *cut = n;
  return true;
}
// ---- ordinary gzip shards: a file of SEVERAL members is cut where members start ------------------------------------------------
// (`cat a.fq.gz b.fq.gz`, `pigz -i`, per-lane or per-tile members of a sequencer's writer.)  Unlike BGZF a member does not say how long
// it is, so a rank that starts in the middle of the file can only LOOK for a member start: the three magic bytes with no reserved flag
// bit set, a header that parses, and deflate data that inflates cleanly for its first 64 KiB — a block header made of chance bits
// survives the Huffman-code tests about once in 4000 tries and then dies within a few hundred symbols.  That makes a false start
// unlikely, not impossible; what PROVES a cut is the rank before it: its members must end — trailer, CRC-32 and ISIZE checked —
// exactly where the next rank began (gz_shard_fold below), or every rank falls back to rank 0 reading the whole file.
//
// gz_member_here: true when a member demonstrably starts at p.  *first_byte: the first byte it (or, when it is empty, a member
// behind it, inside [p, stop)) inflates to; -1 when there is none in that stretch.
inline bool gz_member_here(const uint8_t* img, uint64_t n, uint64_t p, uint64_t stop, int* first_byte) {
  *first_byte = -1;
  std::vector<uint8_t> buf;
  bool first = true;
  while (p < n && (first || p < stop)) {
    if (n - p < 18 || img[p] != 0x1f || img[p + 1] != 0x8b || img[p + 2] != 8 || (img[p + 3] & 0xE0)) return !first;
    const long h = scfq_gzfast::member_header(img + p, (size_t)(n - p));
    if (h <= 0) return !first;
    const uint64_t sample = std::min<uint64_t>(n - (p + (uint64_t)h), 64u << 10);
    if (buf.empty()) buf.resize(scfq_gzfast::kWindow + (2u << 20));
    auto dec = std::unique_ptr<scfq_inflate::Decoder>(new scfq_inflate::Decoder());
    dec->begin(img + p + h, img + p + h + sample);
    uint8_t* o = buf.data() + scfq_gzfast::kWindow;
    const int r = dec->run(o, buf.data() + buf.size());
    const uint64_t got = (uint64_t)(o - (buf.data() + scfq_gzfast::kWindow));
    if (r == scfq_inflate::kErrData) return !first;
    if (r == scfq_inflate::kErrTruncated && sample == n - (p + (uint64_t)h)) return !first;      // (the FILE ends inside the member: damaged)
    if (got) { *first_byte = buf[scfq_gzfast::kWindow]; return true; }
    if (r != scfq_inflate::kStreamEnd) return true;            // (no byte yet and no end either: a long run of empty stored blocks; rare, harmless)
    // an empty member: the first byte is a later member's
    const uint8_t* t = dec->end_of_stream();
    first = false;
    p = (uint64_t)(t - img) + 8;
  }
  return true;
}
// the first demonstrable member start at or after `from`; n when there is none.  *first_byte as above (stop: the end of the rank's stretch)
// (limit: only starts in front of this offset are looked for — a rank that only wants to know what its own share of the file holds does
// not walk a 25 GB member to its end)
inline uint64_t gz_member_boundary(const uint8_t* img, uint64_t n, uint64_t from, uint64_t stop, int* first_byte, uint64_t limit = ~0ull) {
  *first_byte = -1;
  const uint64_t last = std::min<uint64_t>(limit, n >= 17 ? n - 17 : 0);       // first offset that is no candidate any more
  for (uint64_t p = from; p < last;) {
    const void* hit = std::memchr(img + p, 0x1f, (size_t)(last - p));
    if (!hit) break;
    p = (uint64_t)(static_cast<const uint8_t*>(hit) - img);
    if (img[p + 1] == 0x8b && img[p + 2] == 8 && !(img[p + 3] & 0xE0) && gz_member_here(img, n, p, std::max(stop, p + 1), first_byte)) return p;
    ++p;
  }
  return n;
}

// A shard that was scanned as if it began the input (no byte before it is known when its scan starts: that byte is the LAST one the
// member before inflates to), put right once that byte is known.  Two things depend on it: a '\n' at the shard's first position ends
// a line whose '\r' — if the byte before is one — is not part of that line (len, and the quality histogram's '\r' bin, are taken back
// exactly as a range of the device path takes back a '\r' that lies in the range before it: u64 modular); and the shard's first byte
// starts a line only when the byte before is a '\n' (K4's line starts, and what they begin with).
inline void gz_shard_fix(scfq_partial* p, uint64_t* hist, int true_prev, int first_byte, uint32_t flags) {
  if (p->bytes == 0 || true_prev < 0 || first_byte < 0) return;
  if (first_byte == '\n' && true_prev == '\r') {
    p->len[0] -= 1;
    if (hist && (p->hist_class == 0 || p->hist_class == 1)) hist[0 * 256 + 13] -= 1;
  }
  if ((flags & SCFQ_STRUCT_CHECK) && true_prev != '\n') {
    p->starts[0] -= 1;
    if (first_byte == '@') p->first_at[0] -= 1;
    if (first_byte == '+') p->first_plus[0] -= 1;
  }
}
// ---- ONE member over several ranks: the deflate stream is cut where BLOCKS start -----------------------------------------------------
// gz_block_boundary: the first bit at or after byte `from` where a dynamic-Huffman block demonstrably starts (scfq_pgz.hpp's test: a
// header that parses — complete code-length, literal/length and distance codes — and 4096 symbols that decode cleanly); 0 when there is
// none within `span` bytes.  Both neighbours of a cut compute it from the same bytes.  What proves it is the rank before: its chain must
// arrive at exactly this bit (GzStretch: stop_bit), or every rank falls back to rank 0 reading the whole file.
inline uint64_t gz_block_boundary(const uint8_t* img, uint64_t n, uint64_t from, uint64_t span) {
  const uint64_t to = std::min<uint64_t>(from + span, n > 16 ? n - 16 : 0);
  if (from >= to) return 0;
  auto d = std::unique_ptr<scfq_inflate::Decoder>(new scfq_inflate::Decoder());
  std::vector<uint16_t> scratch(scfq_pgz::kWindow + scfq_pgz::kTrialSymbols + 2 * scfq_inflate::kOutSlack);
  for (uint32_t i = 0; i < scfq_pgz::kWindow; ++i) scratch[i] = (uint16_t)(0x8000u | i);
  for (uint64_t b = from * 8; b < to * 8; ++b)
    if (scfq_pgz::plausible_block(*d, img, img + n, b, scratch)) return b;
  return 0;
}

}  // namespace
}  // namespace scfq_shard

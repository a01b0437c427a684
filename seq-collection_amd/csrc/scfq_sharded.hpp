// scfq_sharded.hpp — scfq_count_file_sharded (include/sc_fqcount.h): one file counted by all ranks of a communicator.  Included by
// scfq_api.hip behind its ingest paths (Session, InputFile, ingest, ingest_bgzf_device, ingest_gz_device, count_file_partial); the rules
// that say where a compressed file may be cut are scfq_shard_rules.hpp.
//
// THE INVARIANT.  Every rank takes part in every collective, in the same order, whatever went wrong locally — a rank that cannot open the
// file, has no device or finds its bytes damaged still sends its word, its row and its (identity) partial — so that no rank waits for
// one that has left.  The collectives of a call, in order:
//   1. the vote all-gather: one word per rank; when world > 1 and SCFQ_SHARD_BGZF is not 0, for a ".gz" name;
//   2. in the block scheme, exactly ONE all-gather of the map rows per rank: inside the ingest (between a stretch's decode and its bytes) or,
//      for a rank whose ingest never got that far, right after it (BlockShard::run);
//   3. in both gzip schemes, the all-gather of the ranks' rows (partial, first byte, CRC-32 and length of the stretch);
//   4. the final scfq_comm_exchange, on every path that did not finalise from the rows of 3.
// The code keeps that list true by construction: a scheme function counts this rank's share and RETURNS its status — it has no way out past
// a collective, and none but the block scheme (2, behind the one `exchanged` flag) issues one; the entry point issues 1, 3 and 4 and leaves
// early only when a collective itself failed (the communicator is broken for every rank then) or after every rank has folded the same rows.
#pragma once

namespace {
using namespace scfq_shard;

// ---- the vote: what a rank can tell of the file from its own share of the bytes ----------------------------------------------------------
enum : uint64_t {
  kVoteCannot = 0,        // cannot shard (cannot open or map the file, a switch says no, a cut was not found)
  kVoteBgzf = 1,          // pure BGZF in this rank's range, and its cuts found
  kVoteGzip = 2,          // (bit 1) an ordinary gzip file, as far as this rank can tell without walking it
  kVoteOneMember = 4,     // (bit 2, with bit 1) at most one member starts in this rank's share: the block scheme's condition
};
struct ShardScheme { bool bgzf = false, gz = false, blocks = false; };      // (blocks implies gz)
ShardScheme agree_on_scheme(const std::vector<uint64_t>& votes) {
  ShardScheme s{true, true, true};
  for (const uint64_t v : votes) {
    s.bgzf = s.bgzf && v == kVoteBgzf;
    s.gz = s.gz && (v & kVoteGzip) != 0;
    s.blocks = s.blocks && v == (kVoteGzip | kVoteOneMember);
  }
  return s;
}

struct BgzfRange { uint64_t lo = 0, hi = 0; int prev = -1; };      // this rank's members, and the byte in front of its first inflated byte

// This rank's word of the vote; maps the file when a scheme could take it (so every rank of an agreed scheme holds the image).
// BGZF (bgzip) input shards where its members are: rank r takes the members that start in its byte range, inflates them on its device and
// scans them; the partials fold as for a plain file.  The ranks AGREE (one all-gather of a word) that every one of them found its cuts
// and saw nothing but BGZF members of at most 64 KiB in its range — otherwise, and for every gzip layout no scheme takes (one small deflate
// stream has no shards), rank 0 inflates and scans all of it and the others contribute the identity.
uint64_t shard_vote(InputFile& in, int rank, int world, BgzfRange* b) {
  uint64_t vote = kVoteCannot;
  if (in.is_open() && in.size() > 0 && bgzf_device_enabled() && is_bgzf_input(in) && in.map()) {
    const uint8_t* img = in.img();
    const uint64_t size = in.size();
    bool ok = true;
    int prev_hi = -1;
    if (rank > 0) ok = bgzf_cut(img, size, size / (uint64_t)world * (uint64_t)rank, &b->lo, &b->prev);
    if (rank + 1 < world) ok = bgzf_cut(img, size, size / (uint64_t)world * (uint64_t)(rank + 1), &b->hi, &prev_hi) && ok;
    else b->hi = size;
    if (b->hi < b->lo) b->hi = b->lo;
    ok = ok && (b->lo == b->hi || bgzf_is_pure(img + b->lo, b->hi - b->lo));
    vote = ok ? kVoteBgzf : kVoteCannot;
  }
  // An ordinary gzip file: rank r's members are those that start in [g_lo, g_hi), where a cut is the first demonstrable member start at or
  // after size * r / world (gz_member_boundary; both neighbours find the same one from the bytes alone).  A file of ONE member gives every
  // cut but rank 0's as "none": rank 0 has all of it, as before.
  static const bool shard_gz = env_int("SCFQ_SHARD_GZ", 1) != 0;
  if (!vote && !in.mapped() && in.is_open() && shard_gz && gz_device_enabled() && in.regular() && in.size() >= 64 && in.map()) {
    const uint8_t* img = in.img();
    const uint64_t size = in.size();
    const uint64_t nom_lo = size / (uint64_t)world * (uint64_t)rank, nom_hi = rank + 1 < world ? size / (uint64_t)world * (uint64_t)(rank + 1) : size;
    // (kVoteGzip: the cuts themselves are looked for once the ranks have agreed on a scheme; a rank that then finds none says so in the
    // gathered rows)
    int fb = -1;
    if (rank != 0 || gz_member_here(img, size, 0, 1, &fb)) vote = kVoteGzip;
    // (kVoteOneMember: at most ONE member starts inside this rank's share of the file — rank 0: none behind the file's first.  When every
    // rank says so the members are big ones — one, or a few: `cat lane1.gz lane2.gz` — and the ranks cut the deflate streams where BLOCKS
    // start, a member start being a cut of its own: no rank is left without work, as the member scheme leaves the ranks in whose share
    // no member starts.  The search stays inside the rank's share.)
    static const bool shard_blocks = env_int("SCFQ_SHARD_GZ_BLOCKS", 1) != 0;
    if (vote == kVoteGzip && shard_blocks && size >= (uint64_t)world * (8ull << 20)) {
      const uint64_t m1 = gz_member_boundary(img, size, rank == 0 ? 1 : nom_lo, size, &fb, nom_hi);
      const uint64_t m2 = m1 < nom_hi ? gz_member_boundary(img, size, m1 + 1, size, &fb, nom_hi) : size;
      if (rank == 0 ? m1 >= nom_hi : m2 >= nom_hi) vote |= kVoteOneMember;
    }
  }
  return vote;
}

// ---- the four schemes: each counts this rank's share into *mine (+ hist) and returns the rank's status ------------------------------------

// a plain file: byte ranges
int shard_plain(InputFile& in, int rank, int world, const scfq_opts& o, scfq_partial* mine, std::vector<uint64_t>& hist) {
  if (!in.regular()) return SCFQ_EOPEN;
  const uint64_t size = in.size();
  const uint64_t lo = size / (uint64_t)world * (uint64_t)rank + std::min<uint64_t>(size % (uint64_t)world, (uint64_t)rank);
  const uint64_t hi = size / (uint64_t)world * (uint64_t)(rank + 1) + std::min<uint64_t>(size % (uint64_t)world, (uint64_t)rank + 1);
  int prev = -1;
  if (lo) { uint8_t pb; if (pread(in.fd, &pb, 1, (off_t)(lo - 1)) != 1) return SCFQ_EIO; prev = pb; }
  Session s;
  int local = s.open(o, lo == 0);
  if (!local && hi > lo) {
    FdSource src(in.fd, lo, hi);
    local = ingest(s.c, src, prev, o.flags, std::min<uint64_t>(opt_chunk(&o), std::max<uint64_t>((hi - lo + 4095) & ~4095ull, 4096)), o.flags & SCFQ_TIMING);
  }
  return local ? local : s.finish(o.flags & SCFQ_QUAL_HIST, mine, hist);
}

// BGZF: the members that start in this rank's range (shard_vote found the cuts)
int shard_bgzf_members(InputFile& in, const BgzfRange& b, int rank, const scfq_opts& o, scfq_partial* mine, std::vector<uint64_t>& hist) {
  const bool timing = o.flags & SCFQ_TIMING;
  int local = Session::set_device(o);
  if (local || b.hi <= b.lo) return local;
  Session s;
  if ((local = s.open(rank == 0))) return local;
  local = ingest_bgzf_device(s.c, in.img() + b.lo, b.hi - b.lo, o.flags, opt_chunk(&o), timing, b.prev, in.fd, b.lo);
  if (local == kFallbackToHost || local == kNotPureBgzf) {
    // no room for the device path's buffers (kNotPureBgzf cannot happen: the range was walked): the host's block-parallel
    // inflate over the same members
    local = s.restart(rank == 0);
    if (!local) { BgzfSource src(in.fd, b.hi); src.pos = b.lo; local = ingest(s.c, src, b.prev, o.flags, opt_chunk(&o), timing); }
  }
  return local ? local : s.finish(o.flags & SCFQ_QUAL_HIST, mine, hist);
}

// Ordinary gzip, several members: every rank inflates and scans the members of its stretch as if they were a file of their own (device
// path; the host's decoder when that declines), scanned as if they began the input.  *first_byte: the stretch's first inflated byte (-1:
// none), for the fold (gz_fold_rows) to put the byte before the stretch right.
int shard_gz_members(InputFile& in, int rank, int world, const scfq_opts& o, scfq_partial* mine, std::vector<uint64_t>& hist, int* first_byte) {
  const uint8_t* img = in.img();
  const uint64_t size = in.size();
  const bool timing = o.flags & SCFQ_TIMING;
  // (the cuts: the first demonstrable member start at or after size * r / world and the one after the next rank's)
  uint64_t g_lo = 0, g_hi = 0;
  int f_hi = -1;
  const uint64_t nom_lo = size / (uint64_t)world * (uint64_t)rank, nom_hi = size / (uint64_t)world * (uint64_t)(rank + 1);
  g_hi = rank + 1 < world ? gz_member_boundary(img, size, nom_hi, nom_hi, &f_hi) : size;
  if (rank == 0) g_lo = 0, (void)gz_member_here(img, size, 0, std::max<uint64_t>(g_hi, 1), first_byte);
  else g_lo = gz_member_boundary(img, size, nom_lo, g_hi, first_byte);
  if (g_hi < g_lo) g_hi = g_lo;
  int local = Session::set_device(o);
  if (local || g_hi <= g_lo) return local;
  Session s;
  if ((local = s.open(rank == 0))) return local;
  const uint64_t len = g_hi - g_lo;
  uint64_t end_off = 0;
  static const uint64_t min_bytes = (uint64_t)std::max(0, env_int("SCFQ_GZ_DEVICE_MIN_MB", 4)) << 20;
  local = len >= std::max<uint64_t>(min_bytes, 64) ? ingest_gz_device(s.c, img + g_lo, len, o.flags, timing, &end_off, in.fd, g_lo) : kFallbackToHost;
  if (local == kFallbackToHost) {
    // (small stretches, and whatever the device path declines: the host's decoder over the same bytes — Resume from the first
    // block of the stretch's first member, an empty window, no prefix)
    s.drain();
    local = s.restart(rank == 0);
    const long h = scfq_gzfast::member_header(img + g_lo, (size_t)len);
    if (!local && h <= 0) local = SCFQ_EGZ;
    if (!local) {
      struct RangeSource : Source {
        scfq_gzfast::Resume rs;
        int64_t fill(uint8_t* dst, uint64_t cap) override { const int64_t r = rs.next_chunk(dst, cap); return r < 0 ? (int64_t)SCFQ_EGZ : r; }
      } src;
      const std::vector<uint8_t> no_window(scfq_gzfast::kWindow, 0);
      src.rs.open(img + g_lo, (size_t)len, (uint64_t)h * 8, no_window.data(), 0, 0, 0);
      local = ingest(s.c, src, -1, o.flags, opt_chunk(&o), timing);
      end_off = src.rs.end_offset();
    }
  }
  // the stretch must be members and nothing else, up to the very byte the next stretch starts at (only the file's last stretch may
  // have the trailing bytes gzread ignores behind it)
  if (!local && end_off != len && g_hi < size) { local = SCFQ_EGZ; std::snprintf(g_err, sizeof g_err, "shard %d: its members end at byte %llu, the next shard begins at %llu", rank, (unsigned long long)(g_lo + end_off), (unsigned long long)g_hi); }
  return local ? local : s.finish(o.flags & SCFQ_QUAL_HIST, mine, hist);
}

// Ordinary gzip, big members (one, or a few): rank r's stretch is [cut_r, cut_{r+1}) — a cut is the member start inside the rank's share of
// the file when there is one, else the first block start at or behind the share's first byte; a stretch never crosses a member's end.
// The cuts, and what the ranks exchange about them in the middle of the ingest.
struct BlockShard {
  struct Cut { bool found = false, member = false; uint64_t byte = 0, bit = 0; };
  struct Group { uint64_t first, last, end_byte; };      // a member: the ranks that hold a stretch of it, the offset just behind its trailer
  scfq_comm* comm;
  int rank, world;
  uint64_t size = 0;
  Cut c_lo, c_hi;
  bool cuts_ok = false;
  // the stretch as the pipeline sees it: an image that begins at the member's start (a member cut) or at the file's (a block cut:
  // bit positions are the file's), and ends where the next member starts (a member cut) or with the file
  uint64_t base = 0, image_end = 0;
  std::vector<uint8_t> window;      // what is in front of this rank's stretch, once the maps of the stretches before it are known
  std::vector<Group> groups;        // for the CRC check at the fold (gz_fold_rows)
  bool exchanged = false, agree = false;
  int comm_rc = SCFQ_OK;
  int local = SCFQ_OK;              // this rank's status so far (exchange() reports it to the others)
  int first_byte = -1;              // results, for this rank's row: the stretch's first byte, raw CRC-32 and length
  uint64_t crc_raw = 0, len = 0;

  BlockShard(scfq_comm* comm_, int rank_, int world_) : comm(comm_), rank(rank_), world(world_) {}

  Cut cut_of(const uint8_t* img, int r) const {
    Cut ct;
    if (r <= 0) { ct.found = true; ct.member = true; return ct; }
    if (r >= world) { ct.found = true; ct.member = true; ct.byte = size; ct.bit = size * 8; return ct; }
    const uint64_t lo = size / (uint64_t)world * (uint64_t)r, hi = r + 1 < world ? size / (uint64_t)world * (uint64_t)(r + 1) : size;
    int fb = -1;
    const uint64_t m = gz_member_boundary(img, size, lo, size, &fb, hi);
    if (m < hi) { ct.found = true; ct.member = true; ct.byte = m; ct.bit = m * 8; return ct; }
    const uint64_t bb = gz_block_boundary(img, size, lo, std::min<uint64_t>(16ull << 20, hi - lo));
    if (bb && (bb >> 3) < hi) { ct.found = true; ct.bit = bb; ct.byte = bb >> 3; }
    return ct;
  }

  // Collective 2.  What every rank learns of every stretch — [proven, cut kinds and positions, bytes, where its member ended, the map] —
  // and what it makes of it: the window in front of its own stretch = the maps of the stretches before it IN THE SAME MEMBER, applied in
  // order to the member's (empty) start.  Returns 0 when the cuts joined up and x has its window.
  int exchange(GzStretch& x, bool proven) {
    const uint32_t kMapWords = (uint32_t)(scfq_gzfast::kWindow / 4), kHead = 8, w1 = kHead + kMapWords;
    exchanged = true;
    std::vector<uint64_t> row1(w1, 0), rows1((size_t)world * w1, 0);
    // (a stretch that ends at a member cut must have ended WITH its member, exactly at the cut: nothing but members in between)
    proven = proven && cuts_ok && !local && x.map.size() == scfq_gzfast::kWindow && x.member_ended == c_hi.member &&
             (!c_hi.member || c_hi.byte == size || base + x.end_byte == c_hi.byte);
    row1[0] = proven ? 1 : 0;
    row1[1] = c_lo.member; row1[2] = c_lo.bit; row1[3] = c_hi.member; row1[4] = c_hi.bit;
    row1[5] = x.out_bytes; row1[6] = base + x.end_byte;
    if (proven) std::memcpy(row1.data() + kHead, x.map.data(), 2 * scfq_gzfast::kWindow);
    comm_rc = scfq_comm_allgather_u64(comm, row1.data(), w1, rows1.data(), 0);
    if (comm_rc) return 1;
    agree = true;
    for (int r = 0; r < world; ++r) {
      const uint64_t* rr = rows1.data() + (size_t)r * w1;
      const uint64_t* nx = r + 1 < world ? rows1.data() + (size_t)(r + 1) * w1 : nullptr;
      agree = agree && rr[0] == 1 && (nx ? (rr[3] == nx[1] && rr[4] == nx[2]) : (rr[3] == 1 && rr[4] == size * 8));      // a stretch ends where the next begins
    }
    if (!agree) return 1;
    // the members' ends, for the CRC check at the fold: [first rank, last rank, offset just behind the trailer]
    groups.clear();
    for (int r = 0, a0 = 0; r < world; ++r) {
      const uint64_t* rr = rows1.data() + (size_t)r * w1;
      if (rr[3] == 1) { groups.push_back({(uint64_t)a0, (uint64_t)r, rr[6]}); a0 = r + 1; }
    }
    int first_of_member = rank;
    while (first_of_member > 0 && rows1[(size_t)first_of_member * w1 + 1] == 0) --first_of_member;
    std::vector<uint8_t> next(scfq_gzfast::kWindow, 0);
    uint64_t before_bytes = 0;
    for (int r = first_of_member; r < rank; ++r) {
      const uint16_t* m = reinterpret_cast<const uint16_t*>(rows1.data() + (size_t)r * w1 + kHead);
      for (uint32_t i = 0; i < scfq_gzfast::kWindow; ++i) next[i] = (m[i] & 0x8000u) ? window[m[i] & 0x7FFFu] : (uint8_t)m[i];
      window.swap(next);
      before_bytes += rows1[(size_t)r * w1 + 5];
    }
    x.window = window.data();
    x.valid = (uint32_t)std::min<uint64_t>(scfq_gzfast::kWindow, before_bytes);
    return 0;
  }

  // ONE pass (the default): the stretch's proven symbols are kept — two bytes per inflated byte — while its map goes out and the window
  // comes back (GzStretch::exchange), then they become bytes.  SCFQ_SHARD_GZ_KEEP=0: two passes, the second decoding again (what a
  // device short of memory would want: nothing is kept between them).
  bool keep_symbols() const {
    static const bool keep_env = env_int("SCFQ_SHARD_GZ_KEEP", 1) != 0;
    if (!keep_env || local) return keep_env;
    // (the store of kept symbols: two bytes per inflated byte — taken as 12 per compressed byte of the stretch, FASTQ compresses 3 - 5
    // times — must leave the pipeline its own 12 GB or so: a rank whose device is short of that goes over its stretch twice instead;
    // the ranks need not agree on this, the exchange in the middle is the same)
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = 0; }
    // (SCFQ_TEST_DEVICE_FREE_GB: the tests' way of putting a rank on a device that is short of memory)
    static const int test_free_gb = env_int("SCFQ_TEST_DEVICE_FREE_GB", -1);
    if (test_free_gb >= 0) free_b = std::min<size_t>(free_b, (size_t)test_free_gb << 30);
    return (c_hi.byte > c_lo.byte ? c_hi.byte - c_lo.byte : 0) * 12 + (16ull << 30) <= (uint64_t)free_b;
  }

  // Counts this rank's stretch; issues collective 2 exactly once, whatever happens before it.  Returns `local`; comm_rc says whether the
  // collective itself failed (the entry point leaves with it).
  int run(InputFile& in, const scfq_opts& o, scfq_partial* mine, std::vector<uint64_t>& hist) {
    const uint8_t* img = in.img();
    const bool timing = o.flags & SCFQ_TIMING;
    size = in.size();
    local = Session::set_device(o);
    c_lo = cut_of(img, rank);
    c_hi = cut_of(img, rank + 1);
    const long h0 = scfq_gzfast::member_header(img, (size_t)size);
    base = c_lo.member ? c_lo.byte : 0;
    image_end = c_hi.member ? c_hi.byte : size;
    GzStretch sx;
    sx.start_bit = c_lo.member ? 0 : c_lo.bit;
    sx.stop_bit = c_hi.member ? 0 : c_hi.bit - 8 * base;
    cuts_ok = h0 > 0 && c_lo.found && c_hi.found && image_end > base + 64 && (c_hi.member || c_hi.bit > (c_lo.member ? c_lo.byte * 8 : c_lo.bit));
    window.assign(scfq_gzfast::kWindow, 0);
    Session s;
    if (!local) local = s.take();
    uint64_t out1 = 0;
    if (keep_symbols()) {
      if (!local && cuts_ok) local = s.restart(rank == 0);
      if (!local && cuts_ok) {
        sx.exchange = [this](GzStretch& x, bool proven) { return exchange(x, proven); };
        const int r1 = ingest_gz_device(s.c, img + base, image_end - base, o.flags, timing, nullptr, in.fd, base, &sx);
        if (r1 == kFallbackToHost) { if (agree) local = SCFQ_EGZ; } else if (r1) local = r1;
      }
      if (!exchanged) (void)exchange(sx, false);
      out1 = sx.out_bytes;
    } else {
      GzStretch sx1 = sx;
      sx1.map_only = true;
      bool proven = false;
      if (!local && cuts_ok) {
        const int r1 = ingest_gz_device(s.c, img + base, image_end - base, o.flags, false, nullptr, in.fd, base, &sx1);
        if (r1 == SCFQ_OK) proven = true; else if (r1 != kFallbackToHost) local = r1;
      }
      (void)exchange(sx1, proven);
      out1 = sx1.out_bytes;
      if (agree) {
        sx.window = sx1.window;
        sx.valid = sx1.valid;
        if (!local) local = s.restart(rank == 0);
        if (!local) {
          const int r2 = ingest_gz_device(s.c, img + base, image_end - base, o.flags, timing, nullptr, in.fd, base, &sx);
          local = r2 == kFallbackToHost ? SCFQ_EGZ : r2;
        }
      }
    }
    if (comm_rc) return local;
    if (agree) {
      if (!local && sx.out_bytes != out1) local = SCFQ_EGZ;
      if (!local) local = s.finish(o.flags & SCFQ_QUAL_HIST, mine, hist);
      first_byte = sx.first_byte;
      crc_raw = sx.crc_raw;
      len = sx.out_bytes;
    } else {
      local = SCFQ_EGZ;      // (not an error of this rank: the rows send every rank to the fall-back)
      std::snprintf(g_err, sizeof g_err, "the block cuts of a one-member file did not join up");
    }
    return local;
  }
};

// ---- the gathered rows of the gzip schemes ----------------------------------------------------------------------------------------------
// this rank's row: its partial with [status, first byte + 1 (0: the stretch holds no byte), raw CRC-32 and length of the stretch (block
// scheme)] in the reserved words, then its histogram
std::vector<uint64_t> gz_row(scfq_partial* mine, std::vector<uint64_t>& hist, bool want_hist, int local, int first_byte, uint64_t crc_raw, uint64_t len) {
  if (local) scfq_partial_identity(mine, want_hist ? hist.data() : nullptr);
  mine->reserved[0] = (uint64_t)(int64_t)local;
  mine->reserved[1] = (uint64_t)(first_byte + 1);
  mine->reserved[2] = crc_raw;
  mine->reserved[3] = len;
  std::vector<uint64_t> row(SCFQ_PARTIAL_WORDS + (want_hist ? SCFQ_HIST_WORDS : 0));
  std::memcpy(row.data(), mine, sizeof *mine);
  if (want_hist) std::memcpy(row.data() + SCFQ_PARTIAL_WORDS, hist.data(), SCFQ_HIST_WORDS * sizeof(uint64_t));
  return row;
}

// The rank-order fold of the gathered rows into *all (+ hist_all), the same on every rank.  *joined = false — and nothing folded — when a
// rank failed or, in the block scheme (blk), a member's CRC-32 / ISIZE does not match the join of its stretches': a cut that was no member
// or block start after all, or a damaged file.  Each stretch was scanned as if it began the input; the byte before it (the last byte of the
// stretch before it) is put right first: gz_shard_fix.
int gz_fold_rows(std::vector<uint64_t>& rows, int world, const char* path, uint32_t flags, const BlockShard* blk, scfq_partial* all, std::vector<uint64_t>& hist_all, bool* joined) {
  const bool want_hist = flags & SCFQ_QUAL_HIST;
  const uint32_t words = SCFQ_PARTIAL_WORDS + (want_hist ? SCFQ_HIST_WORDS : 0);
  bool all_ok = true;
  for (int r = 0; r < world; ++r) all_ok = all_ok && rows[(size_t)r * words + offsetof(scfq_partial, reserved) / 8] == 0;
  if (all_ok && blk) {
    // every member's CRC-32 and ISIZE against the join of its stretches' (x^(8 |part|), as between the batches of one stretch)
    InputFile trailers(path);      // (opened again: the scheme's descriptor went with its mapping, before the rows were gathered)
    for (const BlockShard::Group& gpm : blk->groups) {
      uint32_t raw = 0;
      uint64_t len = 0;
      for (uint64_t r = gpm.first; r <= gpm.last; ++r) {
        const uint64_t* rr = rows.data() + (size_t)r * words + offsetof(scfq_partial, reserved) / 8;
        raw = gz_mulmod(gz_xpow8n(rr[3]), raw) ^ (uint32_t)rr[2];
        len += rr[3];
      }
      const uint32_t crc = raw ^ gz_mulmod(gz_xpow8n(len), 0xFFFFFFFFu) ^ 0xFFFFFFFFu;
      uint8_t t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      const bool have_trailer = trailers.is_open() && gpm.end_byte >= 8 && pread(trailers.fd, t, 8, (off_t)(gpm.end_byte - 8)) == 8;
      if (!have_trailer || scfq_bgzf::rd32(t) != crc || scfq_bgzf::rd32(t + 4) != (uint32_t)(len & 0xFFFFFFFFull)) all_ok = false;      // damaged: gzread's verdict, from rank 0's readers
    }
    if (blk->groups.empty()) all_ok = false;
  }
  *joined = all_ok;
  if (!all_ok) return SCFQ_OK;
  scfq_partial_identity(all, want_hist ? hist_all.data() : nullptr);
  int before = -1;      // the last byte in front of the stretch being added (-1: nothing yet)
  for (int r = 0; r < world; ++r) {
    scfq_partial pr;
    std::memcpy(&pr, rows.data() + (size_t)r * words, sizeof pr);
    uint64_t* hr = want_hist ? rows.data() + (size_t)r * words + SCFQ_PARTIAL_WORDS : nullptr;
    gz_shard_fix(&pr, hr, before, (int)pr.reserved[1] - 1, flags);
    pr.reserved[1] = pr.reserved[2] = pr.reserved[3] = 0;
    if (const int rc = scfq_partial_combine(all, &pr, want_hist ? hist_all.data() : nullptr, hr)) return rc;
    if (pr.bytes) before = (int)(pr.last_byte & 0xFF);
  }
  return SCFQ_OK;
}

// The fall-back of both kinds — no scheme agreed on, or the cuts of one did not join up: rank 0 reads the whole file the ordinary way (its
// readers are gzread byte for byte, error text included) and the others give the identity to the final exchange.
int rank0_reads_all(const char* path, const scfq_opts& o, int rank, scfq_partial* mine, std::vector<uint64_t>& hist) {
  const bool want_hist = o.flags & SCFQ_QUAL_HIST;
  scfq_partial_identity(mine, want_hist ? hist.data() : nullptr);
  if (rank != 0) return SCFQ_OK;
  scfq_opts o1 = o;
  o1.n_devices = std::min(o.n_devices, 1);
  return count_file_partial(path, &o1, mine, want_hist ? hist.data() : nullptr);
}

// a collective failed: the comm's text, this rank's own error first
int comm_failed(int local, int rc) {
  std::snprintf(g_err, sizeof g_err, "%s", scfq_comm_error_detail());
  return local ? local : rc;
}

}  // namespace

// fq_count of one file by all ranks of a communicator (include/sc_fqcount.h): shard -> K1/K2 -> exchange -> fold
extern "C" int scfq_count_file_sharded(const char* path, const scfq_opts* opts, scfq_comm* comm, scfq_counts* out) {
  if (!path || !comm || !out || out->struct_size != sizeof(scfq_counts)) return SCFQ_EARG;
  int rc = check_opts(opts);
  if (rc) return rc;
  scfq_opts o = opts_copy(opts);
  o.flags &= ~SCFQ_PREV_IN_MEMORY;
  const bool want_hist = o.flags & SCFQ_QUAL_HIST;
  const int world = scfq_comm_world(comm), rank = scfq_comm_rank(comm);
  std::vector<uint64_t> hist(want_hist ? SCFQ_HIST_WORDS : 0), hist_all(want_hist ? SCFQ_HIST_WORDS : 0);
  scfq_partial mine, all;
  scfq_partial_identity(&mine, want_hist ? hist.data() : nullptr);
  int local = SCFQ_OK;          // a rank that fails still takes part in the exchange (with the identity) so nobody hangs
  InputFile in;
  if (!is_gz_name(path)) {
    in.open(path);
    local = shard_plain(in, rank, world, o, &mine, hist);
  } else {
    static const bool shard_on = env_int("SCFQ_SHARD_BGZF", 1) != 0;
    if (shard_on && world > 1) in.open(path);
    BgzfRange b;
    const uint64_t vote = shard_vote(in, rank, world, &b);
    ShardScheme scheme;
    if (world > 1 && shard_on) {
      // collective 1 (every rank takes part whatever it found: a rank that cannot even open the file says kVoteCannot)
      std::vector<uint64_t> votes((size_t)world, 0);
      if ((rc = scfq_comm_allgather_u64(comm, &vote, 1, votes.data(), 0))) return comm_failed(SCFQ_OK, rc);
      scheme = agree_on_scheme(votes);
    }
    if (scheme.gz) {
      BlockShard blk(comm, rank, world);
      if (scheme.blocks) local = blk.run(in, o, &mine, hist);      // (collective 2 inside)
      else local = shard_gz_members(in, rank, world, o, &mine, hist, &blk.first_byte);
      if (blk.comm_rc) return comm_failed(local, blk.comm_rc);
      in.reset();
      // collective 3: the partials — with each stretch's first byte and whether its members ended exactly where the next rank's begin —
      // are gathered and folded by every rank, in rank order
      const std::vector<uint64_t> row = gz_row(&mine, hist, want_hist, local, blk.first_byte, blk.crc_raw, blk.len);
      std::vector<uint64_t> rows((size_t)world * row.size());
      if ((rc = scfq_comm_allgather_u64(comm, row.data(), (uint32_t)row.size(), rows.data(), 0))) return comm_failed(local, rc);
      bool joined = false;
      if ((rc = gz_fold_rows(rows, world, path, o.flags, scheme.blocks ? &blk : nullptr, &all, hist_all, &joined))) return rc;
      if (joined) return scfq_partial_finalize(&all, want_hist ? hist_all.data() : nullptr, out);
      // every rank knows.  What the block stage said of itself ("did not join up") is no part of the fall-back's text: a damaged file must
      // end with gzread's message alone (tests/test_gpu_inflate_crafted.py::test_sharded_stretch_reference_before_the_member_start)
      g_err[0] = '\0';
      local = rank0_reads_all(path, o, rank, &mine, hist);
    } else if (scheme.bgzf) {
      local = shard_bgzf_members(in, b, rank, o, &mine, hist);
    } else {
      local = rank0_reads_all(path, o, rank, &mine, hist);
    }
  }
  in.reset();
  // collective 4
  if (local) scfq_partial_identity(&mine, want_hist ? hist.data() : nullptr);
  mine.reserved[0] = (uint64_t)(int64_t)local;       // every rank learns whether any rank failed
  if ((rc = scfq_comm_exchange(comm, &mine, want_hist ? hist.data() : nullptr, &all, want_hist ? hist_all.data() : nullptr, 0))) return comm_failed(local, rc);
  if (local) return local;
  if (all.reserved[0]) { std::snprintf(g_err, sizeof g_err, "another rank failed to count its shard"); return SCFQ_EIO; }
  return scfq_partial_finalize(&all, want_hist ? hist_all.data() : nullptr, out);
}

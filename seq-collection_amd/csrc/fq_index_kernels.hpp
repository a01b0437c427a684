// fq_index_kernels.hpp — K5, the line index (record-boundary detection): the kernels behind scfq_index_lines (host side: scfq_index.hpp).
// Included by scfq_api.hip right after fq_scan_kernels.hpp, whose LDS-DMA tile loads, bit-plane classifier and wave scans it uses.
//
// line_off[j] = offset, relative to the first byte of the input, of the first byte of line j.  Lines are what the reference's
// `lines(stream)` yields (src/fq_count.nim:38, src/fq_dedup.nim:42): every '\n' ends one; record i of a FASTQ is lines 4i .. 4i+3.
//
// One pass over the input, in two forms.  Both walk the ranges of K1 (one wave, ~100 consecutive 4 KiB tiles, a 2-slot LDS-DMA ring), keep
// a digest of every tile's newlines and the range's newline count; fq_nl_prefix turns the counts into the ordinal of the first line start
// each range emits; a second kernel walks the DIGESTS, not the input, and writes `position of '\n' + 1` to line_off[ordinal].
//   compact form (the default): fq_index_pos keeps the newline POSITIONS of a tile — 16-bit offsets, packed behind their count, 256 B of
//     scratch per tile — and fq_index_expand_pos writes one coalesced 8-byte store per line.  1.14 x input in bytes for 150 bp reads.
//     fq-dedup rides along: the headers of a tile are hashed while the tile is in LDS (index_hash_lines).
//   mask form (the fall-back): fq_index_masks keeps one bit per input byte (512 B per tile) and fq_index_expand's lanes walk their own
//     bits.  1.34 x input.  A tile with kPosCap or more newlines (lines shorter than 33 bytes on average) does not fit the compact form's
//     slot: fq_index_pos raises a flag and the caller runs this form, which has no such limit; SCFQ_INDEX_COMPACT=0 asks for it outright.
// (The first form of K5 read the input twice, once to count and once to scatter: 2.1 x input in bytes.)
#pragma once
#include "fq_scan_kernels.hpp"

namespace scfq {

// exclusive prefix sum of the per-range newline counts (one block; n_ranges is a few 10^4): first_ord[r] = line_base + 1 +
// number of '\n' in ranges < r  (the first '\n' of range r starts line first_ord[r]); first_ord[n_ranges] = total + line_base + 1
__global__ __launch_bounds__(1024) void fq_nl_prefix(const uint64_t* counts, uint64_t n_ranges, uint64_t line_base, uint64_t* first_ord) {
  __shared__ uint64_t wave_tot[16];
  __shared__ uint64_t carry;
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid == 0) carry = line_base + 1;
  __syncthreads();
  for (uint64_t r0 = 0; r0 < n_ranges; r0 += 1024) {
    const uint64_t r = r0 + tid;
    const uint32_t nl = (r < n_ranges) ? (uint32_t)counts[r] : 0u;   // <= 4096 * kMaxTilesPerRange
    const uint32_t incl = wave_inclusive_scan(nl);
    if (lane == 63) wave_tot[w] = incl;
    __syncthreads();
    uint64_t before = carry;
    for (uint32_t k = 0; k < w; ++k) before += wave_tot[k];
    if (r < n_ranges) first_ord[r] = before + incl - nl;
    __syncthreads();
    if (tid == 1023) carry = before + incl;
    __syncthreads();
  }
  if (tid == 0) first_ord[n_ranges] = carry;
}

// ---- the walk over the input that fq_index_masks and fq_index_pos share ---------------------------------------------------------------
// One wave's range of tiles, as in fq_scan_tiles: tile t covers [A0 + t * 4 KiB, + 4 KiB), A0 the 4 KiB boundary at or below the input's
// first byte; tiles [full_lo, full_hi) lie entirely inside the input [B, E), at most the first and the last tile of an input do not.
// Everything that steers the loop — t_begin, t_end, full_lo, full_hi, the ring's LDS address, hence whole(t) — is wave-uniform and pinned
// in 32-bit SGPRs with readfirstlane (tile indices, not addresses: gfx9 has no ordered 64-bit scalar compare), so that the per-tile
// bookkeeping runs on the scalar unit.  The caller's loop:  if (t_begin < t_end) issue(t_begin, 0);  then per tile  issue(t + 1, slot ^ 1),
// a counted vmcnt wait, index_tile_masks(slot), and for a tile that is not whole(t),  NL &= inside(t).
// (Against private copies in each kernel: the same SGPRs, VGPRs and occupancy, 7 more instructions per kernel — scalar set-up in front of
// the loop and in the edge-tile branch of issue, none on the whole-tile path — and the same wall at 10 GB: profiles/index_refactor/ab.json.)
struct IndexTiles {
  uint64_t B, E, A0;
  uint32_t t_begin, t_end, full_lo, full_hi, ring_lds;
  int lane;

  __device__ __forceinline__ IndexTiles(const uint8_t* base, uint64_t n, uint32_t tiles_per_range, uint64_t range, const uint8_t* ring, int lane_)
      : B((uint64_t)(uintptr_t)base), E(B + n), A0(B & ~(uint64_t)(kTile - 1)), ring_lds((uint32_t)(uintptr_t)ring), lane(lane_) {
    const uint32_t n_tiles = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((E - A0 + kTile - 1) / kTile));
    t_begin = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(range * tiles_per_range));
    uint32_t te = t_begin + tiles_per_range;
    if (te > n_tiles) te = n_tiles;
    t_end = (uint32_t)__builtin_amdgcn_readfirstlane((int)te);
    full_lo = (uint32_t)__builtin_amdgcn_readfirstlane((A0 < B) ? 1 : 0);
    full_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)((A0 + (uint64_t)n_tiles * kTile > E) ? n_tiles - 1 : n_tiles));
  }

  __device__ __forceinline__ bool whole(uint32_t t) const { return t >= full_lo && t < full_hi; }

  // tile t into ring slot `slot`: one whole-tile LDS-DMA, or for an edge tile four pieces, those with no byte of the input redirected
  // to a 16 B piece that is certainly readable
  __device__ __forceinline__ void issue(uint32_t t, uint32_t slot) const {
    const uint64_t ts = A0 + (uint64_t)t * kTile;
    const uint32_t dst = (uint32_t)__builtin_amdgcn_readfirstlane((int)(ring_lds + slot * kTile));
    if (whole(t)) {
      glds_tile<true>(reinterpret_cast<const uint8_t*>(ts + (uint64_t)lane * 16), dst);
    } else {
      const uint64_t safe = (B & ~15ull);
      uint64_t s[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint64_t ps = ts + (uint64_t)k * 1024 + (uint64_t)lane * 16;
        const bool ok = (ps + 16 > B) && (ps < E);
        s[k] = (ok ? ps : safe) - (uint64_t)k * 1024;   // the instruction re-adds offset:k*1024
      }
      glds_tile_edge(reinterpret_cast<const uint8_t*>(s[0]), reinterpret_cast<const uint8_t*>(s[1]),
                     reinterpret_cast<const uint8_t*>(s[2]), reinterpret_cast<const uint8_t*>(s[3]), dst);
    }
  }

  // which of this lane's 64 bytes of tile t lie inside [B, E) (asked of the first / last tile of the input only)
  __device__ __forceinline__ uint64_t inside(uint32_t t) const {
    const uint64_t ts = A0 + (uint64_t)t * kTile;
    const int64_t ls = (int64_t)(ts + (uint64_t)lane * 64);
    int64_t lo = (int64_t)B - ls, hi = (int64_t)E - ls;
    lo = lo < 0 ? 0 : (lo > 64 ? 64 : lo);
    hi = hi < 0 ? 0 : (hi > 64 ? 64 : hi);
    const uint64_t mhi = (hi >= 64) ? ~0ull : ((1ull << hi) - 1);
    const uint64_t mlo = (lo >= 64) ? ~0ull : ((1ull << lo) - 1);
    return mhi & ~mlo;
  }
};

// The loop head of both passes: this lane's 64 bytes of the tile in `slot_bytes` (LDS) -> their newline mask, bit k <=> byte k; with
// want_cr (wave-uniform), cr_seen turns non-zero when a '\r' stands directly before a '\n' inside the 64 bytes or is their last byte
// (conservative: the next byte belongs to another lane).  Bytes of an edge tile outside the input are NOT masked off here.
__device__ __forceinline__ uint64_t index_tile_masks(const uint8_t* slot_bytes, int lane, const PlaneConsts& pc, bool want_cr, uint64_t& cr_seen) {
  const uint4* p = reinterpret_cast<const uint4*>(slot_bytes + lane * 64);
  const uint4 q0 = p[0], q1 = p[1], q2 = p[2], q3 = p[3];
  uint32_t d[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
  uint32_t a0, a1, a2, a3, a4, b0, b1, b2, b3, b4, xa[8], xb[8];
  masks32_planes_x<false>(d, pc, xa, a0, a1, a2, a3, a4);
  masks32_planes_x<false>(d + 8, pc, xb, b0, b1, b2, b3, b4);
  const uint64_t NL = ~((uint64_t)a0 | ((uint64_t)b0 << 32));
  if (want_cr) {
    const uint64_t CR = ~((uint64_t)plane_ne<0x0D>(xa) | ((uint64_t)plane_ne<0x0D>(xb) << 32));
    cr_seen |= ((CR << 1) & NL) | (CR >> 63);
  }
  return NL;
}

// ---- the mask form ---------------------------------------------------------------------------------------------------------------
// (A single kernel with a decoupled look-back over the ranges' counts was built and measured first: with 4096 ranges in flight a range's
// look-back walks 64 dependent steps of 64 predecessors and the kernel ran at 0.33 TB/s; ranges long enough to hide that do not fit their
// masks into registers.)
struct IndexMaskArgs {
  const uint8_t* base;        // first byte of the input (any alignment)
  uint64_t n;                 // bytes
  uint32_t tiles_per_range;
  uint64_t n_ranges;
  uint64_t* masks;            // [n_tiles][64]: newline mask of lane L's 64 bytes of tile t at masks[t * 64 + L]
  uint64_t* counts;           // [n_ranges]
  uint32_t* flags_out;        // optional: bit 0 is set when the input may hold a '\r' directly before a '\n' (conservative: a '\r' in
                              // the last byte of a lane's 64 counts); fq-dedup skips its "\r\n" look-behind reads when it stays clear
};

__global__ __launch_bounds__(64 * kWavesPerBlock) void fq_index_masks(IndexMaskArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int lane = threadIdx.x & 63;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint8_t* ring = smem + wave * (2 * kTile);
  const uint64_t range = (uint64_t)blockIdx.x * kWavesPerBlock + wave;
  if (range >= a.n_ranges) return;
  const IndexTiles w(a.base, a.n, a.tiles_per_range, range, ring, lane);
  const bool want_cr = (bool)__builtin_amdgcn_readfirstlane(a.flags_out != nullptr ? 1 : 0);
  PlaneConsts pc;
  pc.init();

  uint64_t cr_seen = 0;
  uint32_t cnt = 0;                                 // per lane; 64 per tile at most, kMaxTilesPerRange tiles
  if (w.t_begin < w.t_end) w.issue(w.t_begin, 0);
  uint32_t slot = 0;
  for (uint32_t t = w.t_begin; t < w.t_end; ++t) {
    if (t + 1 < w.t_end) { w.issue(t + 1, slot ^ 1u); wait_vmcnt<4>(); } else { wait_vmcnt<0>(); }
    uint64_t NL = index_tile_masks(ring + slot * kTile, lane, pc, want_cr, cr_seen);
    if (!w.whole(t)) NL &= w.inside(t);
    __builtin_nontemporal_store(NL, &a.masks[(uint64_t)t * 64 + lane]);
    cnt += popc64(NL);
    slot ^= 1u;
  }
  const uint32_t total = wave_sum(cnt);
  if (lane == 0) a.counts[range] = total;
  // (a look before the atomic: on a "\r\n" input EVERY wave would otherwise queue one on the same word)
  if (want_cr && __builtin_amdgcn_ballot_w64(cr_seen != 0) != 0 && lane == 0 &&
      !(__hip_atomic_load(a.flags_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 1u))
    atomicOr(a.flags_out, 1u);
}

constexpr int kExpandWaves = 4;      // waves (= ranges) per block of fq_index_expand and fq_index_expand_pos

struct IndexExpandArgs {
  const uint64_t* masks;      // fq_index_masks
  uint64_t lead;              // bytes between the first tile's start and the input's first byte (B - A0)
  uint32_t n_tiles;
  uint32_t tiles_per_range;
  uint64_t n_ranges;
  const uint64_t* first_ord;  // fq_nl_prefix over the ranges' counts
  uint64_t* line_off;         // [cap]
  uint64_t cap;
  uint64_t off_base;          // offset of the input's first byte in the whole input (streaming chunks)
};

// one wave per range again, tile by tile over the masks: wave prefix sum of the per-lane counts + a running ordinal
__global__ __launch_bounds__(64 * kExpandWaves) void fq_index_expand(IndexExpandArgs a) {
  const int lane = threadIdx.x & 63;
  const uint64_t range = (uint64_t)blockIdx.x * kExpandWaves + (threadIdx.x >> 6);
  if (range >= a.n_ranges) return;
  const uint32_t t_begin = (uint32_t)(range * a.tiles_per_range);
  uint32_t t_end = t_begin + a.tiles_per_range;
  if (t_end > a.n_tiles) t_end = a.n_tiles;
  uint64_t ord = a.first_ord[range];
  // the masks of the next tile are requested before this tile's offsets are written
  uint64_t x = t_begin < t_end ? __builtin_nontemporal_load(&a.masks[(uint64_t)t_begin * 64 + lane]) : 0;
  for (uint32_t t = t_begin; t < t_end; ++t) {
    const uint64_t nx = t + 1 < t_end ? __builtin_nontemporal_load(&a.masks[(uint64_t)(t + 1) * 64 + lane]) : 0;
    const uint32_t cnt = popc64(x);
    const uint32_t incl = wave_inclusive_scan(cnt);
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    if (total) {      // wave-uniform
      uint64_t o = ord + (incl - cnt);
      const uint64_t lane_off = a.off_base + ((uint64_t)t * kTile + (uint64_t)lane * 64 - a.lead) + 1;   // offset of the byte AFTER bit 0 of this lane
      while (x) {
        const uint32_t k = (uint32_t)__builtin_ctzll(x);
        x &= x - 1;
        if (o < a.cap) a.line_off[o] = lane_off + k;
        ++o;
      }
    }
    ord += total;
    x = nx;
  }
}

// ---- the compact form ------------------------------------------------------------------------------------------------------------
// ~2 x 46 bytes of positions per 4 KiB tile of 150 bp FASTQ where the masks are 512.
constexpr uint32_t kPosCap = 128;     // uint16 entries per tile: [0] the count, [1 ..] the positions
constexpr uint32_t kPosHashCap = 32;  // hashed lines per tile (fq-dedup): a tile of 150 bp FASTQ holds 11 or 12 headers
constexpr uint32_t kPosStage = 2 * kPosCap + 4 * kPosHashCap + 8 * kPosHashCap;      // a wave's staging: the slot, the (start, length) list, the hashes
constexpr uint32_t kIndexPosLds = kWavesPerBlock * (2 * kTile + kPosStage);      // fq_index_pos: the waves' tile rings + their staging areas

// fq-dedup rides along (IndexPosArgs::hash_at): the lines of this tile that start with '@', begin behind one of its newlines and end at
// the next are hashed HERE, where their bytes are in LDS — lane j looks at the line behind newline j (entries j and j + 1 of the staged
// positions); the lines found are listed, and four lanes take a line each round, every fourth 8-byte word per lane, summed over the four
// with two cross-lane steps: the hash is a sum over words (scfq_hdrhash.hpp).
// The hash kernel of fq-dedup read 1.4 lines of 128 bytes per 57-byte header — 4 - 5 GB for 10 GB of input — to do the same.
__device__ __forceinline__ void index_hash_lines(const uint8_t* tile, uint16_t* stage, uint32_t* hl, uint64_t* hout, uint32_t total, int lane,
                                                 uint64_t* out) {
  const uint32_t j = (uint32_t)lane;
  bool cand = j >= 1u && j + 1u <= total;
  uint32_t S = 0, len = 0;
  if (cand) {
    const uint32_t p0 = stage[j], p1 = stage[j + 1u];
    S = p0 + 1u;
    uint32_t e = p1;
    if (S < e && tile[e - 1u] == '\r') --e;       // (Nim's readLine: "\r\n" ends a line as "\n" does)
    len = e - S;
    cand = S < p1 && tile[S] == '@' && len <= scfq_hdrhash::kMaxLen;
  }
  const uint64_t hmask = __builtin_amdgcn_ballot_w64(cand);
  if (hmask == 0) return;
  const uint32_t rank = (uint32_t)__builtin_popcountll(hmask & ((1ull << lane) - 1ull));
  cand = cand && rank < kPosHashCap;
  if (cand) { hl[rank] = S | len << 16; stage[j] = (uint16_t)(stage[j] | 0x8000u); }
  uint32_t n_h = (uint32_t)__builtin_popcountll(hmask);
  if (n_h > kPosHashCap) n_h = kPosHashCap;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  const uint32_t k0 = (uint32_t)lane & 3u;
  for (uint32_t r0 = 0; r0 < n_h; r0 += 16u) {      // wave-uniform: sixteen lines a round, four lanes each (words k0, k0 + 4, ...)
    const uint32_t hh = r0 + ((uint32_t)lane >> 2);
    uint32_t A = 0, B = 0, ln = 0;
    if (hh < n_h) {
      const uint32_t v = hl[hh];
      const uint32_t Sl = v & 0xFFFFu;
      ln = v >> 16;
      const uint32_t n_words = (ln + 7u) >> 3;
      for (uint32_t kk = k0; kk < n_words; kk += 4u) {
        // the word's eight bytes from LDS: three aligned dwords and two byte alignments (the line starts anywhere)
        const uint32_t at = Sl + 8u * kk;
        const uint32_t* q = reinterpret_cast<const uint32_t*>(tile + (at & ~3u));
        const uint32_t d0 = q[0], d1 = q[1], d2 = q[2];      // (may reach past the tile's end: still this workgroup's LDS, masked below)
        const uint32_t sh = at & 3u;
        uint32_t lo = __builtin_amdgcn_alignbyte(d1, d0, sh), hi = __builtin_amdgcn_alignbyte(d2, d1, sh);
        const uint32_t valid = ln - 8u * kk;                 // >= 1
        if (valid < 4u) { lo &= (1u << (8u * valid)) - 1u; hi = 0; }
        else if (valid == 4u) hi = 0;
        else if (valid < 8u) hi &= (1u << (8u * (valid - 4u))) - 1u;
        scfq_hdrhash::hh_word(lo, hi, kk, A, B);
      }
    }
    // the four lanes of a line add up (DPP quad permutes: the neighbour in the pair, then the other pair); the mixing of the sums is
    // left to the kernel that hands the keys out (fq_index_expand_pos: one lane per header there)
    A += (uint32_t)__builtin_amdgcn_mov_dpp((int)A, 0xB1, 0xF, 0xF, true); B += (uint32_t)__builtin_amdgcn_mov_dpp((int)B, 0xB1, 0xF, 0xF, true);
    A += (uint32_t)__builtin_amdgcn_mov_dpp((int)A, 0x4E, 0xF, 0xF, true); B += (uint32_t)__builtin_amdgcn_mov_dpp((int)B, 0x4E, 0xF, 0xF, true);
    if (hh < n_h && k0 == 0u) hout[hh] = (uint64_t)A | (uint64_t)(B & 0xFFFFFFu) << 32 | (uint64_t)ln << scfq_hdrhash::kHashBits;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if ((uint32_t)lane < n_h) out[lane] = hout[lane];
  asm volatile("" ::: "memory");
}

struct IndexPosArgs {
  const uint8_t* base;        // first byte of the input (any alignment)
  uint64_t n;                 // bytes
  uint32_t tiles_per_range;
  uint64_t n_ranges;
  uint16_t* pos;              // [n_tiles][kPosCap]
  uint64_t* counts;           // [n_ranges]
  uint32_t* flags;            // bit 0: the input may hold a '\r' directly before a '\n' (as fq_index_masks; only when want_cr); bit 1: a tile overflowed
  uint32_t want_cr;
  // fq-dedup (optional): the hashes of the lines that start with '@' and lie inside ONE tile (start behind a newline of the tile, end
  // at the next one, at most 255 bytes), in tile order, at most kPosHashCap per tile: [n_tiles][kPosHashCap] of A | (B & 2^24 - 1) << 32 |
  // length << 56 (scfq_hdrhash.hpp: the sums over the line's words); the entry of the newline in front of such a line carries bit 15
  uint64_t* hash_at;
  uint64_t hash_seed;
};

__global__ __launch_bounds__(64 * kWavesPerBlock) void fq_index_pos(IndexPosArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int lane = threadIdx.x & 63;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint8_t* ring = smem + wave * (2 * kTile);
  uint16_t* stage = reinterpret_cast<uint16_t*>(smem + kWavesPerBlock * (2 * kTile) + wave * kPosStage);      // (launch: kIndexPosLds bytes)
  uint32_t* hl = reinterpret_cast<uint32_t*>(stage + kPosCap);                 // fq-dedup: (start | length << 16) of the lines to hash
  uint64_t* hout = reinterpret_cast<uint64_t*>(hl + kPosHashCap);              // ... and their hashes
  const bool want_hash = (bool)__builtin_amdgcn_readfirstlane(a.hash_at != nullptr ? 1 : 0);
  const uint64_t range = (uint64_t)blockIdx.x * kWavesPerBlock + wave;
  if (range >= a.n_ranges) return;
  const IndexTiles w(a.base, a.n, a.tiles_per_range, range, ring, lane);
  const bool want_cr = (bool)__builtin_amdgcn_readfirstlane((int)a.want_cr);
  PlaneConsts pc;
  pc.init();

  uint64_t cr_seen = 0;
  uint32_t range_total = 0;                         // wave-uniform
  bool overflow = false;                            // wave-uniform
  if (w.t_begin < w.t_end) w.issue(w.t_begin, 0);
  uint32_t slot = 0;
  for (uint32_t t = w.t_begin; t < w.t_end; ++t) {
    if (t + 1 < w.t_end) { w.issue(t + 1, slot ^ 1u); wait_vmcnt<4>(); } else { wait_vmcnt<0>(); }
    uint64_t NL = index_tile_masks(ring + slot * kTile, lane, pc, want_cr, cr_seen);
    if (!w.whole(t)) NL &= w.inside(t);
    const uint32_t cnt = popc64(NL);
    const uint32_t incl = wave_inclusive_scan(cnt);
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    uint32_t* out = reinterpret_cast<uint32_t*>(a.pos + (uint64_t)t * kPosCap);      // (256-byte aligned: a slot is 128 x 2 bytes)
    if (total < kPosCap) {                    // wave-uniform
      // the lanes put their positions into the wave's 256 bytes of LDS, in order, and the wave stores the slot's used part as whole
      // dwords, coalesced (stored straight from the lanes — 2-byte stores to scattered entries, three store instructions per tile —
      // the kernel was SLOWER than the mask form, 2.03 against 1.90 ms, with a third of its writes)
      if (lane == 0) stage[0] = (uint16_t)total;
      uint32_t o = incl - cnt + 1u;
      uint64_t x = NL;
      while (__builtin_amdgcn_ballot_w64(x != 0) != 0) {      // as many rounds as the fullest lane holds newlines (two or three for FASTQ)
        if (x) {
          stage[o++] = (uint16_t)((uint32_t)lane * 64u + (uint32_t)__builtin_ctzll(x));
          x &= x - 1;
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // (one wave: its LDS operations complete in order; nothing is read before they have)
      if (want_hash && total >= 2u) index_hash_lines(ring + slot * kTile, stage, hl, hout, total, lane, a.hash_at + (uint64_t)t * kPosHashCap);
      if ((uint32_t)lane < (total + 2u) / 2u) __builtin_nontemporal_store(reinterpret_cast<const uint32_t*>(stage)[lane], &out[lane]);
      asm volatile("" ::: "memory");
    } else {
      overflow = true;
      if (lane == 0) out[0] = 0xFFFFu;
    }
    range_total += total;
    slot ^= 1u;
  }
  if (lane == 0) a.counts[range] = range_total;
  // (a look before each atomic: on a "\r\n" input EVERY wave would otherwise queue one on the same word)
  uint32_t bits = (want_cr && __builtin_amdgcn_ballot_w64(cr_seen != 0) != 0) ? 1u : 0u;
  if (overflow) bits |= 2u;
  if (bits && lane == 0 && (__hip_atomic_load(a.flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bits) != bits) atomicOr(a.flags, bits);
}

struct IndexExpandPosArgs {
  const uint16_t* pos;        // fq_index_pos
  const uint32_t* flags;      // ... bit 1: some tile overflowed, nothing is written here (the caller runs the mask form)
  uint64_t lead;              // bytes between the first tile's start and the input's first byte (B - A0)
  uint32_t n_tiles;
  uint32_t tiles_per_range;
  uint64_t n_ranges;
  const uint64_t* first_ord;  // fq_nl_prefix over the ranges' counts
  uint64_t* line_off;         // [cap]
  uint64_t cap;
  uint64_t off_base;
  // fq-dedup (optional; hash_at as written by fq_index_pos): line 4r is record r's header — its key (the hash's low hash_bits, or all
  // ones = "not hashed by the index pass": dd_hash_headers does those), its number, and its (start | length << 40)
  const uint64_t* hash_at;
  void* keys;                 // uint32_t[cap_records] (key_bytes == 4) or uint64_t[cap_records]
  uint32_t* idx;
  uint64_t* hdr;
  uint64_t cap_records;
  uint32_t key_bytes;
  uint32_t hash_bits;
  uint64_t hash_seed;
  uint32_t* unk;              // [n_tiles][kPosUnk]: the records of the tile that got the all-ones key (0: none) ...
  uint32_t* flags_rw;         // ... bit 2 of the index's flag word: a tile had more of them, or 64+ newlines: the list is not complete
};
constexpr uint32_t kPosUnk = 4;

__device__ __forceinline__ void index_put_record(const IndexExpandPosArgs& a, uint64_t r, uint64_t start, bool hashed, uint64_t stored) {
  if (r >= a.cap_records) return;
  const uint64_t len = hashed ? stored >> scfq_hdrhash::kHashBits : 0xFFFFFFull;      // (saturated: looked up again through the line index)
  const uint64_t h = scfq_hdrhash::hh_final((uint32_t)stored, (uint32_t)(stored >> 32) & 0xFFFFFFu, len, a.hash_seed);
  const uint64_t key = hashed ? (a.hash_bits < 64 ? h & ((1ull << a.hash_bits) - 1ull) : h) : ~0ull;
  if (a.key_bytes == 4) static_cast<uint32_t*>(a.keys)[r] = (uint32_t)key; else static_cast<uint64_t*>(a.keys)[r] = key;
  a.idx[r] = (uint32_t)r;
  a.hdr[r] = start | len << 40;
}

// one wave per range, tile by tile: lane j holds entries j and 64 + j of the tile (entry 0 is the count), entry j is line ord + j - 1
__global__ __launch_bounds__(64 * kExpandWaves) void fq_index_expand_pos(IndexExpandPosArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t range = (uint64_t)blockIdx.x * kExpandWaves + (threadIdx.x >> 6);
  if (range >= a.n_ranges) return;
  if (*a.flags & 2u) return;
  const uint32_t t_begin = (uint32_t)(range * a.tiles_per_range);
  uint32_t t_end = t_begin + a.tiles_per_range;
  if (t_end > a.n_tiles) t_end = a.n_tiles;
  uint64_t ord = a.first_ord[range];
  static_assert(kPosCap == 128, "two entries per lane");
  const uint16_t* s = a.pos + (uint64_t)t_begin * kPosCap;
  // (the first half of the next tile's entries is requested before this tile's offsets are written; the second half only by a tile
  // that has that many: 46 newlines per tile in 150 bp FASTQ)
  uint32_t v0 = t_begin < t_end ? s[lane] : 0u;
  // (fq-dedup: the tile's hashes come with its entries — lane l holds hash l & 31 — so that no load waits for a rank)
  const uint64_t* hs = a.keys ? a.hash_at + (uint64_t)t_begin * kPosHashCap : nullptr;
  uint64_t h0 = (hs && t_begin < t_end) ? hs[lane & 31u] : 0;
  bool unk_over = false;      // wave-uniform
  for (uint32_t t = t_begin; t < t_end; ++t) {
    const uint16_t* cur = s;
    s += kPosCap;
    const uint32_t n0 = t + 1 < t_end ? s[lane] : 0u;
    uint64_t hn = 0;
    if (hs) { hs += kPosHashCap; if (t + 1 < t_end) hn = hs[lane & 31u]; }
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)v0, 0);
    const uint64_t tile_off = a.off_base + ((uint64_t)t * kTile - a.lead) + 1;      // offset of the byte AFTER the tile's byte 0
    const bool mine = lane >= 1u && lane <= total;
    const uint32_t pos = v0 & 0x7FFFu;                                              // (bit 15: the line behind this newline was hashed)
    if (mine) { const uint64_t o = ord + lane - 1u; if (o < a.cap) a.line_off[o] = tile_off + pos; }
    if (a.keys) {      // kernel-uniform
      const bool hashed = mine && (v0 & 0x8000u);
      const uint64_t hm = __builtin_amdgcn_ballot_w64(hashed);
      const uint32_t rank = (uint32_t)__builtin_popcountll(hm & ((1ull << lane) - 1ull)) & 31u;
      const uint64_t stored = (uint64_t)(uint32_t)__shfl((int)(uint32_t)h0, (int)rank, 64) | (uint64_t)(uint32_t)__shfl((int)(uint32_t)(h0 >> 32), (int)rank, 64) << 32;
      const uint64_t o = ord + lane - 1u;
      const bool head = mine && (o & 3u) == 0;
      if (head) index_put_record(a, o >> 2, tile_off + pos, hashed, stored);
      if (a.unk) {
        const bool un = head && !hashed;
        const uint64_t um = __builtin_amdgcn_ballot_w64(un);
        const uint32_t n_un = (uint32_t)__builtin_popcountll(um);
        uint32_t* u = a.unk + (uint64_t)t * kPosUnk;
        if (un) { const uint32_t ur = (uint32_t)__builtin_popcountll(um & ((1ull << lane) - 1ull)); if (ur < kPosUnk) u[ur] = (uint32_t)(o >> 2); }
        if (lane < kPosUnk && lane >= n_un) u[lane] = 0u;
        if (n_un > kPosUnk || total >= 64u) unk_over = true;
      }
    }
    if (total >= 64u) {      // wave-uniform
      const uint32_t v1 = cur[64 + lane] & 0x7FFFu;
      if (64u + lane <= total) {
        const uint64_t o = ord + 63u + lane;
        if (o < a.cap) a.line_off[o] = tile_off + v1;
        if (a.keys && (o & 3u) == 0) index_put_record(a, o >> 2, tile_off + v1, false, 0);
      }
    }
    ord += total;
    v0 = n0;
    h0 = hn;
  }
  if (unk_over && lane == 0u && !(__hip_atomic_load(a.flags_rw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 4u)) atomicOr(a.flags_rw, 4u);
}

}  // namespace scfq

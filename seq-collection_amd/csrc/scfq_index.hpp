// scfq_index.hpp — K5, the line index of a device-resident input: the host side of scfq_index_lines (include/sc_fqcount.h) and of
// scfq_index_lines_ex2 (scfq_index_aux.hpp: what fq-dedup, fq-readstats, fq-cycles and fq-kmers reach through scfq_scratch::build_line_index).
// Included by scfq_api.hip, whose Session, Ctx, HIPCHK, g_err, trace, env_int, pick_tiles_per_range and wait_for_caller it uses; the kernels
// are fq_index_kernels.hpp.
//
// The compact form runs first (fq_index_pos, fq_nl_prefix, fq_index_expand_pos) and its one question to the device — did every tile fit its
// slot? — comes back together with the line count, the input's last byte and the flag word: one wait.  Only a file of very short lines (or
// SCFQ_INDEX_COMPACT=0) runs the mask form (fq_index_masks, fq_nl_prefix, fq_index_expand) and pays a second pass and a second wait.
// Everything is enqueued on c->compute; the scratch is one grow-only allocation (Ctx::d_first_ord) laid out anew by every form.
#pragma once

namespace {

// The tiles and ranges of a call (the ranges of K1: pick_tiles_per_range) and what the caller asked for.
struct IndexCall {
  Ctx* c;
  const uint8_t* base;
  uint64_t n;             // > 0
  uint64_t* d_line_off;
  uint64_t cap;
  bool write;             // line_off is wanted and has room for line 0 at least
  bool want_cr;           // the caller wants flag bit 0
  scfq_index_aux* aux;
  uint64_t lead;          // bytes between the first tile's start and the input's first byte
  uint64_t n_tiles;
  uint32_t tpr;
  uint64_t n_ranges;
  unsigned grid(unsigned waves_per_block) const { return (unsigned)((n_ranges + waves_per_block - 1) / waves_per_block); }
};

int index_geometry(IndexCall* k) {
  const uint64_t B = (uint64_t)(uintptr_t)k->base, A0 = B & ~(uint64_t)(scfq::kTile - 1);
  k->lead = B - A0;
  k->n_tiles = (B + k->n - A0 + scfq::kTile - 1) / scfq::kTile;
  if (k->n_tiles >= (1ull << 32)) { std::snprintf(g_err, sizeof g_err, "a single index launch covers at most 16 TiB"); return SCFQ_EARG; }
  k->tpr = pick_tiles_per_range(k->c, k->n_tiles);
  k->n_ranges = (k->n_tiles + k->tpr - 1) / k->tpr;
  return SCFQ_OK;
}

// scratch of one form: [n_tiles * per_tile] positions (+ hashes) or masks | [n_ranges] counts | [n_ranges + 1] first ordinals | flags
struct IndexScratch {
  uint64_t* tiles = nullptr;
  uint64_t* counts = nullptr;
  uint64_t* ord = nullptr;
  uint32_t* flags = nullptr;      // bit 0: "\r\n" possible; bit 1: a tile overflowed its compact slot; bit 2: aux->unk is not complete
};

int index_scratch(const IndexCall& k, uint64_t per_tile, IndexScratch* s) {
  Ctx* c = k.c;
  const uint64_t words = k.n_tiles * per_tile + 2 * k.n_ranges + 8;
  if (words > c->cap_first_ord) {
    HIPCHK(hipStreamSynchronize(c->compute));
    if (c->d_first_ord) HIPCHK(hipFree(c->d_first_ord));
    c->d_first_ord = nullptr;
    c->cap_first_ord = 0;
    const uint64_t want = words + words / 8;
    HIPCHK(hipMalloc(&c->d_first_ord, want * sizeof(uint64_t)));
    c->cap_first_ord = want;
  }
  s->tiles = c->d_first_ord;
  s->counts = s->tiles + k.n_tiles * per_tile;
  s->ord = s->counts + k.n_ranges;
  s->flags = reinterpret_cast<uint32_t*>(s->ord + k.n_ranges + 1);
  return SCFQ_OK;
}

// what both forms enqueue in front of their first kernel ...
int index_begin(const IndexCall& k, uint64_t per_tile, IndexScratch* s) {
  const int rc = index_scratch(k, per_tile, s);
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(s->flags, 0, 8, k.c->compute));
  if (k.write) HIPCHK(hipMemsetAsync(k.d_line_off, 0, sizeof(uint64_t), k.c->compute));          // line 0 starts at offset 0
  return SCFQ_OK;
}

// ... and between their two kernels: ord[r] = 1 + number of '\n' in ranges < r, ord[n_ranges] = 1 + number of '\n'
int index_prefix(const IndexCall& k, const IndexScratch& s) {
  hipLaunchKernelGGL(scfq::fq_nl_prefix, dim3(1), dim3(1024), 0, k.c->compute, s.counts, k.n_ranges, (uint64_t)0, s.ord);
  HIPCHK(hipGetLastError());
  return SCFQ_OK;
}

// The compact form: 16-bit newline positions per tile, 256 B of scratch per tile; with aux, the headers' hashes behind the position slots.
int run_compact(const IndexCall& k, IndexScratch* s) {
  Ctx* c = k.c;
  const scfq_index_aux* aux = k.aux;
  const bool with_hash = aux && k.write;
  int rc = index_begin(k, scfq::kPosCap / 4 + (with_hash ? scfq::kPosHashCap : 0), s);
  if (rc) return rc;
  uint64_t* hash_at = with_hash ? s->tiles + k.n_tiles * (scfq::kPosCap / 4) : nullptr;
  scfq::IndexPosArgs pa{};
  pa.hash_at = hash_at;
  pa.hash_seed = aux ? aux->seed : 0;
  pa.base = k.base;
  pa.n = k.n;
  pa.tiles_per_range = k.tpr;
  pa.n_ranges = k.n_ranges;
  pa.pos = reinterpret_cast<uint16_t*>(s->tiles);
  pa.counts = s->counts;
  pa.flags = s->flags;
  pa.want_cr = k.want_cr ? 1u : 0u;
  hipLaunchKernelGGL(scfq::fq_index_pos, dim3(k.grid(scfq::kWavesPerBlock)), dim3(64 * scfq::kWavesPerBlock), scfq::kIndexPosLds, c->compute, pa);
  HIPCHK(hipGetLastError());
  if ((rc = index_prefix(k, *s))) return rc;
  if (!k.write) return SCFQ_OK;
  scfq::IndexExpandPosArgs ea{};
  if (with_hash) {
    ea.hash_at = hash_at;
    ea.keys = aux->keys; ea.idx = aux->idx; ea.hdr = aux->hdr;
    ea.cap_records = aux->cap_records; ea.key_bytes = aux->key_bytes; ea.hash_bits = aux->hash_bits; ea.hash_seed = aux->seed;
    ea.unk = (aux->unk && aux->unk_tiles >= k.n_tiles) ? aux->unk : nullptr;
    ea.flags_rw = s->flags;
  }
  ea.pos = reinterpret_cast<const uint16_t*>(s->tiles);
  ea.flags = s->flags;
  ea.lead = k.lead;
  ea.n_tiles = (uint32_t)k.n_tiles;
  ea.tiles_per_range = k.tpr;
  ea.n_ranges = k.n_ranges;
  ea.first_ord = s->ord;
  ea.line_off = k.d_line_off;
  ea.cap = k.cap;
  ea.off_base = 0;
  hipLaunchKernelGGL(scfq::fq_index_expand_pos, dim3(k.grid(scfq::kExpandWaves)), dim3(64 * scfq::kExpandWaves), 0, c->compute, ea);
  HIPCHK(hipGetLastError());
  return SCFQ_OK;
}

// The mask form: a bit per byte, 512 B of scratch per tile; no limit on the newlines of a tile, no hashes.
int run_masks(const IndexCall& k, IndexScratch* s) {
  Ctx* c = k.c;
  int rc = index_begin(k, 64, s);
  if (rc) return rc;
  scfq::IndexMaskArgs ma;
  ma.base = k.base;
  ma.n = k.n;
  ma.tiles_per_range = k.tpr;
  ma.n_ranges = k.n_ranges;
  ma.masks = s->tiles;
  ma.counts = s->counts;
  ma.flags_out = k.want_cr ? s->flags : nullptr;
  hipLaunchKernelGGL(scfq::fq_index_masks, dim3(k.grid(scfq::kWavesPerBlock)), dim3(64 * scfq::kWavesPerBlock), scfq::kWavesPerBlock * 2 * scfq::kTile, c->compute, ma);
  HIPCHK(hipGetLastError());
  if ((rc = index_prefix(k, *s))) return rc;
  if (!k.write) return SCFQ_OK;
  scfq::IndexExpandArgs ea;
  ea.masks = s->tiles;
  ea.lead = k.lead;
  ea.n_tiles = (uint32_t)k.n_tiles;
  ea.tiles_per_range = k.tpr;
  ea.n_ranges = k.n_ranges;
  ea.first_ord = s->ord;
  ea.line_off = k.d_line_off;
  ea.cap = k.cap;
  ea.off_base = 0;
  hipLaunchKernelGGL(scfq::fq_index_expand, dim3(k.grid(scfq::kExpandWaves)), dim3(64 * scfq::kExpandWaves), 0, c->compute, ea);
  HIPCHK(hipGetLastError());
  return SCFQ_OK;
}

// The wait of a form: h_state[0] = 1 + number of '\n', h_state[1] = the input's last byte, h_state[2] = the flag word.
int index_read_back(const IndexCall& k, const IndexScratch& s) {
  Ctx* c = k.c;
  HIPCHK(hipMemcpyAsync(c->h_state + 2, s.flags, 4, hipMemcpyDeviceToHost, c->compute));
  HIPCHK(hipMemcpyAsync(c->h_state, s.ord + k.n_ranges, sizeof(uint64_t), hipMemcpyDeviceToHost, c->compute));
  HIPCHK(hipMemcpyAsync(c->h_state + 1, k.base + k.n - 1, 1, hipMemcpyDeviceToHost, c->compute));
  HIPCHK(hipStreamSynchronize(c->compute));
  return SCFQ_OK;
}

int index_lines(Ctx* c, const uint8_t* base, uint64_t n, uint64_t* d_line_off, uint64_t cap, uint64_t* lines_out, uint32_t* flags_out, scfq_index_aux* aux) {
  IndexCall k{};
  k.c = c; k.base = base; k.n = n; k.d_line_off = d_line_off; k.cap = cap; k.aux = aux;
  k.write = d_line_off && cap >= 1;
  k.want_cr = flags_out != nullptr;
  int rc = index_geometry(&k);
  if (rc) return rc;
  static const bool compact_on = env_int("SCFQ_INDEX_COMPACT", 1) != 0;
  IndexScratch s;
  bool done = false;
  if (compact_on) {
    if ((rc = run_compact(k, &s)) || (rc = index_read_back(k, s))) return rc;
    done = !(c->h_state[2] & 2u);
    if (done && aux && k.write) {
      aux->filled = 1;
      aux->n_tiles = k.n_tiles;
      aux->unk_complete = (aux->unk && aux->unk_tiles >= k.n_tiles && !(c->h_state[2] & 4u)) ? 1 : 0;
    }
    if (!done) trace("line index: a tile with more newlines than the compact form's slot holds, the mask form runs");
  }
  if (!done && ((rc = run_masks(k, &s)) || (rc = index_read_back(k, s)))) return rc;
  if (flags_out) *flags_out = (uint32_t)(c->h_state[2] & 1u);
  const uint64_t nl = c->h_state[0] - 1;
  const bool open_end = (uint8_t)(c->h_state[1] & 0xFF) != (uint8_t)'\n';
  const uint64_t lines = nl + (open_end ? 1u : 0u);
  *lines_out = lines;
  if (k.write && cap >= lines + 1 && open_end) {
    // the final line has no '\n': the sentinel pretends there is one right after the input
    c->h_state[0] = n + 1;
    HIPCHK(hipMemcpyAsync(d_line_off + lines, c->h_state, sizeof(uint64_t), hipMemcpyHostToDevice, c->compute));
    HIPCHK(hipStreamSynchronize(c->compute));
  }
  return SCFQ_OK;
}

}  // namespace

extern "C" {

int scfq_index_lines_ex2(const void* dptr, uint64_t n, uint64_t* d_line_off, uint64_t cap, uint64_t* lines_out, uint32_t* flags_out, scfq_index_aux* aux) {
  if ((!dptr && n) || !lines_out) return SCFQ_EARG;
  if (aux) { aux->filled = 0; aux->unk_complete = 0; aux->n_tiles = 0; }
  if (aux && (!aux->keys || !aux->idx || !aux->hdr || (aux->key_bytes != 4 && aux->key_bytes != 8) || aux->hash_bits > 56 || !d_line_off)) return SCFQ_EARG;
  if (flags_out) *flags_out = 1u;            // unknown until the index pass says otherwise
  Session s;
  int rc = s.open(true);
  Ctx* c = s.c;
  if (rc) return rc;
  if ((rc = wait_for_caller(c, nullptr))) return rc;      // input and line_off are the caller's device buffers
  *lines_out = 0;
  if (n == 0) {
    if (flags_out) *flags_out = 0;
    if (d_line_off && cap >= 1) { HIPCHK(hipMemsetAsync(d_line_off, 0, sizeof(uint64_t), c->compute)); HIPCHK(hipStreamSynchronize(c->compute)); }
    return SCFQ_OK;
  }
  return index_lines(c, static_cast<const uint8_t*>(dptr), n, d_line_off, cap, lines_out, flags_out, aux);
}

int scfq_index_lines(const void* dptr, uint64_t n, uint64_t* d_line_off, uint64_t cap, uint64_t* lines_out) {
  return scfq_index_lines_ex2(dptr, n, d_line_off, cap, lines_out, nullptr, nullptr);
}

}  // extern "C"

"""fq-kcount, fq-normalize and fq-demux on device-resident inputs whose offsets pass 2^32, against their checkers: the layout, the
composition laws and the inputs are tests/_big_offset_cases.py's, proven without a GPU in tests/test_big_offset_cases_host.py; the
device-side comparison (Big, Room, assert_tiled, check_outputs) is tests/test_gpu_big_offsets.py's.  Every comparison is ==.

What a narrowed offset, a 32-bit group sum or a unit number cut to 32 bits looks like is said in every test's docstring.  The k-mer
tables always get table_bits: automatic sizing would take 2^30 slots for inputs of this size."""
import os

import numpy as np
import pytest

import _big_offset_cases as C
import test_gpu_big_offsets as G
from conftest import GOLDEN
from _demux_check import assert_stats as assert_demux
from _kcount_check import CANONICAL, assert_summary as assert_kcount, canonical_key, dump_of, hist_of
from _kmers_check import revcomp_index
from _normalize_check import assert_stats as assert_norm
from _screen_check import contigs_of

pytestmark = pytest.mark.gpu

Big, Room, assert_tiled, packed_tiled, check_outputs, where = G.Big, G.Room, G.assert_tiled, G.packed_tiled, G.check_outputs, G.where
NORM_REC = np.dtype([("kmers", "<u4"), ("depth", "<u4"), ("min_count", "<u4"), ("weak", "<u4")])
DEMUX_REC = np.dtype([("sample", "<u2"), ("mm1", "u1"), ("mm2", "u1"), ("state", "u1"), ("reserved", "u1", (3,))])
K, BINS = 21, 1002


@pytest.fixture(autouse=True)
def pool_memory(scfq, gpu):
    before = scfq.lib().scfq_device_bytes_now()
    yield
    gpu.cuda.empty_cache()
    assert scfq.lib().scfq_device_bytes_now() == before
    assert gpu.cuda.max_memory_allocated() < 36e9, "inputs and outputs of the tests stay below 36 GB, which leaves 4 GB for the library's own"


@pytest.fixture(scope="module")
def ref_texts():
    return [c for n in G.NAMES for c in contigs_of(open(os.path.join(GOLDEN, "screen", n + ".fa"), "rb").read()) if len(c) > 400]


@pytest.fixture(scope="module")
def pair_data(ref_texts):
    return C.tables_pair_data(ref_texts)


@pytest.fixture(scope="module")
def barcoded_data(ref_texts):
    return C.barcoded_data(ref_texts)


class Inputs:
    """the inputs in device memory, one set at a time: asking for another set closes the one that is there"""

    def __init__(self):
        self.kind, self.bigs = None, ()

    def drop(self):
        for b in self.bigs:
            b.close()
        self.kind, self.bigs = None, ()

    def get(self, kind, make):
        if self.kind != kind:
            self.drop()
            self.bigs, self.kind = make(), kind
        return self.bigs


@pytest.fixture(scope="module")
def inputs(gpu):
    held = Inputs()
    yield held
    held.drop()


@pytest.fixture
def pair(gpu, inputs, pair_data):
    """R1 and R2 above 2^32: blocks of different lengths, repeated equally often, at different offsets from a 16-byte boundary"""
    (b1, b2, _), (t1, t2, _) = pair_data
    R = -(-C.LIMIT // min(b1.size, b2.size))
    p1, p2 = inputs.get("pair", lambda: (Big(gpu, b1, t1, R), Big(gpu, b2, t2, R, at=11)))
    assert p1.n != p2.n and min(p1.n, p2.n) > C.LIMIT and p1.ptr % 16 != p2.ptr % 16
    return p1, p2


@pytest.fixture
def barcoded(gpu, inputs, barcoded_data):
    """R1 and R2 with inline barcodes, repeated until the last destination of both clipped outputs starts above 2^32"""
    (b1, b2, _), (t1, t2, _) = barcoded_data
    R = C.demux_R(C.demux_of(b1, b2, **C.DEMUX_KW))
    return inputs.get("barcoded", lambda: (Big(gpu, b1, t1, R), Big(gpu, b2, t2, R, at=11)))


def bits_for(distinct):
    """the least table_bits with 2^bits >= 4 * distinct"""
    return max(10, (4 * distinct - 1).bit_length())


def marks_text(offsets, total, what):
    """for the message: which of the consecutive pieces that start at `offsets` holds bytes 2^31 and 2^32 of `total` bytes"""
    at = ["in piece %d" % (int(np.searchsorted(offsets, m, "right")) - 1) if m < total else "behind its end" for m in (2 ** 31, 2 ** 32)]
    return "%s of %d bytes: byte 2^31 lies %s, byte 2^32 %s" % (what, total, at[0], at[1])


# ---- fq-kcount ------------------------------------------------------------------------------------------------------------------

def check_kcount(scfq, want, k, flags, ctx, *bufs, readers=True):
    """the summary against the composed Want and the whole dump as arrays; with readers: the histograms, 1000 present and 1000
    absent keys, and the summary-only call"""
    table = want.table
    bits = bits_for(want.distinct)
    s, t = scfq.kcount_device(*bufs, k=k, flags=flags, table_bits=bits)
    with t:
        assert_kcount(s, want, k, flags, ctx)
        assert (int(s.slots), int(s.passes)) == (1 << bits, 1), (ctx, int(s.slots), int(s.passes))
        got, owed = t.dump(1, 0), np.array(dump_of(table), np.uint64).reshape(-1, 2)
        if got.shape != owed.shape or not np.array_equal(got, owed):
            rows = np.flatnonzero((got != owed).any(axis=1))[:4] if got.shape == owed.shape else []
            raise AssertionError((ctx, "dump differs", got.shape, owed.shape, [(got[i].tolist(), owed[i].tolist()) for i in rows]))
        if not readers:
            return
        for bins in (2, 8193, 1 << 20):
            h = t.hist(bins)
            assert np.array_equal(h, np.array(hist_of(table, bins), np.uint64)), (ctx, "hist", bins)
        rng = np.random.default_rng(k)
        R = ctx[-1]
        often = [key for key, c in table.items() if c > R]
        present = [often[i] for i in rng.choice(len(often), 1000, replace=False)]
        full = 4 ** k - 1
        absent = [v for v in (int(x) & full for x in rng.integers(0, 2 ** 64, 1200, dtype=np.uint64))
                  if (canonical_key(v, k) if flags & CANONICAL else v) not in table][:1000]
        assert len(absent) == 1000
        ask = [revcomp_index(v, k) if (flags & CANONICAL) and i % 2 else v for i, v in enumerate(present)]
        counts = t.query(np.array(ask + absent, dtype=np.uint64)).tolist()
        assert counts == [table[v] for v in present] + [0] * 1000, (ctx, "query")
    s0, none = scfq.kcount_device(*bufs, k=k, flags=flags, table_bits=bits, table=False)
    assert none is None and bytes(s0) == bytes(s), (ctx, "the summary without a table")


@pytest.mark.parametrize("k,canonical", [(13, False), (21, True), (32, True)])
def test_kcount(gpu, scfq, pair, pair_data, k, canonical):
    """two inputs above 2^32 into one table.  Every count is R * the block's + the tail's: lines behind 2^32 that a narrowed line_off or
    line_run + before sends elsewhere show as counts that are short of a multiple of R in the dump (the message prints the first
    rows that differ), as kmers / windows / short_lines that differ in the summary, or as histogram bins around R that moved"""
    (b1, b2, _), (t1, t2, _) = pair_data
    p1, p2 = pair
    w = C.compose_kcount(C.kcount_of(b1, b2, k, canonical), C.kcount_of(t1, t2, k, canonical), p1.R)
    want = C.kcount_want(w)
    assert want.input_bytes == p1.n + p2.n and want.max_count > 8192 * 4 and want.short_lines > 0
    check_kcount(scfq, want, k, CANONICAL if canonical else 0, ("kcount", where(0, (p1.B, p2.B)), p1.R), p1.ptr, p1.n, p2.ptr, p2.n)


@pytest.mark.parametrize("n", C.CUTS)
def test_kcount_length_at_the_edge(gpu, scfq, pair, pair_data, n):
    """one input with a length next to 2^31 or 2^32, which ends inside a record: the chunk behind an input that ends next to 2^32.  A
    length or a last line taken modulo 2^32 shows as windows / kmers / lines of a far shorter input in the summary"""
    big, block = pair[0], pair_data[0][0]
    assert 0 < n % big.B and n < big.L["filler"]
    w = C.cut_of(lambda a: C.kcount_of(a, None, 13, False), C.compose_kcount, block, n)
    ctx = ("kcount", "n = %d: %d repetitions and %d bytes" % (n, n // big.B, n % big.B), n // big.B)
    check_kcount(scfq, C.kcount_want(w), 13, 0, ctx, big.ptr, n, readers=False)


# ---- fq-normalize ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def norm_table(gpu, scfq, pair_data):
    """(the library's table of the counted input — small, on the host —, the checker's): counted once, before any test's own
    memory is counted"""
    (b1, b2, _), (t1, t2, _) = pair_data
    counted = C.normalize_counted(b1, b2, t1, t2)
    ctable = C.kcount_of(counted, None, K, True)["table"]
    bits = bits_for(len(ctable))
    s, dtable = scfq.kcount_host(counted, k=K, flags=CANONICAL, table_bits=bits)
    assert (int(s.distinct), int(s.slots)) == (len(ctable), 1 << bits)
    with dtable:
        yield dtable, ctable


def check_kept(torch, big, body, kept, len_block, len_tail, ctx):
    """body: an output on the device.  It holds the bytes of the kept units (kept: uint8 per unit of the whole input; len_block /
    len_tail: the bytes a unit of the block / the tail has in this output) in input order: 256 repetitions at a time, the byte mask of
    the chunk selects from the input what the output must hold between the chunk's first and last output offset"""
    R, B, Ub = big.R, big.B, len_block.size
    assert int(len_block.sum()) == B and int(len_tail.sum()) == big.tail.size and kept.size == R * Ub + len_tail.size
    per_rep = (kept[:R * Ub].reshape(R, Ub).astype(np.int64) * len_block).sum(axis=1)
    at = np.concatenate([[0], np.cumsum(per_rep)])                   # where every repetition's kept bytes start in the output
    places = marks_text(at, body.numel(), "the output (pieces: the repetitions' kept bytes)")
    kept_d, lens_d = torch.from_numpy(kept[:R * Ub].copy()).cuda().bool(), torch.from_numpy(len_block.copy()).cuda()
    filler = big.filler()
    for r0 in range(0, R, 256):
        r1 = min(R, r0 + 256)
        mask = torch.repeat_interleave(kept_d[r0 * Ub:r1 * Ub], lens_d.repeat(r1 - r0))
        owed, have = filler[r0 * B:r1 * B][mask], body[int(at[r0]):int(at[r1])]
        if not torch.equal(owed, have):
            for r in range(r0, r1):                                 # name the first repetition that differs
                m = torch.repeat_interleave(kept_d[r * Ub:(r + 1) * Ub], lens_d)
                o, h = filler[r * B:(r + 1) * B][m], body[int(at[r]):int(at[r + 1])]
                if not torch.equal(o, h):
                    i = int((o != h).nonzero()[0])
                    raise AssertionError((ctx, "the kept bytes of repetition %d of %d differ at byte %d of them" % (r, R, i), where(r, B),
                                          "output bytes [%d, %d)" % (at[r], at[r + 1]), places, bytes(h[i:i + 60].cpu().numpy()), bytes(o[i:i + 60].cpu().numpy())))
    start = np.cumsum(len_tail) - len_tail
    owed = b"".join(big.tail[a:a + n].tobytes() for a, n, k in zip(start.tolist(), len_tail.tolist(), kept[R * Ub:].tolist()) if k)
    assert body[int(at[R]):].cpu().numpy().tobytes() == owed, (ctx, "the tail's kept records differ", "output bytes from %d" % at[R], places)


def sampled_want(ctable, blocks, tails, R, **more):
    block = C.normalize_of(ctable, K, True, *blocks, bins=BINS, **more, **C.NORM_SAMPLED)
    tail = C.normalize_of(ctable, K, True, *tails, bins=BINS, **more, **C.NORM_SAMPLED)
    return C.compose_normalize_sampled(block, tail, R, **C.NORM_SAMPLED)


def check_sampled(torch, scfq, dtable, want, bigs, interleaved, ctx):
    """the sampled rule against a given table: the sizing call, then outputs and the per-read table between guards"""
    first = bigs[0]
    R, Ub = first.R, (len(want["classes"]) - len(want["recs"].tail) // 2) // first.R
    # the unit number counts beyond 2^32 bytes: some record of a repetition behind the one that holds input byte 2^32 gets another
    # class than the same record in repetition 0 (a unit number that restarts, or is cut, gives repetition 0's classes again)
    cls = want["classes"][:R * Ub].reshape(R, Ub)
    beyond = max(b.L["marks"][2 ** 32] for b in bigs) + 1
    assert beyond < R and (cls[beyond:] != cls[0]).any() and len(set(want["classes"].tolist())) == 4
    assert 0 < want["units_out"] < want["units_in"]
    args = [x for b in bigs for x in (b.ptr, b.n)] + ([None, 0] if len(bigs) == 1 else [])
    opts = scfq.norm_opts(interleaved=interleaved, **C.NORM_SAMPLED)
    s0, _ = scfq.norm_device(dtable, *args, opts)
    assert_norm(s0, want, (ctx, "sizing"))
    reads = want["reads_in"]
    outs = [Room(torch, want["out%d_bytes" % (j + 1)]) for j in range(len(bigs))]
    recs = Room(torch, 16 * reads)
    s, hist = scfq.norm_device(dtable, *args, opts, *[o.arg() for o in outs], recs=(recs.ptr, reads), bins=BINS)
    assert_norm(s, want, ctx)
    assert np.array_equal(hist.astype(np.int64), want["hist"]), (ctx, "hist", np.flatnonzero((hist.astype(np.int64) != want["hist"]).any(axis=1))[:5])
    assert recs.intact() and all(o.intact() for o in outs), (ctx, "bytes around the outputs or the per-read table were written")
    B = tuple(b.B for b in bigs) if len(bigs) > 1 else first.B
    assert_tiled(torch, recs.body.view(reads, 16), packed_tiled(want["recs"], NORM_REC), (ctx, "per-read table"), B)
    for j, (big, o) in enumerate(zip(bigs, outs)):
        ln = want["len%d" % (j + 1)]
        check_kept(torch, big, o.body, want["kept"], ln.block, ln.tail, (ctx, "out%d" % (j + 1)))


def test_normalize_given_table_sampled(gpu, scfq, pair, pair_data, norm_table):
    """target = 3 against a table of small depths: whether a unit of depth 4, 9 or 12 is kept depends on its number u, which passes
    the block's unit count 7000 times.  A narrowed text offset ss + c0 + pos shows as a repetition next to 2^31 or 2^32 whose rows of
    the per-read table differ (assert_tiled names it); a narrowed off_1[g] / w1 or a 32-bit scan of group_len as kept bytes of a
    repetition that differ, with the place of 2^31 and 2^32 in the output in the message; a unit number that is cut as
    dropped_high / units_out that differ in the statistics"""
    (b1, b2, _), (t1, t2, _) = pair_data
    dtable, ctable = norm_table
    want = sampled_want(ctable, (b1, b2), (t1, t2), pair[0].R)
    check_sampled(gpu, scfq, dtable, want, pair, False, "normalize, sampled")


def test_normalize_two_pass(gpu, scfq, pair, pair_data):
    """table = NULL: count_resident over both inputs, then N0 - N3, past 2^32 in one call.  min_depth = R + 1 drops the reads whose
    median k-mer occurs once per repetition; a k-mer of a line behind 2^32 that is counted elsewhere or not at all lowers a depth below
    a multiple of R, which shows in `distinct`, in the per-read table of a repetition (assert_tiled) and in the histogram, whose
    depths all lie above the 2048 bins kept in LDS"""
    torch = gpu
    (b1, b2, _), (t1, t2, _) = pair_data
    p1, p2 = pair
    R, bins = p1.R, 1 << 20
    table = C.compose_kcount(C.kcount_of(b1, b2, K, True), C.kcount_of(t1, t2, K, True), R)["table"]
    rule = dict(target=0, min_depth=R + 1)
    want = C.compose_normalize(C.normalize_of(table, K, True, b1, b2, bins=bins, **rule), C.normalize_of(table, K, True, t1, t2, bins=bins, **rule), R)
    assert want["dropped_low"] > R and want["units_out"] > R and int(want["hist"][2048:, 0].sum()) > want["units_in"] - 1000
    opts = scfq.norm_opts(k=K, canonical=True, table_bits=bits_for(len(table)), **rule)
    reads = want["reads_in"]
    recs = Room(torch, 16 * reads)
    hists = []

    def call(outs):
        s, hist = scfq.norm_device(None, p1.ptr, p1.n, p2.ptr, p2.n, opts, *outs, recs=(recs.ptr, reads) if outs[0] else None, bins=bins)
        hists.append(hist)
        return s

    s = check_outputs(torch, call, lambda s: [int(s.out1_bytes), int(s.out2_bytes)], want, ("out1", "out2"), (p1.B, p2.B), "normalize, two-pass")
    assert_norm(s, want, "normalize, two-pass")
    assert int(s.distinct) == len(table) and int(s.slots) == 1 << bits_for(len(table))
    for hist in hists:
        assert np.array_equal(hist.astype(np.int64), want["hist"]), ("hist", np.flatnonzero((hist.astype(np.int64) != want["hist"]).any(axis=1))[:5])
    assert recs.intact(), "bytes around the per-read table were written"
    assert_tiled(torch, recs.body.view(reads, 16), packed_tiled(want["recs"], NORM_REC), "normalize, two-pass, per-read table", (p1.B, p2.B))


def test_normalize_given_table_keeps_all(gpu, scfq, pair, pair_data, norm_table):
    """no rule at all against the given table: every unit with a k-mer is kept, so both outputs pass 2^32 (the sampled rule keeps a
    third of the bytes).  A narrowed off_1[g] / w1 or a 32-bit scan of group_len shows as a repetition next to 2^31 or 2^32 of an
    output that differs from the input's"""
    (b1, b2, _), (t1, t2, _) = pair_data
    p1, p2 = pair
    dtable, ctable = norm_table
    rule = dict(target=0, min_depth=0)
    want = C.compose_normalize(C.normalize_of(ctable, K, True, b1, b2, **rule), C.normalize_of(ctable, K, True, t1, t2, **rule), p1.R)
    assert min(len(want["out1"]), len(want["out2"])) > C.LIMIT and want["dropped_no_kmers"] > 0
    opts = scfq.norm_opts(**rule)
    s = check_outputs(gpu, lambda outs: scfq.norm_device(dtable, p1.ptr, p1.n, p2.ptr, p2.n, opts, *outs)[0],
                      lambda s: [int(s.out1_bytes), int(s.out2_bytes)], want, ("out1", "out2"), (p1.B, p2.B), "normalize, everything kept")
    assert_norm(s, want, "normalize, everything kept")


def test_normalize_interleaved_sampled(gpu, scfq, inputs, pair_data, norm_table):
    """one interleaved input: both mates of a unit go to out1, so a unit's bytes are two records.  (Failures read as in the two-file
    test.)"""
    (_, _, bi), (_, _, ti) = pair_data
    dtable, ctable = norm_table
    inputs.drop()
    big = Big(gpu, bi, ti)
    try:
        want = sampled_want(ctable, (bi,), (ti,), big.R, interleaved=True)
        assert want["out2_bytes"] == 0
        check_sampled(gpu, scfq, dtable, want, (big,), True, "normalize, sampled, interleaved")
    finally:
        big.close()


# ---- fq-demux -------------------------------------------------------------------------------------------------------------------

def check_demux(torch, scfq, want, bigs, ctx, **kw):
    """before the device sees anything: the outputs pass 2^32 inside other slices than the input does.  Then the sizing call, the call
    with outputs and the per-unit table between guards, and every destination's slice of every output against its Tiled"""
    rows, which = want["rows"], "12"[:len(bigs)]
    assert sum(r["bytes1"] > 2 ** 29 for r in rows) >= 3
    for w in which:
        for m in (2 ** 31, 2 ** 32):
            assert any(r["off" + w] < m < r["off" + w] + r["bytes" + w] - 1 for r in rows), (ctx, "byte %d of out%s lies on a slice's edge" % (m, w), rows)
        assert rows[-1]["off" + w] > 2 ** 32, (ctx, "the last destination of out%s starts at %d" % (w, rows[-1]["off" + w]))
    assert want["no_barcode"] > 0 and min(want["perfect"], want["mismatched"], want["unmatched"]) > bigs[0].R
    args = [x for b in bigs for x in (b.ptr, b.n)] + ([None, 0] if len(bigs) == 1 else [])
    opts = scfq.demux_opts(**C.DEMUX_KW, **kw)
    B = tuple(b.B for b in bigs) if len(bigs) > 1 else bigs[0].B
    with scfq.demux_sheet(list(C.DEMUX_SAMPLES)) as sheet:
        s0, rows0 = scfq.demux_device(sheet, *args, opts)
        assert_demux(s0, rows0, want, (ctx, "sizing"))
        units = want["units_in"]
        table = Room(torch, 8 * units)
        outs = [Room(torch, want["out%s_bytes" % w]) for w in which]
        s, got_rows = scfq.demux_device(sheet, *args, opts, *[o.arg() for o in outs], *([None] if len(bigs) == 1 else []), recs=(table.ptr, units))
    assert_demux(s, got_rows, want, ctx)
    assert table.intact() and all(o.intact() for o in outs), (ctx, "bytes around the outputs or the per-unit table were written")
    assert_tiled(torch, table.body.view(units, 8), packed_tiled(want["recs"], DEMUX_REC), (ctx, "per-unit table"), B)
    for w, o in zip(which, outs):
        places = marks_text(np.array([r["off" + w] for r in rows]), want["out%s_bytes" % w], "out%s (pieces: the destinations)" % w)
        for d, r in enumerate(rows):
            lo, hi = r["off" + w], r["off" + w] + r["bytes" + w]
            assert_tiled(torch, o.body[lo:hi], want["out" + w][d], (ctx, "destination %d: bytes [%d, %d) of out%s" % (d, lo, hi, w), places), B)


@pytest.mark.parametrize("keep_barcode", [False, True])
def test_demux_two_files(gpu, scfq, barcoded, barcoded_data, keep_barcode):
    """inline barcodes, one mismatch; clipped (dx_write's three runs) and keep_barcode (whole records).  More than 10^7 units are sorted
    by (key, unit): a unit number cut in the sort or a 32-bit group sum in dx_lengths shows as rows whose bytes1 / off1 differ in the
    statistics; a narrowed write offset as a repetition of a destination's slice that differs — assert_tiled names it, and the
    message says which destination holds bytes 2^31 and 2^32 of that output, which is another sample's slice than in the input"""
    (b1, b2, _), (t1, t2, _) = barcoded_data
    kw = dict(keep_barcode=keep_barcode)
    want = C.compose_demux(C.demux_of(b1, b2, **C.DEMUX_KW, **kw), C.demux_of(t1, t2, **C.DEMUX_KW, **kw), barcoded[0].R)
    assert want["units_in"] > 10 ** 7 and (want["bases_clipped"] == 0) == keep_barcode
    check_demux(gpu, scfq, want, barcoded, ("demux, two files", kw), **kw)


def test_demux_interleaved(gpu, scfq, inputs, barcoded_data):
    """one interleaved input, one output: dx_write's `second` branch writes mate 2 behind mate 1 at w1 + first.  A narrowed w1 + first
    shows as a repetition of a destination's slice whose second records differ"""
    (_, _, bi), (_, _, ti) = barcoded_data
    kw = dict(interleaved=True)
    block = C.demux_of(bi, **C.DEMUX_KW, **kw)
    inputs.drop()
    big = Big(gpu, bi, ti, C.demux_R(block))
    try:
        want = C.compose_demux(block, C.demux_of(ti, **C.DEMUX_KW, **kw), big.R)
        assert want["out2_bytes"] == 0 and want["unpaired"] == 0
        check_demux(gpu, scfq, want, (big,), "demux, interleaved", **kw)
    finally:
        big.close()

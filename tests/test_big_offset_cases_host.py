"""tests/_big_offset_cases.py without a GPU: every composition law against the checker on the whole of block x 3 + tail, the cut
inputs against the checker on block x 3 cut in its last repetition, and the arithmetic of `layout`.  Every comparison is ==."""
import os

import numpy as np
import pytest

import _big_offset_cases as C
from conftest import GOLDEN
from _fa_gc_check import FaModel
from _screen_check import index_of_np

R = 3
NAMES = ("spike", "vector", "rrna")


def same(composed, direct):
    bad = C.equal(C.whole(composed), direct)
    assert not bad, bad


@pytest.fixture(scope="module")
def probes(scfq):
    return [seq.encode() for _, seq in scfq.adapters_default()]


@pytest.fixture(scope="module")
def single(probes):
    rng = np.random.default_rng(20261001)
    block, fields = C.single_block(rng, probes, records=40)
    tail = C.single_tail(rng, probes, block, fields, (0, 1, 1, 2))
    return block, fields, tail, np.concatenate([np.tile(block, R), tail])


@pytest.fixture(scope="module")
def refs():
    return [open(os.path.join(GOLDEN, "screen", n + ".fa"), "rb").read() for n in NAMES]


@pytest.fixture(scope="module")
def paired(refs):
    from _screen_check import contigs_of
    texts = [c for r in refs for c in contigs_of(r) if len(c) > 400]
    rng = np.random.default_rng(20261002)
    blocks = C.paired_blocks(rng, texts, pairs=60)
    tails = C.paired_tails(rng, texts)
    return blocks, tails, [np.concatenate([np.tile(b, R), t]) for b, t in zip(blocks, tails)]


def test_layout_facts(probes, refs):
    from _screen_check import contigs_of
    texts = [c for r in refs for c in contigs_of(r) if len(c) > 400]
    rng = np.random.default_rng(20261003)
    block, fields = C.single_block(rng, probes)
    b1, b2, bi = C.paired_blocks(rng, texts)
    fa, _, _ = C.fasta_block(rng)
    assert len({block.size, b1.size, b2.size, bi.size, fa.size}) == 5
    # the inputs of fq-kcount / fq-normalize (other pairs of the same lengths) and of fq-demux: new lengths, and repeated more often
    (k1, k2, ki), _ = C.tables_pair_data(texts)
    (x1, x2, xi), _ = C.barcoded_data(texts)
    assert len({block.size, b1.size, b2.size, bi.size, fa.size, x1.size, x2.size, xi.size}) == 8 and len({k1.size, k2.size, ki.size}) == 3
    more = C.demux_R(C.demux_of(x1, x2, **C.DEMUX_KW))
    assert more > -(-C.LIMIT // min(x1.size, x2.size))
    for blk in (k1, k2, ki, x1, x2, xi):
        off = C.index_of(blk)["off"]
        assert blk[-1] == 10 and (off.size - 1) % 4 == 0
        for m in C.MARKS:                                        # strictly inside a record: no record of any repetition starts there
            assert m % blk.size not in off[::4] and (m + 1) % blk.size not in off[::4]
    pairs = ((b1.size, None), (bi.size, None), (max(b1.size, b2.size), -(-C.LIMIT // min(b1.size, b2.size))),
             (k1.size, None), (ki.size, None), (max(k1.size, k2.size), -(-C.LIMIT // min(k1.size, k2.size))),
             (x1.size, more), (x2.size, more), (xi.size, C.demux_R(C.demux_of(xi, interleaved=True, **C.DEMUX_KW))))
    for B, given in ((block.size, None), (fa.size, None)) + pairs:
        assert 400_000 < B < 1_300_000
        L = C.layout(B, 12345, given)
        assert B % 2 == 1 and B % 3 != 0
        assert L["R"] * B >= C.LIMIT and (given is not None or (L["R"] - 1) * B < C.LIMIT)
        assert L["filler"] == L["R"] * B == L["tail_at"] and L["n"] == L["filler"] + 12345
        assert 2 ** 32 < L["tail_at"] and L["n"] < 2 ** 33
        for m in C.MARKS:
            r = L["marks"][m]
            assert r * B <= m < (r + 1) * B and 0 < r < L["R"] - 1 and m < L["filler"]
        # a record's edge does not sit on 2^31 or 2^32: a repetition starts there at most by accident, and then none of these would
        assert all(m % B not in (0, B - 1) for m in C.MARKS)
        # every residue mod 16 is the start of some repetition (B is odd), and more than a thousand residues mod 4096
        starts = (np.arange(L["R"], dtype=np.int64) * B)
        assert np.unique(starts % 16).size == 16 and np.unique(starts % 4096).size == min(L["R"], 4096)
        for n in C.CUTS:
            assert 0 < n % B and n < L["filler"]


def test_tiled_and_compose():
    t = C.Tiled(np.array([0, 5, 9], np.int64), 3, np.array([0, 2, 4], np.int64), step=11)
    assert t.whole().tolist() == [0, 5, 9, 11, 16, 20, 22, 27, 31, 33, 35, 37] and len(t) == 12
    assert C.Tiled(b"ab", 2, b"c").whole() == b"ababc"
    w = C.compose(dict(a=1, p=7, m=3, t=b"x", v=[1, 2], h=np.array([1, 2])), dict(a=10, p=7, m=5, t=b"y", v=[0, 1], h=np.array([1, 1, 1])), 4,
                  same=("p",), longest=("m",), tiled=("t",))
    assert C.whole(w)["t"] == b"xxxxy" and (w["a"], w["p"], w["m"], w["v"], w["h"].tolist()) == (14, 7, 5, [4, 9], [5, 9, 1])
    assert sorted(C.equal(dict(a=1, b=np.zeros(2)), dict(a=2, b=np.zeros(3)))) == ["a", "b"]


def test_line_index(single):
    block, _, tail, data = single
    same(C.compose_index(C.index_of(block), C.index_of(tail), R, block.size), C.index_of(data))
    for c in (1, 2, block.size // 2, block.size - 1):
        cut = np.tile(block, R)[:2 * block.size + c]
        same(C.cut_of(C.index_of, C.compose_index, block, cut.size, B=block.size), C.index_of(cut))


def test_readstats(single):
    from _readstats_check import summary_of
    block, _, tail, data = single
    want = C.compose_readstats(C.readstats_of(block), C.readstats_of(tail), R)
    direct = C.readstats_of(data)
    same(want, direct)
    assert summary_of(want["rows"].whole()) == summary_of(direct["rows"])
    for c in (1, block.size // 3, block.size - 1):
        cut = np.tile(block, R)[:2 * block.size + c]
        same(C.cut_of(C.readstats_of, C.compose_readstats, block, cut.size), C.readstats_of(cut))


def test_cycles(single):
    block, _, tail, data = single
    same(C.compose_cycles(C.cycles_of(block), C.cycles_of(tail), R), C.cycles_of(data))
    same(C.compose_cycles(C.cycles_of(tail), C.cycles_of(block), R), C.cycles_of(np.concatenate([np.tile(tail, R), block])))


@pytest.mark.parametrize("k,canonical", [(7, False), (7, True), (12, False), (12, True)])
def test_kmers(single, k, canonical):
    block, _, tail, data = single
    same(C.compose_kmers(C.kmers_of(block, k, canonical), C.kmers_of(tail, k, canonical), R), C.kmers_of(data, k, canonical))
    if k == 7:
        for c in (5, block.size // 3, block.size - 1):
            cut = np.tile(block, R)[:2 * block.size + c]
            want = C.cut_of(lambda a: C.kmers_of(a, k, canonical), C.compose_kmers, block, cut.size)
            same(want, C.kmers_of(cut, k, canonical))


def test_adapters(single, probes):
    block, _, tail, data = single
    direct = C.adapters_of(data, probes)
    same(C.compose_adapters(C.adapters_of(block, probes), C.adapters_of(tail, probes), R), direct)
    assert sum(direct["hits"]) > 20 and sum(C.adapters_of(tail, probes)["hits"]) > 5


def test_dedup(single, oracle):
    block, fields, tail, _ = single
    data = np.concatenate([C.numbered(block, fields, R), tail])
    out, st = oracle.dedup(data)
    kept, want = C.dedup_of(block, fields, R, tail)
    assert out == data[:R * block.size].tobytes() + kept
    assert {k: int(getattr(st, k)) for k in want} == want
    assert want["duplicates"] == 300 // 5 + 1
    # without the repetition numbers the law does not hold: the test of the law can fail
    assert oracle.dedup(np.concatenate([np.tile(block, R), tail]))[0] != out


def test_insert_size(paired):
    (b1, b2, bi), (t1, t2, ti), (d1, d2, di) = paired
    direct = C.insert_of(d1, d2)
    same(C.compose_insert(C.insert_of(b1, b2), C.insert_of(t1, t2), R), direct)
    same(C.compose_insert(C.insert_of(bi), C.insert_of(ti), R), C.insert_of(di))
    assert direct["overlapped"] > 100 and direct["too_long"] > 20 and direct["min_insert"] < direct["median_insert"] < direct["max_insert"]


def test_merge(paired):
    (b1, b2, _), (t1, t2, _), (d1, d2, _) = paired
    direct = C.merge_of(d1, d2)
    same(C.compose_merge(C.merge_of(b1, b2), C.merge_of(t1, t2), R), direct)
    assert min(len(direct[k]) for k in C.MERGE_OUTPUTS) > 1000


def test_trim(paired):
    (b1, b2, _), (t1, t2, _), (d1, d2, _) = paired
    direct = C.trim_of(d1, d2, **C.TRIM_ALL)
    same(C.compose_trim(C.trim_of(b1, b2, **C.TRIM_ALL), C.trim_of(t1, t2, **C.TRIM_ALL), R), direct)
    assert min(direct[k] for k in ("cut_overlap", "cut_adapter", "cut_polyg", "cut_quality", "dropped_reads", "too_long")) > 0


def test_screen(paired, refs):
    index = index_of_np(list(zip(NAMES, refs)), 31)
    (b1, b2, _), (t1, t2, _), (d1, d2, _) = paired
    direct = C.screen_of(index, d1, d2, **C.SCREEN_KW)
    same(C.compose_screen(C.screen_of(index, b1, b2, **C.SCREEN_KW), C.screen_of(index, t1, t2, **C.SCREEN_KW), R), direct)
    assert direct["matched_pairs"] > 20 and 0 < direct["reads_out"] < direct["reads_in"]


def test_fasta():
    """the contig table of block x 3 + tail, the repetition numbers written in, is the block's R times (names numbered, offsets moved on
    by r B) and the tail's; the counts of an interval are those of the block's model"""
    rng = np.random.default_rng(20261004)
    block, fields, names = C.fasta_block(rng)
    tail = C.fasta_tail(rng)
    mb, mt = FaModel(block), FaModel(tail)
    whole = FaModel(np.concatenate([C.numbered(block, fields, R), tail]))
    cb = len(mb.contigs)
    want = [(nm[:len(names[j])] + b"%08x" % r, off + r * block.size, ln) for r in range(R) for j, (nm, off, _, ln) in enumerate(mb.contigs)]
    want += [(nm, off + R * block.size, ln) for nm, off, _, ln in mt.contigs]
    assert [(c[0], c[1], c[3]) for c in whole.contigs] == want
    assert (whole.bases, whole.gc_bases, whole.acgt_bases) == (R * mb.bases + mt.bases, R * mb.gc_bases + mt.gc_bases, R * mb.acgt_bases + mt.acgt_bases)
    for r in range(R):
        q = C.fasta_intervals(rng, mb, r * cb)
        assert (whole.count_many(q) == mb.count_many([(c - r * cb, lo, hi) for c, lo, hi in q])).all()
    q = C.fasta_intervals(rng, mt, R * cb)
    assert (whole.count_many(q) == mt.count_many([(c - R * cb, lo, hi) for c, lo, hi in q])).all()
    assert mb.gc_bases != mb.acgt_bases and mb.acgt_bases != mb.bases


# ---- fq-kcount, fq-demux, fq-normalize ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def texts(refs):
    from _screen_check import contigs_of
    return [c for r in refs for c in contigs_of(r) if len(c) > 400]


@pytest.fixture(scope="module")
def barcoded(texts):
    rng = np.random.default_rng(20261005)
    blocks = C.barcoded_blocks(rng, texts, pairs=60)
    tails = C.barcoded_tails(rng, texts)
    return blocks, tails, [np.concatenate([np.tile(b, R), t]) for b, t in zip(blocks, tails)]


@pytest.mark.parametrize("k,canonical", [(13, False), (21, True), (32, False)])
def test_kcount(paired, k, canonical):
    (b1, b2, _), (t1, t2, _), (d1, d2, _) = paired
    for blocks, tails, data in (((b1, None), (t1, None), (d1, None)), ((b1, b2), (t1, t2), (d1, d2))):
        block, tail = C.kcount_of(*blocks, k, canonical), C.kcount_of(*tails, k, canonical)
        want, direct = C.compose_kcount(block, tail, R), C.kcount_of(*data, k, canonical)
        same(want, direct)
        assert C.kcount_want(want) == C.kcount_want(direct) and C.kcount_want(want).distinct == len(direct["table"])
        assert set(tail["table"]) - set(block["table"]), "a key that only the tail has"
        assert set(tail["table"]) & set(block["table"]), "a key whose count is R * the block's + the tail's"
    if k == 13:
        for c in (5, b1.size // 3, b1.size - 1):
            cut = np.tile(b1, R)[:2 * b1.size + c]
            same(C.cut_of(lambda a: C.kcount_of(a, None, k, canonical), C.compose_kcount, b1, cut.size), C.kcount_of(cut, None, k, canonical))


def written_demux(w):
    out = C.whole(w)
    for which in ("out1", "out2"):
        out[which] = b"".join(t.whole() for t in w[which])
    return out


@pytest.mark.parametrize("keep_barcode", [False, True])
def test_demux(barcoded, keep_barcode):
    (b1, b2, bi), (t1, t2, ti), (d1, d2, di) = barcoded
    kw = dict(C.DEMUX_KW, keep_barcode=keep_barcode)
    for blocks, tails, data, more in (((b1, b2), (t1, t2), (d1, d2), {}), ((bi,), (ti,), (di,), dict(interleaved=True))):
        block, tail = C.demux_of(*blocks, **kw, **more), C.demux_of(*tails, **kw, **more)
        want, direct = C.compose_demux(block, tail, R), C.demux_of(*data, **kw, **more)
        bad = C.equal(written_demux(want), direct)
        assert not bad, bad
        assert [len(t) for t in want["out1"]] == [r["bytes1"] for r in direct["rows"]]
        assert min(block["perfect"], block["mismatched"], block["unmatched"]) > 0 and block["no_barcode"] == 0 and tail["no_barcode"] > 0
        assert (direct["bases_clipped"] > 0) != keep_barcode


def test_demux_barcodes_and_shares(texts):
    """the sheet's barcodes are far enough apart for one mismatch, and the block the GPU module repeats gives every sample and
    "undetermined" at least 8 % of its units"""
    for j in (1, 2):
        codes = [s[j] for s in C.DEMUX_SAMPLES]
        assert all(len(c) == 8 for c in codes)
        assert min(sum(x != y for x, y in zip(p, q)) for i, p in enumerate(codes) for q in codes[:i]) >= 4
    (b1, b2, bi), (t1, t2, ti) = C.barcoded_data(texts)
    for blocks, tails, more in (((b1, b2), (t1, t2), {}), ((bi,), (ti,), dict(interleaved=True))):
        block, tail = C.demux_of(*blocks, **C.DEMUX_KW, **more), C.demux_of(*tails, **C.DEMUX_KW, **more)
        assert len(block["rows"]) == 6 and all(r["units"] >= 0.08 * block["units_in"] for r in block["rows"])
        assert min(block["perfect"], block["mismatched"], block["unmatched"]) > 0 and tail["no_barcode"] > 0


def test_classify_np():
    from _normalize_check import classify
    rng = np.random.default_rng(20261006)
    n = 10_000
    u = rng.integers(0, 2 ** 33, n).astype(np.uint64)
    u[:6] = (0, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1)
    for target, min_depth, seed in ((3, 2, 77), (0, 2, 5), (20, 0, 2 ** 64 - 1), (7, 7, 0)):
        mates = [rng.integers(0, 3, n), rng.integers(max(0, target - 3), target + 12, n), rng.integers(0, 3, n), rng.integers(0, 2 * target + 40, n)]
        mates[1][:6], mates[3][:6], mates[0][:6], mates[2][:6] = target + 5, target + 9, 1, 1
        cls, D = C.classify_np(*mates, u, target, min_depth, seed)
        want = [classify([(int(mates[0][i]), int(mates[1][i])), (int(mates[2][i]), int(mates[3][i]))], int(u[i]), target, min_depth, seed) for i in range(n)]
        assert list(zip(cls.tolist(), D.tolist())) == want
        assert set(cls.tolist()) == {0, 1} | ({2} if min_depth else set()) | ({3} if target else set())
    # the number of the unit matters past 32 bits: among units above 2^32 some change class when the number is cut
    big = u[u >= 2 ** 32]
    deep = np.full(big.size, 9)
    a, _ = C.classify_np(deep, deep, deep, deep, big, 3, 2, 77)
    b, _ = C.classify_np(deep, deep, deep, deep, big & np.uint64(2 ** 32 - 1), 3, 2, 77)
    assert (a != b).any()


def kept_bytes(data, lens, kept):
    at = np.cumsum(lens) - lens
    return b"".join(data[a:a + n].tobytes() for a, n, k in zip(at.tolist(), lens.tolist(), kept.tolist()) if k)


NORM_FIELDS = ("reads1", "reads2", "lines1", "lines2", "input_bytes1", "input_bytes2", "pairs", "unpaired", "units_in", "units_out", "reads_in",
               "reads_out", "dropped_no_kmers", "dropped_low", "dropped_high", "short_reads", "bases_in", "bases_out", "windows", "kmers", "skipped",
               "weak_kmers", "absent_kmers", "out1_bytes", "out2_bytes", "flags", "k", "table_flags", "target", "min_depth", "weak_below", "seed",
               "distinct", "hist", "classes", "recs")


def test_normalize(paired):
    from _normalize_check import FIELDS
    assert set(FIELDS) <= set(NORM_FIELDS)
    (b1, b2, bi), (t1, t2, ti), (d1, d2, di) = paired
    table = C.kcount_of(C.normalize_counted(b1, b2, t1, t2), None, 21, True)["table"]
    for blocks, tails, data, more in (((b1, b2), (t1, t2), (d1, d2), {}), ((bi,), (ti,), (di,), dict(interleaved=True))):
        # a rule without the hash
        rule = dict(more, target=0, min_depth=2, bins=12)
        block, tail = C.normalize_of(table, 21, True, *blocks, **rule), C.normalize_of(table, 21, True, *tails, **rule)
        direct = C.normalize_of(table, 21, True, *data, **rule)
        same(C.compose_normalize(block, tail, R), direct)
        assert 0 < direct["dropped_low"] and 0 < direct["units_out"] and tail["dropped_no_kmers"] > 0
        # the sampled rule: the statistics and the histogram, then the outputs from the kept mask and the lengths
        for keep in (False, True):
            want = C.compose_normalize_sampled(block, tail, R, keep_no_kmers=keep, **C.NORM_SAMPLED)
            direct = C.normalize_of(table, 21, True, *data, bins=12, keep_no_kmers=keep, **more, **C.NORM_SAMPLED)
            bad = C.equal({k: v for k, v in C.whole(want).items() if k in NORM_FIELDS}, {k: direct[k] for k in NORM_FIELDS})
            assert not bad, bad
            kept = want["kept"]
            assert kept.size == direct["units_in"] and kept_bytes(data[0], want["len1"].whole(), kept) == direct["out1"]
            if more:
                assert direct["out2"] == b"" and want["out2_bytes"] == 0
            else:
                assert kept_bytes(data[1], want["len2"].whole(), kept) == direct["out2"]
            assert min(direct["dropped_high"], direct["dropped_low"], direct["units_out"]) > 0
        # the law can fail: with the block's own numbering in every repetition other units are kept
        Ub = len(block["classes"])
        local = np.concatenate([np.tile(np.arange(Ub, dtype=np.uint64), R), R * Ub + np.arange(len(tail["classes"]), dtype=np.uint64)])
        right = C.compose_normalize_sampled(block, tail, R, **C.NORM_SAMPLED)["kept"]
        wrong = C.compose_normalize_sampled(block, tail, R, u=local, **C.NORM_SAMPLED)["kept"]
        assert (wrong[:Ub] == right[:Ub]).all() and (wrong[Ub:R * Ub] != right[Ub:R * Ub]).any() and (wrong[R * Ub:] == right[R * Ub:]).all()


def test_normalize_shares(texts):
    """the block the GPU module repeats, against the table of its counted input and under its sampled rule: each of kept without the
    hash, dropped_low, dropped_high and kept by the hash is at least 5 % of the units; the tail has units without k-mers"""
    (b1, b2, _), (t1, t2, _) = C.tables_pair_data(texts)
    table = C.kcount_of(C.normalize_counted(b1, b2, t1, t2), None, 21, True)["table"]
    block = C.normalize_of(table, 21, True, b1, b2, **C.NORM_SAMPLED)
    units, target = block["units_in"], C.NORM_SAMPLED["target"]
    D = np.minimum(block["recs"][0::2, 1], block["recs"][1::2, 1])           # (every mate of the block has k-mers)
    assert (block["recs"][:, 0] > 0).all()
    kept = block["classes"] == 0
    shares = dict(plain=int((kept & (D <= target)).sum()), low=block["dropped_low"], high=block["dropped_high"], hashed=int((kept & (D > target)).sum()))
    assert sum(shares.values()) == units and all(20 * v >= units for v in shares.values()), (shares, units)
    assert C.normalize_of(table, 21, True, t1, t2, **C.NORM_SAMPLED)["dropped_no_kmers"] > 0

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
    for B, given in ((block.size, None), (b1.size, None), (bi.size, None), (fa.size, None), (max(b1.size, b2.size), -(-C.LIMIT // min(b1.size, b2.size)))):
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

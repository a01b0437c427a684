"""fq-kcount's readers work in the table's own scratch, a piece at a time (csrc/scfq_kcount.hip: kDumpPiece slots per piece of a dump,
kQueryPiece keys per piece of a query): tables and key lists of more than one piece against the checker, compared with ==."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG
from _kcount_check import CANONICAL, dump_of, kcount_of, rows_text, top_of

pytestmark = pytest.mark.gpu

SC = os.path.join(PKG, "sc")
READS = os.path.join(GOLDEN, "kcount", "reads.fq")
K = 21


def piece_sizes():
    host = open(os.path.join(PKG, "csrc", "scfq_kcount_host.hpp")).read()
    text = open(os.path.join(PKG, "csrc", "scfq_kcount.hip")).read()
    bins = re.search(r"constexpr uint64_t kMaxBins = 1ull << (\d+);", host)
    assert bins and "kScratchBytes = kMaxBins * 8;" in text
    assert "kDumpPiece = kScratchBytes / sizeof(scfq_kmer_count);" in text and "kQueryPiece = kScratchBytes / 16;" in text
    scratch = 8 << int(bins.group(1))
    return scratch // 16, scratch // 16


@pytest.fixture(scope="module")
def want():
    data = open(READS, "rb").read()
    return data, {flags: kcount_of(data, K, flags != 0) for flags in (0, CANONICAL)}


@pytest.mark.parametrize("pieces", (1, 2, 4))
def test_dump_of_a_table_of_several_pieces(gpu, scfq, want, pieces):
    """tables of exactly one piece, of two and of four: the rows of every piece arrive, once each, filters included"""
    data, wants = want
    dump_piece, _ = piece_sizes()
    bits = (dump_piece * pieces).bit_length() - 1
    assert 1 << bits == dump_piece * pieces
    for flags in (0, CANONICAL):
        w = wants[flags]
        s, table = scfq.kcount_host(data, k=K, flags=flags, table_bits=bits)
        with table:
            assert s.slots == dump_piece * pieces and s.distinct == len(w.table)
            assert [tuple(r) for r in table.dump().tolist()] == dump_of(w.table), (pieces, flags)
            for lo, hi in ((2, 0), (5, 9), (w.max_count, 0), (w.max_count + 1, 0)):
                assert [tuple(r) for r in table.dump(lo, hi).tolist()] == dump_of(w.table, lo, hi), (pieces, flags, lo, hi)


def test_query_of_more_keys_than_a_piece(gpu, scfq, want):
    """2 pieces and 17 keys: present keys at the start, across the boundary between the pieces and at the end, absent ones between"""
    data, wants = want
    _, query_piece = piece_sizes()
    n = 2 * query_piece + 17
    for flags in (0, CANONICAL):
        w = wants[flags]
        present = np.array(sorted(w.table), dtype=np.uint64)
        rng = np.random.default_rng(5 + flags)
        keys = rng.integers(0, 1 << (2 * K), size=n, dtype=np.uint64)
        third = present.size // 3
        keys[:third] = present[:third]
        at = query_piece - third // 2
        keys[at:at + third] = present[third:2 * third]
        keys[n - (present.size - 2 * third):] = present[2 * third:]
        canon = np.minimum(keys, _revcomp(keys)) if flags else keys
        expect = np.array([w.table.get(x, 0) for x in canon.tolist()], dtype=np.uint64)
        assert int((expect > 0).sum()) >= present.size
        s, table = scfq.kcount_host(data, k=K, flags=flags)
        with table:
            got = table.query(keys)
            assert got.dtype == np.uint64 and got.shape == (n,) and np.array_equal(got, expect), flags


def _revcomp(keys):
    """reverse complement of K-mers given as indices (codes A C G T = 0 1 2 3, first base most significant)"""
    out = np.zeros_like(keys)
    x = keys.copy()
    for _ in range(K):
        out = (out << np.uint64(2)) | (np.uint64(3) - (x & np.uint64(3)))
        x >>= np.uint64(2)
    return out


def test_cli_every_row_in_a_fresh_process(gpu, want):
    """`sc fq-kcount` stages the file, counts, lets the file go and reads the table right behind that: the whole dump and a --top that
    takes every key, each in a process of its own"""
    data, wants = want
    w = wants[CANONICAL]

    def sc(*args):
        r = subprocess.run([SC, "fq-kcount", "--k=%d" % K, "--canonical", *args, READS], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        return r.stdout

    assert sc("--dump") == rows_text(dump_of(w.table), K)
    assert sc("--top=%d" % (len(w.table) + 1)) == rows_text(top_of(w.table, len(w.table) + 1), K)
    assert sc("--table-bits=21", "--dump", "--min-count=2") == rows_text(dump_of(w.table, 2), K)

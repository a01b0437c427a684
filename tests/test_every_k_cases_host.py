"""The case set of tests/_every_k_cases.py can tell a right kernel from a subtly wrong one at every k = 1 .. 32 and in both strand modes:
with the Python checkers alone, the checker's result differs from each of a handful of deliberately wrong restatements of the k-mer
spectrum (MUTANTS below), every listed ingredient is there (taking one out fails an assertion here), and the plain facts the device
sweep of test_gpu_every_k.py relies on hold.  Conditions on the inputs, not measurements; no GPU."""
import numpy as np
import pytest

import _deep_counts_cases as deep
from _every_k_cases import NORM_OPTS, OFFSETS, cases, fastq_of, forward_is_smaller, line_lengths, revcomp
from _kcount_check import kcount_of, kcount_of_np
from _kmers_check import index_of, kmers_of, kmers_of_np, revcomp_index
from _normalize_check import HIGH, KEPT, LOW, NO_KMERS, normalize_of
from _readstats_check import line_spans_np
from _screen_check import index_of as screen_index_of, index_of_np as screen_index_of_np, same, screen_of, screen_of_np

KS = range(1, 33)
MODES = (False, True)
U = np.uint64


def arr(data):
    return np.frombuffer(data, dtype=np.uint8)


def part_counts(reads, k, canonical=False):
    return kcount_of_np(arr(fastq_of(reads, final=True)), k, canonical)


# ---- the spectrum once more, with a hook at every k-dependent step -----------------------------------------------------------------
def spectrum(a, k, canonical, smear=None, at=0, key=None, cr_is_text=False):
    """(table, windows, kmers, skipped, short_lines) of the uint8 array a.  smear: the letters that decide whether a window is a k-mer
    (k); at: where the key's letters begin, relative to the window (0); key(fw, rc): the entry (fw, or the minimum in canonical mode);
    cr_is_text: a '\\r' before '\\n' belongs to the line's text (it does not)"""
    starts, tends = line_spans_np(a)
    s, e = starts[1::4], tends[1::4]
    if cr_is_text:
        e = e + ((e < a.size) & (a[np.minimum(e, a.size - 1)] == 13))
    per_line = np.maximum(e - s - k + 1, 0)
    windows, short = int(per_line.sum()), int(((e - s) < k).sum())
    first = np.cumsum(per_line) - per_line
    pos = np.arange(windows, dtype=np.int64) - np.repeat(first, per_line) + np.repeat(s, per_line)
    lut = np.full(256, 4, np.uint64)
    lut[list(b"ACGT")] = (0, 1, 2, 3)
    code = lut[np.concatenate([a, np.full(k + 2, 10, np.uint8)])]
    bad = np.zeros(windows, bool)
    for i in range(k if smear is None else smear):
        bad |= code[pos + i] == 4
    fw, rc = np.zeros(windows, U), np.zeros(windows, U)
    for i in range(k):
        c = code[pos + at + i] & U(3)
        fw = (fw << U(2)) | c
        rc |= (U(3) - c) << U(2 * i)
    idx = key(fw, rc) if key is not None else np.minimum(fw, rc) if canonical else fw
    vals, counts = np.unique(idx[~bad], return_counts=True)
    skipped = int(bad.sum())
    return {int(v): int(c) for v, c in zip(vals, counts)}, windows, windows - skipped, skipped, short


def canon(fw, rc, canonical):
    return np.minimum(fw, rc) if canonical else fw


# the wrong restatements: name -> (applies(k, canonical), keyword arguments of spectrum)
MUTANTS = {
    "smear of k - 1": (lambda k, c: True, lambda k, c: dict(smear=k - 1)),
    "smear of k + 1": (lambda k, c: True, lambda k, c: dict(smear=k + 1)),
    "key of 2 (k - 1) bits": (lambda k, c: True, lambda k, c: dict(key=lambda fw, rc: canon(fw, rc, c) & U(4 ** (k - 1) - 1))),
    "key one base on": (lambda k, c: True, lambda k, c: dict(at=1)),
    "reverse complement of k - 1": (lambda k, c: c, lambda k, c: dict(key=lambda fw, rc: np.minimum(fw, rc >> U(2)))),
    "max for min": (lambda k, c: c, lambda k, c: dict(key=np.maximum)),
    "key of 32 bits": (lambda k, c: k > 16, lambda k, c: dict(key=lambda fw, rc: canon(fw, rc, c) & U(0xFFFFFFFF))),
    "\\r is text": (lambda k, c: True, lambda k, c: dict(cr_is_text=True)),
}


def as_tuple(w):
    return w.table, w.windows, w.kmers, w.skipped, w.short_lines


@pytest.mark.parametrize("k", KS)
def test_every_wrong_restatement_differs(k):
    a = arr(cases(k).fastq)
    for canonical in MODES:
        want = as_tuple(kcount_of_np(a, k, canonical))
        assert spectrum(a, k, canonical) == want, "the restatement itself is the checker's"
        for name, (applies, kw) in MUTANTS.items():
            if applies(k, canonical):
                got = spectrum(a, k, canonical, **kw(k, canonical))
                assert got != want, (k, canonical, name)
                if name not in ("\\r is text", "smear of k - 1", "smear of k + 1"):
                    assert got[0] != want[0], (k, canonical, name, "the table")
                else:
                    assert got[3] != want[3], (k, canonical, name, "skipped")


def test_the_checkers_agree_on_the_case_set():
    """the plain forms (a slice and a dict) against the numpy forms that the sweep compares with"""
    for k in (1, 5, 6, 12, 13, 32):
        data = cases(k).fastq
        for canonical in MODES:
            assert kcount_of(data, k, canonical) == kcount_of_np(arr(data), k, canonical)
            if k <= 12:
                assert kmers_of(data, k, canonical) == kmers_of_np(arr(data), k, canonical)
    assert cases(7).fastq == type(cases(7))(7).fastq and 9_000 < len(cases(1).fastq) < len(cases(32).fastq) < 30_000


# ---- the ingredients, one by one -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_ingredients(k):
    c = cases(k)
    data, parts = c.fastq, c.parts
    assert list(parts) == ["invalid", "edges", "lengths"] and data == fastq_of([r for p in parts.values() for r in p])
    assert not data.endswith(b"\n") and fastq_of(parts["lengths"][-1:], final=True).endswith(b"\r\n")
    # every length with both line ends
    want = line_lengths(k)
    assert {0, k - 1, k, k + 1, 2 * k - 1, 2 * k, 15, 16, 17, 27, 28, 29, 46, 47, 48, 49, 63, 64, 65, 127, 128, 129, 510 + k, 511 + k, 512 + k} == set(want)
    for eol in (b"\n", b"\r\n"):
        assert [len(s) for s, e in parts["lengths"] if e == eol] == want
    assert all(set(s) <= set(b"ACGT") for s, e in parts["lengths"])
    # one invalid letter at every position: the skipped windows are those that hold position p, exactly
    inv = parts["invalid"]
    assert len(inv) == 2 * k + 1 and all(len(s) == 2 * k + 1 for s, e in inv)
    for p, (s, e) in enumerate(inv):
        assert [i for i, b in enumerate(s) if b not in b"ACGT"] == [p] and s[p:p + 1] == (b"N" if p % 2 == 0 else s[p:p + 1].lower())
    w = part_counts(inv, k)
    assert w.windows == (2 * k + 1) * (k + 2) and w.skipped == sum(min(p, k + 1) - max(0, p - k + 1) + 1 for p in range(2 * k + 1))
    # the key edges
    seqs = [s for s, e in parts["edges"]]
    assert b"T" * (k + 20) in seqs and b"A" * (k + 20) in seqs and b"C" * 300 in seqs
    if k % 2 == 0:
        assert len(c.palindrome) == 1 and revcomp(c.palindrome[0]) == c.palindrome[0] and len(c.palindrome[0]) == k and c.palindrome[0] in seqs
    else:
        assert len(c.palindrome) == 2 and revcomp(c.palindrome[0]) == c.palindrome[1] != c.palindrome[0] and all(len(s) == k and s in seqs for s in c.palindrome)
    alt = c.alternating
    kinds = [forward_is_smaller(alt[i:i + k]) for i in range(len(alt) - k + 1)]
    assert alt in seqs and len(kinds) == (6 if k != 2 else 3) and None not in kinds and all(kinds[i] != kinds[i + 1] for i in range(len(kinds) - 1))
    if k >= 2:
        assert len(c.t_to_a) == 3 and all(s in seqs and len(s) == k for s in c.t_to_a)
        for s in c.t_to_a:
            v = index_of(s)
            assert v >> (2 * k - 2) == 3 and v & 3 == 0
    # the facts the device tests rely on
    plain, canonical = kcount_of_np(arr(data), k), kcount_of_np(arr(data), k, True)
    assert plain.skipped > 0 and plain.short_lines >= 2 and plain.skipped == canonical.skipped
    assert plain.table[4 ** k - 1] >= 21 and plain.table[0] >= 21 and canonical.table[0] == plain.table[0] + plain.table[4 ** k - 1]
    assert plain.table[index_of(b"C" * k)] >= 300 - k + 1
    v = index_of(c.palindrome[0])
    if k % 2 == 0:
        assert revcomp_index(v, k) == v and canonical.table[v] == plain.table[v] >= 1
    else:
        r = revcomp_index(v, k)
        assert r != v and canonical.table[min(v, r)] == plain.table[v] + plain.table[r] >= 2
    # a window starts at each of the 16 byte phases of a chunk at every pointer offset
    starts, tends = line_spans_np(arr(data))
    pos = np.concatenate([np.arange(s, e - k + 1) for s, e in zip(starts[1::4], tends[1::4]) if e - s >= k])
    for off in OFFSETS:
        assert set(((pos + off) % 16).tolist()) == set(range(16)), off
    # k = 5 and k = 6: the partial-copy layouts of the LDS counters (16 and 4 copies); one k-mer comes from lanes that differ in
    # lane & rmask, where the lane is the 16-byte chunk of the window's first byte, modulo 64
    if k in (5, 6):
        rmask = 15 if k == 5 else 3
        run = data.index(b"C" * 300)
        for off in OFFSETS:
            assert len({((run + off + i) // 16) & 63 & rmask for i in range(300 - k + 1)}) == rmask + 1


# ---- what the screen and normalize sweeps need -------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(8, 33))
def test_reads_hit_one_reference_both_and_none(k):
    c = cases(k)
    index = screen_index_of_np(c.refs, k)
    if k in (8, 32):
        assert same(index, screen_index_of(c.refs, k))
    assert index["refs"][0]["contigs"] == 4 and index["refs"][1]["contigs"] == 2 and all(r["shared"] > 0 and r["distinct"] > r["shared"] for r in index["refs"])
    assert max(len(line) for line in c.refs[0][1].split(b"\n")) == 70                 # wrapped at 70 columns
    assert index["keys"][0] == 3 and index["keys"][min(index_of(c.palindrome[0]), index_of(revcomp(c.palindrome[0])))] & 1
    w = screen_of_np(index, arr(c.fastq), min_hits=1)
    masks = {r[3] for r in w["recs"] if r[0] > 0}
    assert masks == {0, 1, 2, 3} and w["short_reads"] > 0 and w["skipped"] > 0 and 0 < w["reads_out"] < w["reads_in"]
    if k in (8, 32):
        assert same(w, screen_of(index, c.fastq, min_hits=1))
    crlf = fastq_of([(s, b"\r\n") for p in c.parts.values() for s, e in p], final=True)
    w = screen_of_np(index, arr(crlf), interleaved=True, min_hits=2, min_hit_pct=5)
    assert 0 < w["matched_pairs"] < w["pairs"] and w["multi_reads"] > 0


@pytest.mark.parametrize("k", range(13, 33))
def test_normalize_takes_every_class(k):
    data = cases(k).fastq
    for canonical in MODES:
        table = kcount_of_np(arr(data), k, canonical).table
        w = normalize_of(table, k, canonical, data, bins=12, **NORM_OPTS)
        assert set(w["classes"]) == {KEPT, NO_KMERS, LOW, HIGH}, (k, canonical)
        assert w["absent_kmers"] == 0 and w["weak_kmers"] > 0 and max(r[0] for r in w["recs"]) == 513 and w["hist"][11][0] > 0


# ---- counts past 32 bits: tests/_deep_counts_cases.py --------------------------------------------------------------------------------
def test_the_deep_table_is_arithmetic():
    """the formula against the checker on runs of a few dozen letters, then the identities of the real one"""
    small = ((b"A", 70), (b"T", 81), (b"C", 52), (b"G", 45))
    data = deep.HEAD + b"N".join(letter * n for letter, n in small) + deep.TAIL
    for k, canonical in deep.TABLES:
        w = kcount_of(data, k, canonical)
        assert w.table == deep.table_of(k, canonical, small) and w.skipped == 3 * k and (w.reads, w.lines, w.short_lines) == (1, 4, 0)
        table, s = deep.table_of(k, canonical), deep.summary_of(k, canonical)
        assert s["kmers"] == sum(table.values()) == sum(n - k + 1 for _, n in deep.RUNS) == s["windows"] - s["skipped"]
        assert s["windows"] == deep.LINE - k + 1 and s["distinct"] == len(table) == (2 if canonical else 4) and s["max_count"] > 2 ** 32
        assert [n > 2 ** 32 for _, n in deep.RUNS] == [True, True, False, False]
    assert deep.LINE == 2 ** 33 + 2 ** 31 + 2 ** 24 + 4096 + 8192 + 5 + 1 + 3 and 10 * 2 ** 30 < deep.INPUT_BYTES < 10.6 * 2 ** 30
    assert deep.table_of(32, False) == {0: 2 ** 32 + 4065, 2 ** 64 - 1: 2 ** 32 + 8161, index_of(b"C" * 32): 2 ** 31 - 26, index_of(b"G" * 32): 2 ** 24 - 30}
    assert deep.table_of(32, True) == {0: 2 ** 33 + 4065 + 8161, index_of(b"C" * 32): 2 ** 31 + 2 ** 24 - 56}
    assert [(x, at) for x, at, n in deep.run_offsets()][:2] == [(b"A", 6), (b"T", 6 + 2 ** 32 + 4096 + 1)]


@pytest.mark.parametrize("k,canonical", deep.TABLES)
def test_the_deep_reads_take_every_shape(k, canonical):
    table, data = deep.table_of(k, canonical), deep.fastq_reads(k)
    names = list(deep.reads_of(k))
    SAT = deep.SAT
    c_count, g_count = table[index_of(b"C" * k)], table[index_of((b"C" if canonical else b"G") * k)]
    # the count under k x C: 2^31 - (k - 6) in plain mode (bits 30 .. 3 set), with G's 2^24 on top and bit 31 set in canonical mode; either
    # way the select parts it from the saturated counts at bit 31
    assert c_count == 2 ** 31 + 6 - k + (2 ** 24 + 2 - k if canonical else 0) and (c_count >> 31 == 1) == canonical and c_count < SAT
    assert 2 ** 24 - 32 <= g_count < SAT and min(table[0], table[0 if canonical else 4 ** k - 1]) > 2 ** 32
    if (k, canonical) == (32, False):
        assert index_of(b"T" * k) == 2 ** 64 - 1                     # the key that has no slot: the table's counter of its own
    w = normalize_of(table, k, canonical, data)
    rec = dict(zip(names, w["recs"]))
    assert rec["all saturated, A"] == rec["all saturated, T"] == (11, SAT, SAT, 0)
    assert rec["saturated beside markers"] == (6 + 4 + 3, SAT, SAT, 0)
    assert rec["median C, maximum saturated"] == (4 + 7, c_count, c_count, 0)
    assert rec["median G"] == (7 + 4, g_count, g_count, 0)
    assert rec["median 0, maximum saturated"] == (3 + 9, 0, 0, 9)
    assert rec["all absent"] == (k + 9, 0, 0, k + 9)
    assert rec["long, median C"] == (4 * (301 - k) + 4 * (401 - k), c_count, c_count, 0) and rec["long, median C"][0] > 2048
    assert rec["long, median saturated"] == (4 * (501 - k) + 4 * (251 - k) + 41 - k, SAT, c_count, 0) and rec["long, median saturated"][0] > 2048
    assert w["recs"][len(names):] == [(1, SAT, SAT, 0)] * deep.UNITS and deep.UNITS >= 200 and len(data) < 30_000
    # the largest weak_below: every k-mer is weak, the saturated ones too
    weak = normalize_of(table, k, canonical, data, weak_below=deep.WEAK_BELOW_MAX)
    assert all(r[3] == r[0] for r in weak["recs"]) and weak["weak_kmers"] == weak["kmers"] > 5000
    # the keep rule at D = 2^32 - 2
    classes = {}
    for target in deep.TARGETS:
        for bins in (2, 64):
            got = normalize_of(table, k, canonical, data, target=target, seed=7 if target == 2 ** 31 else 0, bins=bins)
            classes[target] = got["classes"][len(names):]
            assert got["hist"][bins - 1][0] >= deep.UNITS + 4 and got["hist"][0][0] == 2
    assert set(classes[20]) == {HIGH} and set(classes[2 ** 32 - 1]) == {KEPT}
    assert set(classes[2 ** 31]) == {HIGH, KEPT} and 60 < classes[2 ** 31].count(KEPT) < deep.UNITS - 60
    assert [c["target"] for c in deep.CALLS[:3]] == list(deep.TARGETS) and {c["bins"] for c in deep.CALLS} == {2, deep.MAX_BINS}
    assert deep.CALLS[3]["target"] == 2 ** 31 and deep.CALLS[4]["weak_below"] == 2 ** 32 - 1

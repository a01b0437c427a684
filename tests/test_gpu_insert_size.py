"""fq-insert-size on the device (csrc/scfq_insert.hip) against the checkers of tests/_insert_size_check.py: the per-pair table, the
histogram and every field of the summary, compared with ==."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG
from _insert_size_check import (DEFAULTS, HIST_BINS, assert_result, cli_text, fastq, insert_of, insert_of_np, interleave, paired_block, planted,
                                random_dna, revcomp, same)
from test_gpu_hist_spec import make_fastq
from test_gpu_parity import to_dev

pytestmark = pytest.mark.gpu

SC = os.path.join(PKG, "sc")
PAIRS = os.path.join(GOLDEN, "pairs")
R1, R2, IL, R2GZ = (os.path.join(PAIRS, f) for f in ("r1.fq", "r2.fq", "interleaved.fq", "r2.fq.gz"))
SENTINEL = 0x5A5A5A5A
EXTRA = 3
WAVES = 4                      # pairs a block of the overlap kernel works on at a time (kIsWaves)
MAX_BLOCKS = 4096              # ... and the most blocks it starts: beyond WAVES * MAX_BLOCKS pairs a block makes a second round
EDGES = (0, 1, 29, 30, 31, 63, 64, 65, 127, 128, 129, 191, 192, 193, 511, 512)


class Table:
    """device memory for `cap` scfq_overlap_rec between sentinel entries"""

    def __init__(self, torch, cap):
        self.cap = cap
        self.t = torch.full((cap + 2 * EXTRA, 2), SENTINEL, dtype=torch.int32, device="cuda")
        self.ptr = self.t.data_ptr() + 8 * EXTRA
        torch.cuda.synchronize()

    def rows(self, pairs):
        """(offset, overlap, mismatches) of the first `pairs` entries; everything else still holds the sentinel"""
        h = self.t.cpu().numpy().astype(np.int64)
        assert (h[:EXTRA] == SENTINEL).all() and (h[EXTRA + pairs:] == SENTINEL).all(), "entries outside [0, pairs) were written"
        body = h[EXTRA:EXTRA + pairs]
        return np.stack([body[:, 0], body[:, 1] & 0xFFFF, (body[:, 1] >> 16) & 0xFFFF], axis=1)


def as_array(data):
    return None if data is None else np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data


def check_device(torch, scfq, d1, d2, params=None, ctx="", off1=0, off2=0, want=None, checker=insert_of_np, extra_cap=2):
    """the device entry point on d1 / d2 (d2 = None: interleaved) with a table of pairs + extra_cap entries"""
    a1, a2 = as_array(d1), as_array(d2)
    if want is None:
        want = checker(a1, a2, params or DEFAULTS)
    t1, p1 = to_dev(torch, a1, off1)
    t2, p2 = to_dev(torch, a2, off2) if a2 is not None else (None, None)
    tab = Table(torch, want["pairs"] + extra_cap)
    got = scfq.insert_size_device(p1, a1.size, p2, a2.size if a2 is not None else 0, params, tab.ptr, tab.cap)
    assert_result(got, want, (ctx, params, off1, off2), tab.rows(want["pairs"]))
    return want, got


def test_fixtures_every_entry_point(gpu, scfq):
    torch = gpu
    r1, r2, il = (open(p, "rb").read() for p in (R1, R2, IL))
    two, one = insert_of(r1, r2), insert_of(il)
    assert same(two, insert_of_np(as_array(r1), as_array(r2))) and same(one, insert_of_np(as_array(il)))
    assert (two["pairs"], two["overlapped"], two["not_overlapped"], two["read_through"]) == (88, 66, 22, 22)
    check_device(torch, scfq, r1, r2, want=two, ctx="device, two")
    check_device(torch, scfq, il, None, want=one, ctx="device, interleaved")
    for params in (None, (20, 2, 5)):
        w2 = two if params is None else insert_of(r1, r2, params)
        w1 = one if params is None else insert_of(il, None, params)
        for what, call, want in (("host, two", lambda t: scfq.insert_size_host(r1, r2, params, t.ptr, t.cap), w2),
                                 ("host, interleaved", lambda t: scfq.insert_size_host(il, None, params, t.ptr, t.cap), w1),
                                 ("file, two", lambda t: scfq.insert_size_file(R1, R2, params, t.ptr, t.cap), w2),
                                 ("file, gz", lambda t: scfq.insert_size_file(R1, R2GZ, params, t.ptr, t.cap), w2),
                                 ("file, interleaved", lambda t: scfq.insert_size_file(IL, None, params, t.ptr, t.cap), w1)):
            tab = Table(torch, 88)
            assert_result(call(tab), want, (what, params), tab.rows(88))
    # without a table; and a table that is too small says how many pairs there are
    assert_result(scfq.insert_size_file(R1, R2), two, "no table")
    assert_result(scfq.insert_size_host(il), one, "no table")
    tab = Table(torch, 87)
    with pytest.raises(scfq.ScfqError) as e:
        scfq.insert_size_file(R1, R2, None, tab.ptr, tab.cap)
    assert e.value.rc == scfq.SCFQ_EARG and "87" in str(e.value) and "88" in str(e.value)
    assert (e.value.summary.pairs, e.value.summary.reads1, e.value.summary.reads2, e.value.summary.lines1) == (88, 88, 88, 352)
    tab.rows(0)


def sc(*args):
    r = subprocess.run([SC, "fq-insert-size"] + list(args), capture_output=True, text=True, stdin=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_cli(gpu, scfq):
    r1, r2, il = (open(p, "rb").read() for p in (R1, R2, IL))
    two, one = insert_of(r1, r2), insert_of(il)
    header = "pairs\toverlapped\tpercent_overlapped\tmin\tmedian\tmean\tstd_dev\tmode\tmax\tread_through\tmismatch_rate"
    assert sc(R1, R2) == cli_text(two) == "88\t66\t75.0\t34\t167\t159.8484848484848\t65.28080195405784\t158\t269\t22\t0.004473503097040606\n"
    assert sc("-t", "-b", R1, R2, R1, R2GZ) == header + "\tbasename\n" + 2 * cli_text(two, suffix="\tr1.fq")
    assert sc("--interleaved", "-b", IL, IL) == 2 * cli_text(one, suffix="\tinterleaved.fq")
    assert sc("--dist", "-t", R1, R2) == "insert_size\tcount\n" + cli_text(two, dist=True)
    assert sc("--dist", "--interleaved", "-a", IL) == cli_text(one, dist=True, suffix="\t" + os.path.abspath(IL))
    strict = insert_of(r1, r2, (40, 0, 0))
    assert strict["overlapped"] < two["overlapped"]
    assert sc("--min-overlap=40", "--max-mismatches=0", "--max-mismatch-pct=0", R1, R2) == cli_text(strict)
    assert sc("--min-overlap=40", "--max-mismatches=0", "--max-mismatch-pct=0", "--dist", R1, R2) == cli_text(strict, dist=True)


def lone(la, lb):
    """mates whose only agreeing pair of bases is A[0] with C[lb - 1]: with no mismatch allowed d* = -(lb - 1), overlap 1"""
    return b"A" + b"C" * (la - 1), revcomp(b"G" * (lb - 1) + b"A")


def test_word_edges(gpu, scfq):
    """every length of EDGES against every other, the true offset at -(Lb-1), min_overlap - Lb, -64, -63, -1, 0, 1, 63, 64 and
    La - min_overlap where the lengths allow it"""
    rng = np.random.default_rng(71)
    m1, m2, truth = [], [], []
    for la in EDGES:
        for lb in EDGES:
            for d in (-(lb - 1), 30 - lb, -64, -63, -1, 0, 1, 63, 64, la - 30):
                if lb >= 1 and -(lb - 1) <= d <= la - 1:
                    a, b = planted(rng, la, lb, d + lb)
                    m1.append(a), m2.append(b), truth.append((la, lb, d))
            if min(la, lb) == 0:
                m1.append(random_dna(rng, la)), m2.append(random_dna(rng, lb)), truth.append((la, lb, None))
    want, _ = check_device(gpu, scfq, fastq(m1), fastq(m2), ctx="edges")
    assert want["pairs"] == len(truth) > 1500
    # the planted offset is found wherever its overlap is 30 or more
    for k, (la, lb, d) in enumerate(truth):
        ov = 0 if d is None else min(lb, la - d) - max(0, -d)
        if ov >= 30:
            assert want["recs"][k].tolist() == [d, ov, 0], (la, lb, d, want["recs"][k].tolist())
        elif max(la, lb) < 30:
            assert want["recs"][k].tolist() == [0, 0, 0], (la, lb, d)
    found = {tuple(r[:2]) for r, (la, lb, d) in zip(want["recs"].tolist(), truth) if r[1]}
    for d in (-482, -64, -63, -1, 0, 1, 63, 64, 482):
        assert any(f[0] == d for f in found), d
    check_device(gpu, scfq, fastq(interleave(m1, m2)), None, ctx="edges, interleaved")
    # d* at -(Lb - 1) and at La - 1 themselves: an overlap of one base
    l1, l2 = zip(*[lone(la, lb) for la in EDGES[1:] for lb in EDGES[1:]])
    want, _ = check_device(gpu, scfq, fastq(l1), fastq(l2), (1, 0, 0), "lone base")
    assert want["recs"].tolist() == [[-(lb - 1), 1, 0] for la in EDGES[1:] for lb in EDGES[1:]]
    want, _ = check_device(gpu, scfq, fastq([revcomp(b) for b in l2]), fastq([revcomp(a) for a in l1]), (1, 0, 0), "lone base, mirrored")
    assert want["recs"].tolist() == [[lb - 1, 1, 0] for la in EDGES[1:] for lb in EDGES[1:]]


def test_too_long(gpu, scfq):
    rng = np.random.default_rng(73)
    a, b = planted(rng, 512, 512, 600)
    long_a, long_b = planted(rng, 600, 600, 700)
    m1 = [a, a + b"A", a, long_a, long_a[:513], a, b"", a]
    m2 = [b, b, b"T" + b, long_b, b, long_b[:513], long_b, b]
    want, got = check_device(gpu, scfq, fastq(m1), fastq(m2), ctx="too long")
    assert want["recs"].tolist() == [[88, 424, 0]] + [[0, 0, 0xFFFF]] * 6 + [[88, 424, 0]]
    assert (got[0].too_long, got[0].overlapped, got[0].not_overlapped) == (6, 2, 0)
    check_device(gpu, scfq, fastq(interleave(m1, m2)), None, ctx="too long, interleaved")
    # a too-long line's bytes are not looked at: the same line of other letters, lengths kept, changes nothing
    other = [s if len(s) <= 512 else b"N" * len(s) for s in m1]
    assert same(want, dict(insert_of_np(as_array(fastq(other)), as_array(fastq(m2)))))


def test_parameters(gpu, scfq):
    rng = np.random.default_rng(79)
    m1, m2 = [], []
    for la, lb, ins, errs in ((512, 512, 512, 0), (512, 512, 512, 1), (512, 512, 513, 0), (150, 150, 200, 0), (150, 150, 200, 3), (150, 150, 200, 9),
                              (150, 150, 292, 0), (150, 150, 293, 1), (150, 150, 299, 0), (40, 60, 33, 0), (100, 100, 108, 2), (100, 100, 108, 30),
                              (8, 8, 8, 0), (8, 9, 10, 1), (1, 1, 1, 0), (1, 1, 1, 1), (150, 150, 1000, 0)):
        a, b = planted(rng, la, lb, ins) if ins < la + lb else (random_dna(rng, la), random_dna(rng, lb))
        a = bytearray(a)
        lo = max(0, ins - lb)
        for k in range(errs):                        # inside the overlap where there is one
            i = min(lo + 2 * k, la - 1)
            a[i] = ord("N")
        m1.append(bytes(a)), m2.append(b)
    d1, d2 = fastq(m1), fastq(m2)
    for params in ((1, 5, 20), (8, 5, 20), (512, 5, 20), (512, 0, 0), (30, 0, 20), (30, 5, 0), (30, 65535, 100), (1, 65535, 100), (1, 0, 100), (8, 2, 100)):
        want, got = check_device(gpu, scfq, d1, d2, params, "parameters")
        assert same(want, insert_of(d1, d2, params)), params
        assert (got[0].min_overlap, got[0].max_mismatches, got[0].max_mismatch_pct) == params
    w = insert_of(d1, d2, (512, 5, 20))
    assert w["recs"][:3].tolist() == [[0, 512, 0], [0, 512, 1], [0, 0, 0]] and w["overlapped"] == 2
    assert insert_of(d1, d2, (512, 0, 0))["overlapped"] == 1
    # with everything allowed every pair of non-empty reads overlaps, in the whole of the shorter one
    w = insert_of(d1, d2, (1, 65535, 100))
    assert w["overlapped"] == len(m1) and w["recs"][:, 1].tolist() == [min(len(a), len(b)) for a, b in zip(m1, m2)]


def test_planted_mismatches(gpu, scfq):
    rng = np.random.default_rng(83)
    m1, m2, recs = [], [], []
    for la, lb, d in ((200, 200, 5), (200, 200, -70), (200, 180, 0), (130, 200, -64), (200, 130, 64)):
        a, b = planted(rng, la, lb, d + lb)
        c = revcomp(b)
        lo, hi = max(0, -d), min(lb, la - d)
        ys = sorted({lo, hi - 1} | {y for y in (63, 64, 127, 128, 191, 192) if lo <= y < hi} |
                    {y - d for y in (63, 64, 127, 128, 191, 192) if lo <= y - d < hi})       # word edges of C and of A
        put = lambda s, i, ch: s[:i] + ch + s[i + 1:]
        for y in ys:
            for bad in (b"N", a[y + d:y + d + 1].lower(), b"\xc1", b"\x00"):
                m1.append(put(a, y + d, bad)), m2.append(b), recs.append([d, hi - lo, 1])
                m1.append(a), m2.append(revcomp(put(c, y, b"N"))[:lb - 1 - y] + bad + revcomp(put(c, y, b"N"))[lb - y:]), recs.append([d, hi - lo, 1])
                m1.append(put(a, y + d, bad)), m2.append(m2[-1]), recs.append([d, hi - lo, 1])     # both at one place: one mismatch
        for k in range(1, min(len(ys), 7) + 1):      # 1 .. 7 at once: six and seven are too many
            aa = a
            for y in ys[:k]:
                aa = put(aa, y + d, b"N")
            m1.append(aa), m2.append(b), recs.append([d, hi - lo, k] if k <= 5 else [0, 0, 0])
    for eol in (b"\n", b"\r\n"):
        want, _ = check_device(gpu, scfq, fastq(m1, eol), fastq(m2, eol), ctx=("mismatches", eol))
        assert want["recs"].tolist() == recs
        assert eol != b"\n" or same(want, insert_of(fastq(m1), fastq(m2)))
    d1, d2 = fastq(m1[:40], b"\r\n"), fastq(m2[:40])
    want = insert_of_np(as_array(d1), as_array(d2))
    for k in range(16):                              # every alignment of either input
        check_device(gpu, scfq, d1, d2, want=want, off1=k, off2=(5 * k + 3) % 16, ctx="alignment")
        check_device(gpu, scfq, d1, d2, want=want, off1=(7 * k + 1) % 16, off2=k, ctx="alignment")
    il = fastq(interleave(m1[:40], m2[:40]), b"\r\n")
    want = insert_of_np(as_array(il))
    for k in range(16):
        check_device(gpu, scfq, il, None, want=want, off1=k, ctx="alignment, interleaved")


def test_partition_edges(gpu, scfq):
    torch = gpu
    rng = np.random.default_rng(89)
    pool = [planted(rng, 60, 50, ins) for ins in rng.integers(1, 110, 64)]
    for pairs in (1, WAVES - 1, WAVES, WAVES + 1, 4 * WAVES + 1, WAVES * MAX_BLOCKS - 1, WAVES * MAX_BLOCKS, WAVES * MAX_BLOCKS + 1, 2 * WAVES * MAX_BLOCKS + 3):
        m1, m2 = zip(*[pool[(7 * k) % 64] for k in range(pairs)])
        want, _ = check_device(torch, scfq, fastq(m1), fastq(m2), ctx=("pairs", pairs))
        assert want["pairs"] == pairs and want["overlapped"] > 0 or pairs < 4
        if pairs < 100:
            check_device(torch, scfq, fastq(interleave(m1, m2)), None, ctx=("pairs, interleaved", pairs))
    m1, m2 = zip(*[pool[k] for k in range(21)])
    d1, d2 = fastq(m1), fastq(m2)
    full = insert_of(d1, d2)
    # reads1 != reads2 by one and by many, either way round
    for n1, n2 in ((21, 20), (20, 21), (21, 3), (3, 21), (21, 0), (0, 21), (0, 0), (1, 1)):
        want, got = check_device(torch, scfq, fastq(m1[:n1]), fastq(m2[:n2]), ctx=("reads", n1, n2))
        assert (got[0].pairs, got[0].unpaired, got[0].reads1, got[0].reads2) == (min(n1, n2), abs(n1 - n2), n1, n2)
        assert np.array_equal(want["recs"], full["recs"][:min(n1, n2)])
    # interleaved: an odd record at the end
    for n in (1, 2, 3, 41):
        want, got = check_device(torch, scfq, fastq(interleave(m1, m2)[:n]), None, ctx=("interleaved reads", n))
        assert (got[0].pairs, got[0].unpaired, got[0].reads1, got[0].reads2, got[0].lines2, got[0].input_bytes2) == (n // 2, n & 1, n, 0, 0, 0)
    # the last record truncated after each of its lines, with and without the final newline
    last = d2.rindex(b"@r20")
    cuts = [last + k for k in range(len(d2) - last + 1) if k == 0 or d2[last + k - 1:last + k] == b"\n" or d2[last + k:last + k + 1] == b"\n"]
    assert len(cuts) == 9
    for cut in cuts + [last + 20, len(d2) - 70]:
        for first, second in ((d1, d2[:cut]), (d2[:cut], d1)):
            want, _ = check_device(torch, scfq, first, second, ctx=("cut", cut - last))
            assert same(want, insert_of(first, second)), cut - last
    il = fastq(interleave(m1, m2))
    last = il.rindex(b"@r41")
    for cut in (last, last + 5, last + 30, len(il) - 60, len(il) - 1):
        want, _ = check_device(torch, scfq, il[:cut], None, ctx=("interleaved cut", cut - last))
        assert same(want, insert_of(il[:cut]))
    # nothing at all: the histogram is still written
    t, p = to_dev(torch, np.zeros(0, np.uint8))
    s, hist = scfq.insert_size_device(p, 0, p, 0)
    assert (s.pairs, s.reads1, s.lines1, s.unpaired, s.overlapped, s.min_overlap) == (0, 0, 0, 0, 0, 30) and not hist.any()
    s, hist = scfq.insert_size_host(b"", b"")
    assert s.pairs == 0 and not hist.any()
    s, hist = scfq.insert_size_host(d1, b"")
    assert (s.pairs, s.unpaired, s.reads1, s.reads2, s.input_bytes1, s.input_bytes2) == (0, 21, 21, 0, len(d1), 0) and not hist.any()


def test_ties(gpu, scfq):
    m1 = [b"ACGT" * 15, b"A" * 100, b"A" * 60, b"A" * 40, b"ACGT" * 128, b"AC" * 100, b"G" * 512, b"A" * 64]
    m2 = [revcomp(b"ACGT" * 10), b"T" * 60, b"T" * 100, b"A" * 40, revcomp(b"ACGT" * 128), revcomp(b"CA" * 100), b"C" * 512, b"T" * 65]
    want, _ = check_device(gpu, scfq, fastq(m1), fastq(m2), ctx="ties")
    assert want["recs"].tolist() == [[20, 40, 0], [40, 60, 0], [0, 60, 0], [0, 0, 0], [0, 512, 0], [1, 199, 0], [0, 512, 0], [0, 64, 0]]
    assert same(want, insert_of(fastq(m1), fastq(m2)))
    # equal overlap and equal mismatches: the larger offset
    want, _ = check_device(gpu, scfq, fastq([b"ACGT" * 15]), fastq([revcomp(b"ACGT" * 4 + b"ACTT" + b"ACGT" * 5)]), ctx="ties, one mismatch")
    assert want["recs"].tolist() == [[20, 40, 1]]
    check_device(gpu, scfq, fastq(m1), fastq(m2), (1, 65535, 100), "ties, everything allowed", checker=insert_of)


def test_contention(gpu, scfq):
    """20 000 pairs of one insert: one bin, one set of sums"""
    rng = np.random.default_rng(97)
    a, b = planted(rng, 150, 150, 222)
    pairs = 20_000
    d1, d2 = fastq([a]) * pairs, fastq([b]) * pairs
    want, got = check_device(gpu, scfq, d1, d2, ctx="contention")
    s, hist = got
    assert {int(k): int(hist[k]) for k in np.flatnonzero(hist)} == {222: pairs}
    assert (s.overlapped, s.not_overlapped, s.read_through, s.overlap_bases, s.mismatches) == (pairs, 0, 0, 78 * pairs, 0)
    assert (s.insert_sum, s.insert_sq_sum, s.min_insert, s.median_insert, s.mode_insert, s.max_insert) == (222 * pairs, 222 * 222 * pairs, 222, 222, 222, 222)
    assert want["recs"].tolist() == [[72, 78, 0]] * pairs


def test_a_long_line_among_short_pairs(gpu, scfq):
    rng = np.random.default_rng(101)
    mates = [planted(rng, 100, 100, 150) for _ in range(9)]
    big = random_dna(rng, 3_000_000)
    m1 = [m[0] for m in mates[:4]] + [big] + [m[0] for m in mates[4:]]
    m2 = [m[1] for m in mates[:4]] + [mates[0][1]] + [m[1] for m in mates[4:]]
    want, got = check_device(gpu, scfq, fastq(m1), fastq(m2), ctx="3 MB line in R1")
    assert want["recs"].tolist() == [[50, 50, 0]] * 4 + [[0, 0, 0xFFFF]] + [[50, 50, 0]] * 5 and got[0].too_long == 1
    want, got = check_device(gpu, scfq, fastq(m2), fastq(m1), ctx="3 MB line in R2")
    assert got[0].too_long == 1 and got[0].overlapped == 9
    check_device(gpu, scfq, fastq(interleave(m1, m2)), None, ctx="3 MB line, interleaved")


def test_repeatability_and_memory(gpu, scfq):
    torch = gpu
    rng = np.random.default_rng(103)
    r1, r2 = paired_block(rng, 3000, 100, 90)
    other = make_fastq(rng, 2000)
    t1, p1 = to_dev(torch, r1)
    t2, p2 = to_dev(torch, r2, 5)
    t3, p3 = to_dev(torch, other)
    want = insert_of_np(r1, r2)
    tabs = [Table(torch, 3000) for _ in range(3)]
    first = scfq.insert_size_device(p1, r1.size, p2, r2.size, None, tabs[0].ptr, 3000)
    assert_result(first, want, "first", tabs[0].rows(3000))
    before = scfq.lib().scfq_device_bytes_now()
    again = scfq.insert_size_device(p1, r1.size, p2, r2.size, None, tabs[1].ptr, 3000)
    scfq.cycles_device(p3, other.size, 100)
    scfq.insert_size_device(p3, other.size)
    third = scfq.insert_size_device(p1, r1.size, p2, r2.size, None, tabs[2].ptr, 3000)
    for got, tab in ((again, tabs[1]), (third, tabs[2])):
        assert bytes(first[0]) == bytes(got[0]) and first[1].tobytes() == got[1].tobytes()
        assert np.array_equal(tab.rows(3000), tabs[0].rows(3000))
    assert scfq.lib().scfq_device_bytes_now() == before
    assert len(scfq.insert_size_stages()) == 4 and scfq.insert_size_stages()[0] > 0


def test_many_pairs_against_the_numpy_checker(gpu, scfq):
    rng = np.random.default_rng(107)
    parts = [paired_block(rng, 66_000, la, lb) for la, lb in ((72, 72), (64, 90), (90, 60))]
    r1, r2 = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    want, got = check_device(gpu, scfq, r1, r2, ctx="198 000 pairs")
    assert want["pairs"] == 198_000 and 60_000 < want["overlapped"] < 120_000 and want["read_through"] > 20_000 and want["mismatches"] > 20_000
    assert np.count_nonzero(want["hist"]) > 80

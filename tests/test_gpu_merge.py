"""fq-merge on the device (csrc/scfq_merge.hip) against the checkers of tests/_merge_check.py: the three outputs compared with ==, byte
for byte, every field of the statistics, and the bytes around every output buffer."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG
from _insert_size_check import DEFAULTS, fastq, interleave, paired_block, planted, random_dna, revcomp
from _merge_check import OUTPUTS, STATS_HEADER, assert_stats, merge_of, merge_of_np, same, stat, stats_text, with_random_qualities
from test_gpu_parity import to_dev

pytestmark = pytest.mark.gpu

SC = os.path.join(PKG, "sc")
PAIRS = os.path.join(GOLDEN, "pairs")
R1, R2, IL, R2GZ = (os.path.join(PAIRS, f) for f in ("r1.fq", "r2.fq", "interleaved.fq", "r2.fq.gz"))
GOLD = tuple(os.path.join(PAIRS, f) for f in ("merged.fq", "unmerged1.fq", "unmerged2.fq"))
SENTINEL = 0xA5
GUARD = 256
G = 32                         # pairs of a group: a wave of the write kernel, an entry of the scans (kMgGroup)
WAVES = 4                      # groups of a block of the write kernel (kMgWaves); its grid is not capped
P1_WAVES, P1_MAX_BLOCKS = 4, 4096      # the overlap kernel's: beyond their product a block of P1 makes a second round
EDGES = (1, 29, 30, 31, 63, 64, 65, 127, 128, 129, 511, 512)
HEADERS = (1, 3, 4, 5, 15, 16, 17, 300)


class Out:
    """device memory for `cap` bytes between sentinel bytes, `off` bytes past a 256-byte boundary"""

    def __init__(self, torch, cap, off=0):
        self.cap, self.off = cap, off
        self.t = torch.full((2 * GUARD + off + cap,), SENTINEL, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 256 == 0
        self.ptr = self.t.data_ptr() + GUARD + off
        torch.cuda.synchronize()

    def arg(self):
        return (self.ptr, self.cap)

    def bytes(self, n):
        """the first n bytes; everything else still holds the sentinel"""
        h = self.t.cpu().numpy()
        lo = GUARD + self.off
        assert (h[:lo] == SENTINEL).all() and (h[lo + n:] == SENTINEL).all(), "bytes outside [0, %d) were written" % n
        return h[lo:lo + n].tobytes()


def as_array(data):
    return None if data is None else np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data


def check_device(torch, scfq, d1, d2, params=None, q0=33, ctx="", offs=(0, 0), out_offs=(0, 0, 0), want=None, checker=merge_of_np, extra=7, sizing=True):
    """the device entry point on d1 / d2 (d2 = None: interleaved): the sizing call, then outputs of the reported sizes + extra bytes"""
    a1, a2 = as_array(d1), as_array(d2)
    if want is None:
        want = checker(a1, a2, params or DEFAULTS, q0)
    t1, p1 = to_dev(torch, a1, offs[0])
    t2, p2 = to_dev(torch, a2, offs[1]) if a2 is not None else (None, None)
    n2 = a2.size if a2 is not None else 0
    if sizing:
        assert_stats(scfq.merge_device(p1, a1.size, p2, n2, params, q0), want, (ctx, "sizing"))
    outs = [Out(torch, len(want[k]) + extra, o) for k, o in zip(OUTPUTS, out_offs)]
    if a2 is None:
        outs[2] = None
    got = scfq.merge_device(p1, a1.size, p2, n2, params, q0, *[o.arg() if o else None for o in outs])
    assert_stats(got, want, (ctx, params, q0, offs, out_offs))
    for k, o in zip(OUTPUTS, outs):
        if o:
            have = o.bytes(len(want[k]))
            if have != want[k]:
                at = next(i for i in range(min(len(have), len(want[k]))) if have[i] != want[k][i])
                raise AssertionError((ctx, k, "differs at byte", at, have[max(0, at - 40):at + 40], want[k][max(0, at - 40):at + 40]))
    return want, got


def file_call(scfq, tmp_path, p1, p2, params=None, q0=33, which=(True, True, True)):
    """scfq_merge_files into three files; returns (stats, the three contents or None)"""
    paths = [tmp_path / ("out%d.fq" % k) for k in range(3)]
    fds = [os.open(str(p), os.O_WRONLY | os.O_CREAT | os.O_TRUNC) if w else -1 for p, w in zip(paths, which)]
    try:
        s = scfq.merge_file(p1, p2, params, q0, *fds)
    finally:
        for fd in fds:
            if fd >= 0:
                os.close(fd)
    return s, [p.read_bytes() if w else None for p, w in zip(paths, which)]


def test_fixtures_every_entry_point(gpu, scfq, tmp_path):
    torch = gpu
    r1, r2, il = (open(p, "rb").read() for p in (R1, R2, IL))
    two, one = merge_of(r1, r2), merge_of(il)
    assert same(two, merge_of_np(as_array(r1), as_array(r2))) and same(one, merge_of_np(as_array(il)))
    assert tuple(two[k] for k in OUTPUTS) == tuple(open(p, "rb").read() for p in GOLD)
    assert (two["pairs"], two["merged_pairs"], two["not_overlapped"]) == (88, 66, 22)
    check_device(torch, scfq, r1, r2, want=two, ctx="device, two")
    check_device(torch, scfq, il, None, want=one, ctx="device, interleaved")
    for params, q0 in ((None, 33), ((20, 2, 5), 64)):
        w2 = two if params is None else merge_of(r1, r2, params, q0)
        w1 = one if params is None else merge_of(il, None, params, q0)
        s, m, u1, u2 = scfq.merge_host(r1, r2, params, q0)
        assert_stats(s, w2, "host, two")
        assert (m, u1, u2) == tuple(w2[k] for k in OUTPUTS)
        s, m, u1, u2 = scfq.merge_host(il, None, params, q0)
        assert_stats(s, w1, "host, interleaved")
        assert (m, u1, u2) == (w1["merged"], w1["unmerged1"], None)
        # host outputs with room to spare, and only one of them asked for
        s, m, u1, u2 = scfq.merge_host(r1, r2, params, q0, caps=(None, len(w2["unmerged1"]) + 9, None))
        assert_stats(s, w2, "host, one output")
        assert (m, u1, u2) == (None, w2["unmerged1"], None)
        for what, a, b, want in (("file, two", R1, R2, w2), ("file, gz", R1, R2GZ, w2), ("file, interleaved", IL, None, w1)):
            s, outs = file_call(scfq, tmp_path, a, b, params, q0, (True, True, b is not None))
            assert_stats(s, want, what)
            assert outs[0] == want["merged"] and outs[1] == want["unmerged1"] and (b is None or outs[2] == want["unmerged2"]), what
        s, outs = file_call(scfq, tmp_path, R1, R2, params, q0, (False, False, True))
        assert_stats(s, w2, "file, one output")
        assert outs == [None, None, w2["unmerged2"]]
        assert_stats(scfq.merge_file(R1, R2GZ, params, q0), w2, "file, no output")
    # an output that is one byte too small: SCFQ_EARG that names it, the statistics complete, no byte written anywhere
    t1, p1 = to_dev(torch, as_array(r1))
    t2, p2 = to_dev(torch, as_array(r2), 3)
    for k, name in enumerate(OUTPUTS):
        outs = [Out(torch, len(two[o]) - (1 if o == name else 0), 1 + j) for j, o in enumerate(OUTPUTS)]
        with pytest.raises(scfq.ScfqError) as e:
            scfq.merge_device(p1, len(r1), p2, len(r2), None, 33, *[o.arg() for o in outs])
        assert e.value.rc == scfq.SCFQ_EARG and name in str(e.value), (name, str(e.value))
        assert str(len(two[name])) in str(e.value) and str(len(two[name]) - 1) in str(e.value), str(e.value)
        assert_stats(e.value.stats, two, ("too small", name))
        for o in outs:
            assert o.bytes(0) == b""
        with pytest.raises(scfq.ScfqError) as e:
            scfq.merge_host(r1, r2, caps=tuple(len(two[o]) - (1 if o == name else 0) for o in OUTPUTS))
        assert e.value.rc == scfq.SCFQ_EARG and name in str(e.value)
        assert_stats(e.value.stats, two, ("too small, host", name))
    ti, pi = to_dev(torch, as_array(il))
    outs = [Out(torch, len(one["merged"]), 0), Out(torch, len(one["unmerged1"]) - 1, 0)]
    with pytest.raises(scfq.ScfqError) as e:
        scfq.merge_device(pi, len(il), None, 0, None, 33, outs[0].arg(), outs[1].arg())
    assert e.value.rc == scfq.SCFQ_EARG and "unmerged1" in str(e.value)
    assert_stats(e.value.stats, one, "too small, interleaved")
    assert outs[0].bytes(0) == b"" and outs[1].bytes(0) == b""


def named_fastq(seqs, quals, names, eol=b"\n"):
    return b"".join(b"@" + n + eol + s + eol + b"+" + eol + q + eol for n, s, q in zip(names, seqs, quals))


def header_of(k, i):
    """a header text of HEADERS[k % 8] bytes behind the '@'... the '@' included: 1 is the '@' alone"""
    ln = HEADERS[k % len(HEADERS)]
    return (b"%d" % i).ljust(ln - 1, b"x")[:ln - 1]


def random_quals(rng, ln):
    return rng.integers(ord("!"), ord("I") + 1, ln, dtype=np.uint8).tobytes()


def spoil(rng, a, b, d, k):
    """up to three places inside the overlap of a planted pair changed, so that every row of the table occurs: a substitution in mate 1, an
    N in mate 2, an N in both at one place (few enough for the defaults where the overlap is 30 or more)"""
    la, lb = len(a), len(b)
    lo, hi = max(0, d), min(la, d + lb)                     # the overlap in positions of the merged read
    if hi - lo < 30:
        return a, b
    a, b = bytearray(a), bytearray(b)
    x1, x2, x3 = (int(v) for v in rng.integers(lo, hi, 3))
    if k % 2 == 0:
        a[x1] = ord("ACGT"[("ACGT".index(chr(a[x1])) + 1 + k % 3) % 4])
    if k % 3 == 0:
        b[lb - 1 - (x2 - d)] = ord("N")
    if k % 5 == 0:
        a[x3] = ord("N")
        b[lb - 1 - (x3 - d)] = ord("N")
    return bytes(a), bytes(b)


@pytest.fixture(scope="module")
def edge_pairs():
    """every length of EDGES against every other, the true offset at -(Lb-1), 30 - Lb, -64, -63, -1, 0, 1, 63, 64 and La - 30 where the
    lengths allow it; header lengths in turn; random qualities; the checker's result, computed once"""
    rng = np.random.default_rng(211)
    m1, m2, q1, q2, names = [], [], [], [], []
    for la in EDGES:
        for lb in EDGES:
            for d in (-(lb - 1), 30 - lb, -64, -63, -1, 0, 1, 63, 64, la - 30):
                if -(lb - 1) <= d <= la - 1:
                    a, b = planted(rng, la, lb, d + lb)
                    a, b = spoil(rng, a, b, d, len(m1))
                    names.append(header_of(len(m1), len(m1)))
                    m1.append(a), m2.append(b), q1.append(random_quals(rng, la)), q2.append(random_quals(rng, lb))
    r1, r2 = named_fastq(m1, q1, names), named_fastq(m2, q2, names)
    return r1, r2, merge_of_np(as_array(r1), as_array(r2)), (m1, m2, q1, q2, names)


def test_word_and_run_edges(gpu, scfq, edge_pairs):
    r1, r2, want, _ = edge_pairs
    assert want["pairs"] > 1000 and want["merged_pairs"] > 400 and want["not_overlapped"] > 100
    assert want["took_mate1"] > 0 and want["took_mate2"] > 0 and want["neither_valid"] > 0
    check_device(gpu, scfq, r1, r2, want=want, ctx="edges")


def test_word_and_run_edges_interleaved_and_crlf(gpu, scfq, edge_pairs):
    _, _, want, (m1, m2, q1, q2, names) = edge_pairs
    il = named_fastq(interleave(m1, m2), interleave(q1, q2), interleave(names, names))
    wi = merge_of_np(as_array(il))
    assert wi["merged"] == want["merged"] and stat(wi, "merged") == stat(want, "merged")
    check_device(gpu, scfq, il, None, want=wi, ctx="edges, interleaved", sizing=False)
    # "\r\n" inputs: the outputs are the same bytes, in "\n"
    c1, c2 = named_fastq(m1, q1, names, b"\r\n"), named_fastq(m2, q2, names, b"\r\n")
    wc = dict(want, input_bytes1=len(c1), input_bytes2=len(c2))
    assert same(wc, merge_of_np(as_array(c1), as_array(c2)))
    check_device(gpu, scfq, c1, c2, want=wc, ctx="edges, crlf", sizing=False)
    # ... and without the final newline, and with a final "\r" that is no line end
    wc = merge_of_np(as_array(c1[:-2]), as_array(c2[:-1]))
    check_device(gpu, scfq, c1[:-2], c2[:-1], want=wc, ctx="edges, crlf, cut", sizing=False)


def small_mixed(rng):
    """six pairs: merged ones of three shapes and unmerged ones, header lengths differing"""
    m1, m2 = [], []
    for la, lb, ins in ((100, 100, 150), (70, 90, 60), (33, 35, 36), (120, 80, 100)):
        a, b = planted(rng, la, lb, ins)
        m1.append(a), m2.append(b)
    m1 += [random_dna(rng, 50), random_dna(rng, 61)]
    m2 += [random_dna(rng, 50), random_dna(rng, 47)]
    order = [0, 4, 1, 2, 5, 3]
    m1, m2 = [m1[k] for k in order], [m2[k] for k in order]
    names = [b"p" * (k + 1) for k in range(6)]
    return (named_fastq(m1, [random_quals(rng, len(s)) for s in m1], names), named_fastq(m2, [random_quals(rng, len(s)) for s in m2], names))


def test_alignment(gpu, scfq):
    """one small input at all 16 alignments of each input buffer and of each output buffer"""
    rng = np.random.default_rng(223)
    r1, r2 = small_mixed(rng)
    want = merge_of(r1, r2)
    assert (want["merged_pairs"], want["not_overlapped"]) == (4, 2)
    il = b"".join(x for pair in zip(split_records(r1), split_records(r2)) for x in pair)
    wi = merge_of(il)
    for off in range(16):
        check_device(gpu, scfq, r1, r2, want=want, offs=(off, 0), ctx="input 1", sizing=False)
        check_device(gpu, scfq, r1, r2, want=want, offs=(3, off), ctx="input 2", sizing=False)
        for k in range(3):
            out_offs = [5, 9, 2]
            out_offs[k] = off
            check_device(gpu, scfq, r1, r2, want=want, out_offs=tuple(out_offs), ctx="output %d" % k, sizing=False)
        check_device(gpu, scfq, il, None, want=wi, offs=(off, 0), out_offs=(15 - off, off, 0), ctx="interleaved", sizing=False)


def split_records(data):
    lines = data.split(b"\n")[:-1]
    return [b"".join(x + b"\n" for x in lines[k:k + 4]) for k in range(0, len(lines), 4)]


def test_disagreements_and_ns_at_word_edges(gpu, scfq):
    rng = np.random.default_rng(227)
    la, lb, d = 200, 180, 50                                  # the overlap: positions 50 .. 199 of mate 1, 0 .. 149 of C
    m1, m2 = [], []
    places = sorted({63, 64, 127, 128} | {y + d for y in (63, 64, 127, 128)} | {d, la - 1})
    flip = lambda ch: ord("ACGT"[("ACGT".index(chr(ch)) + 2) % 4])
    for x in places:
        for kind in ("sub1", "sub2", "n1", "n2", "both"):
            a, b = (bytearray(s) for s in planted(rng, la, lb, d + lb))
            yb = lb - 1 - (x - d)
            if kind == "sub1":
                a[x] = flip(a[x])
            elif kind == "sub2":
                b[yb] = flip(b[yb])
            if kind in ("n1", "both"):
                a[x] = ord("N")
            if kind in ("n2", "both"):
                b[yb] = ord("N")
            m1.append(bytes(a)), m2.append(bytes(b))
    names = [b"e%d" % k for k in range(len(m1))]
    r1 = named_fastq(m1, [random_quals(rng, la) for _ in m1], names)
    r2 = named_fastq(m2, [random_quals(rng, lb) for _ in m2], names)
    want = merge_of(r1, r2)
    assert want["merged_pairs"] == len(m1) == 50 and want["mismatches"] == 50
    assert want["took_mate1"] + want["took_mate2"] == 20 and want["neither_valid"] == 10 and min(want["took_mate1"], want["took_mate2"]) > 0
    check_device(gpu, scfq, r1, r2, want=want, ctx="word edges")
    check_device(gpu, scfq, r1, r2, q0=64, checker=merge_of, ctx="word edges, 64", sizing=False)


def short_pairs(rng, count, pattern):
    """`count` pairs of 40-base mates: pattern(k) says whether pair k overlaps (by 35)"""
    hit, miss = planted(rng, 40, 40, 45), (random_dna(rng, 40), random_dna(rng, 40))
    m = [hit if pattern(k) else miss for k in range(count)]
    qa, qb = random_quals(rng, 40), random_quals(rng, 40)
    names = [b"%d" % k for k in range(count)]
    return named_fastq([p[0] for p in m], [qa] * count, names), named_fastq([p[1] for p in m], [qb] * count, names)


def test_partitions(gpu, scfq):
    rng = np.random.default_rng(229)
    counts = (1, G - 1, G, G + 1, WAVES * G - 1, WAVES * G, WAVES * G + 1)
    for count in counts:
        for what, pattern in (("all", lambda k: True), ("none", lambda k: False), ("alternating", lambda k: k % 2 == 0), ("groups", lambda k: (k // G) % 2 == 1)):
            r1, r2 = short_pairs(rng, count, pattern)
            want = merge_of_np(as_array(r1), as_array(r2))
            assert stat(want, "merged") == sum(1 for k in range(count) if pattern(k)), (count, what)
            check_device(gpu, scfq, r1, r2, want=want, ctx=(count, what), sizing=False)
    # a count at which a block of the overlap kernel makes a second round (the write kernel's grid is not capped), interleaved as well
    count = P1_WAVES * P1_MAX_BLOCKS + G + 1
    r1, r2 = short_pairs(rng, count, lambda k: k % 3 != 1)
    want, _ = check_device(gpu, scfq, r1, r2, ctx="second round")
    assert stat(want, "merged") == count - (count + 1) // 3
    # reads1 != reads2 either way round; an odd interleaved record
    r1, r2 = short_pairs(rng, 70, lambda k: k % 4 != 0)
    recs1, recs2 = split_records(r1), split_records(r2)
    for a, b in ((r1, b"".join(recs2[:41])), (b"".join(recs1[:33]), r2)):
        want, got = check_device(gpu, scfq, a, b, ctx="uneven")
        assert got.unpaired == 70 - got.pairs > 0
    il = b"".join(interleave(recs1, recs2)[:77])
    want, got = check_device(gpu, scfq, il, None, ctx="odd interleaved")
    assert (got.pairs, got.unpaired) == (38, 1)
    # empty inputs
    for a, b in ((b"", b""), (b"", None), (r1, b""), (b"", r2), (b"\n", b"\n")):
        want, got = check_device(gpu, scfq, a, b, checker=merge_of, ctx="empty")
        assert got.merged_bytes == 0


def test_truncated_last_record(gpu, scfq):
    """the last record cut after each of its lines, with and without a final newline, on either input and interleaved"""
    rng = np.random.default_rng(233)
    r1, r2 = short_pairs(rng, G + 2, lambda k: k != 5)
    last1, last2 = split_records(r1)[-1], split_records(r2)[-1]
    cuts = []
    for last in (last1, last2):
        ends = [i + 1 for i, ch in enumerate(last) if ch == 10]           # behind each of the four lines
        cuts.append([len(last) - e for e in ends[:3]] + [len(last) - e + 1 for e in ends] + [len(last) - ends[0] - 7])
    for drop in cuts[0]:
        check_device(gpu, scfq, r1[:len(r1) - drop], r2, checker=merge_of, ctx=("cut 1", drop), sizing=False)
    for drop in cuts[1]:
        check_device(gpu, scfq, r1, r2[:len(r2) - drop], checker=merge_of, ctx=("cut 2", drop), sizing=False)
        check_device(gpu, scfq, r1[:len(r1) - cuts[0][1]], r2[:len(r2) - drop], checker=merge_of, ctx=("cut both", drop), sizing=False)
    il = b"".join(interleave(split_records(r1), split_records(r2)))
    for drop in cuts[1]:
        check_device(gpu, scfq, il[:len(il) - drop], None, checker=merge_of, ctx=("cut interleaved", drop), sizing=False)
    # the merged pair itself cut short: its quality line is missing or partial
    r1, r2 = short_pairs(rng, 3, lambda k: True)
    for drop in (1, 2, 20, 41, 42, 43):
        want, _ = check_device(gpu, scfq, r1, r2[:len(r2) - drop], checker=merge_of, ctx=("merged, cut", drop), sizing=False)
        assert stat(want, "merged") == 3
        check_device(gpu, scfq, r1[:len(r1) - drop], r2, checker=merge_of, q0=64, ctx=("merged, cut 1", drop), sizing=False)


def test_too_long_pairs_land_unmerged_verbatim(gpu, scfq):
    rng = np.random.default_rng(239)
    hit = planted(rng, 100, 100, 150)
    long_a, long_b = planted(rng, 513, 100, 550)
    big = random_dna(rng, 3_000_000)
    m1 = [hit[0]] * 4 + [long_a, hit[0], big] + [hit[0]] * 3
    m2 = [hit[1]] * 4 + [long_b, hit[1], revcomp(big[:200])] + [hit[1]] * 3
    names = [b"t%d" % k for k in range(len(m1))]
    r1 = named_fastq(m1, [b"I" * len(s) for s in m1], names)
    r2 = named_fastq(m2, [b"5" * len(s) for s in m2], names)
    want, got = check_device(gpu, scfq, r1, r2, ctx="too long")
    assert (got.too_long, got.merged, got.not_overlapped) == (2, 8, 0)
    recs1 = split_records(r1)
    assert want["unmerged1"] == recs1[4] + recs1[6] and len(want["unmerged1"]) > 6_000_000
    il = b"".join(interleave(recs1, split_records(r2)))
    check_device(gpu, scfq, il, None, ctx="too long, interleaved", sizing=False)
    check_device(gpu, scfq, r1.replace(b"\n", b"\r\n"), r2, ctx="too long, crlf", sizing=False)


def test_parameters(gpu, scfq, edge_pairs):
    torch = gpu
    r1, r2, base, _ = edge_pairs
    everything, _ = check_device(torch, scfq, r1, r2, (1, 65535, 100), ctx="everything merges", sizing=False)
    lens = [(len(a), len(b)) for a, b in zip(*edge_pairs[3][:2])]
    assert stat(everything, "merged") == everything["pairs"] and everything["unmerged1"] == b""
    strict, _ = check_device(torch, scfq, r1, r2, (512, 0, 0), ctx="strict", sizing=False)
    assert 0 < stat(strict, "merged") <= sum(1 for la, lb in lens if la == lb == 512)
    q64, _ = check_device(torch, scfq, r1, r2, None, 64, ctx="phred 64", sizing=False)
    assert q64["merged"] != base["merged"] and len(q64["merged"]) == len(base["merged"]) and q64["unmerged1"] == base["unmerged1"]
    ri, _ = (open(p, "rb").read() for p in (IL, R1))
    check_device(torch, scfq, ri, None, (20, 2, 5), 64, checker=merge_of, ctx="fixture, interleaved", sizing=False)


def test_repeatability_and_memory(gpu, scfq):
    torch = gpu
    rng = np.random.default_rng(241)
    r1, r2 = paired_block(rng, 3000, 100, 90)
    r1, r2 = with_random_qualities(rng, r1), with_random_qualities(rng, r2)
    want = merge_of_np(r1, r2)
    t1, p1 = to_dev(torch, r1)
    t2, p2 = to_dev(torch, r2, 5)

    def call():
        outs = [Out(torch, len(want[k]), 1) for k in OUTPUTS]
        s = scfq.merge_device(p1, r1.size, p2, r2.size, None, 33, *[o.arg() for o in outs])
        return bytes(s), [o.bytes(len(want[k])) for o, k in zip(outs, OUTPUTS)]

    first = call()
    assert first[1] == [want[k] for k in OUTPUTS]
    second = call()
    before = scfq.lib().scfq_device_bytes_now()
    scfq.insert_size_device(p1, r1.size, p2, r2.size)
    third = call()
    assert first == second == third
    assert scfq.lib().scfq_device_bytes_now() == before
    assert len(scfq.merge_stages()) == 4 and scfq.merge_stages()[0] > 0


def test_one_larger_run(gpu, scfq):
    torch = gpu
    rng = np.random.default_rng(251)
    parts = [paired_block(rng, 20_000, la, lb) for la, lb in ((150, 150), (100, 151), (250, 250))]
    r1 = with_random_qualities(rng, np.concatenate([p[0] for p in parts]))
    r2 = with_random_qualities(rng, np.concatenate([p[1] for p in parts]))
    want, got = check_device(torch, scfq, r1, r2, ctx="larger", sizing=False)
    assert got.pairs == 60_000 and got.merged > 20_000 and got.not_overlapped > 5_000 and got.neither_valid > 0
    t1, p1 = to_dev(torch, r1)
    t2, p2 = to_dev(torch, r2)
    ins, _ = scfq.insert_size_device(p1, r1.size, p2, r2.size)
    assert (got.overlap_bases, got.mismatches, got.merged) == (ins.overlap_bases, ins.mismatches, ins.overlapped)
    assert got.merged_bases == ins.insert_sum


def sc(*args):
    r = subprocess.run([SC, "fq-merge"] + list(args), capture_output=True, stdin=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr
    return r.stdout, r.stderr.decode()


def test_cli(gpu, scfq, tmp_path):
    r1, r2, il = (open(p, "rb").read() for p in (R1, R2, IL))
    gold = [open(p, "rb").read() for p in GOLD]
    two, one = merge_of(r1, r2), merge_of(il)
    out, err = sc(R1, R2)
    assert out == gold[0] == two["merged"] and err == ""
    u1, u2 = tmp_path / "u1.fq", tmp_path / "u2.fq"
    out, err = sc("--unmerged1=%s" % u1, "--unmerged2=%s" % u2, "--stats", R1, R2GZ)
    assert out == gold[0] and u1.read_bytes() == gold[1] and u2.read_bytes() == gold[2]
    assert err == STATS_HEADER + "\n" + stats_text(two) + "\n"
    u = tmp_path / "u.fq"
    out, err = sc("--interleaved", "--unmerged=%s" % u, "--stats", IL)
    assert out == one["merged"] and u.read_bytes() == one["unmerged1"] and err.splitlines()[1] == stats_text(one)
    strict = merge_of(r1, r2, (40, 0, 0))
    assert stat(strict, "merged") < stat(two, "merged")
    out, err = sc("--min-overlap=40", "--max-mismatches=0", "--max-mismatch-pct=0", "--unmerged2=%s" % u2, R1, R2)
    assert out == strict["merged"] and u2.read_bytes() == strict["unmerged2"]
    out, _ = sc("--phred-offset=64", R1, R2)
    assert out == merge_of(r1, r2, q0=64)["merged"]
    # a reader of stdout that goes away ends the command quietly
    p = subprocess.Popen([SC, "fq-merge", R1, R2], stdout=subprocess.PIPE, stderr=subprocess.PIPE, stdin=subprocess.DEVNULL)
    p.stdout.close()
    assert p.wait(timeout=60) == 0 and p.stderr.read() == b""
    p.stderr.close()

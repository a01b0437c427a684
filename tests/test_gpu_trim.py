"""fq-trim on the device (csrc/scfq_trim.hip) against the checkers of tests/_trim_check.py: the outputs compared with ==, byte for byte,
every field of the statistics, and the bytes around every output buffer."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG
from _insert_size_check import paired_block, planted, random_dna
from _merge_check import with_random_qualities
from _trim_check import DEFAULT_PROBES, STATS_HEADER, assert_stats, check_identities, same, stats_text, trim_of, trim_of_np
from test_gpu_parity import to_dev

pytestmark = pytest.mark.gpu

SC = os.path.join(PKG, "sc")
TRIM = os.path.join(GOLDEN, "trim")
R1, R2, IL, R2GZ = (os.path.join(TRIM, f) for f in ("r1.fq", "r2.fq", "interleaved.fq", "r2.fq.gz"))
GOLD = {k: os.path.join(TRIM, f) for k, f in (("single", "single.fq"), ("out1", "paired1.fq"), ("out2", "paired2.fq"), ("interleaved", "interleaved_out.fq"))}
FIXTURE = dict(poly_g=10, window_quality=20)       # tests/golden/trim/make_trim.py's PARAMS
ALL = dict(poly_g=5, window_quality=20)            # every step on
OFF = dict(no_adapters=True, no_overlap=True, min_length=0)      # every step off (poly-G and the window are off by default)
SENTINEL = 0xA5
GUARD = 256
G = 32                         # reads or pairs of a group: a wave of the write kernel, an entry of the scans (kTrGroup)
WAVES = 4                      # groups of a block of the write kernel, reads of a block of the decision kernel (kTrWaves)
P1_WAVES, P1_MAX_BLOCKS = 4, 4096      # the overlap kernel's and the decision kernel's: beyond their product a block makes a second round
LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 511, 512, 513)
HEADERS = (1, 15, 16, 17, 300)
UNIVERSAL = DEFAULT_PROBES[0]
LONG_ADAPTER = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCACGATCTCGTATGCCGTCTTCTGCTTG"


class Out:
    """device memory for `cap` bytes between sentinel bytes, `off` bytes past a 256-byte boundary"""

    def __init__(self, torch, cap, off=1):
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


def differ(ctx, name, have, want):
    if have != want:
        at = next((i for i in range(min(len(have), len(want))) if have[i] != want[i]), min(len(have), len(want)))
        raise AssertionError((ctx, name, "differs at byte", at, len(have), len(want), have[max(0, at - 40):at + 40], want[max(0, at - 40):at + 40]))


def check_device(torch, scfq, d1, d2=None, kw=None, ctx="", offs=(0, 0), out_offs=(1, 3), want=None, checker=trim_of_np, extra=7):
    """the device entry point on d1 / d2: the sizing call, then outputs of the reported sizes + extra bytes between sentinels"""
    kw = kw or {}
    a1, a2 = as_array(d1), as_array(d2)
    if want is None:
        want = checker(a1, a2, **kw) if checker is trim_of_np else checker(bytes(d1), None if d2 is None else bytes(d2), **kw)
    check_identities(want)
    opts = scfq.trim_opts(**kw)
    t1, p1 = to_dev(torch, a1, offs[0])
    t2, p2 = to_dev(torch, a2, offs[1]) if a2 is not None else (None, None)
    n2 = a2.size if a2 is not None else 0
    assert_stats(scfq.trim_device(p1, a1.size, p2, n2, opts), want, (ctx, "sizing"))
    outs = [Out(torch, len(want["out1"]) + extra, out_offs[0]), Out(torch, len(want["out2"]) + extra, out_offs[1]) if a2 is not None else None]
    got = scfq.trim_device(p1, a1.size, p2, n2, opts, *[o.arg() if o else None for o in outs])
    assert_stats(got, want, (ctx, kw, offs, out_offs))
    for k, o in zip(("out1", "out2"), outs):
        if o:
            differ(ctx, k, o.bytes(len(want[k])), want[k])
    return want, got


def file_call(scfq, tmp_path, p1, p2, opts, which=(True, True)):
    """scfq_trim_files into two files; returns (stats, the two contents or None)"""
    paths = [tmp_path / ("out%d.fq" % k) for k in range(2)]
    fds = [os.open(str(p), os.O_WRONLY | os.O_CREAT | os.O_TRUNC) if w else -1 for p, w in zip(paths, which)]
    try:
        s = scfq.trim_file(p1, p2, opts, *fds)
    finally:
        for fd in fds:
            if fd >= 0:
                os.close(fd)
    return s, [p.read_bytes() if w else None for p, w in zip(paths, which)]


def every_entry_point(torch, scfq, tmp_path, r1, r2, kw, want, ctx, files=None):
    """device, host and file calls on one input; files: the paths that hold r1 and r2 (made in tmp_path when None)"""
    interleaved = bool(kw.get("interleaved"))
    check_device(torch, scfq, r1, r2, kw, want=want, ctx=(ctx, "device"))
    opts = scfq.trim_opts(**kw)
    s, o1, o2 = scfq.trim_host(r1, r2, opts)
    assert_stats(s, want, (ctx, "host"))
    assert o1 == want["out1"] and (o2 == want["out2"] if r2 is not None else o2 is None), (ctx, "host")
    if files is None:
        files = [tmp_path / "in1.fq", tmp_path / "in2.fq" if r2 is not None else None]
        for p, d in zip(files, (r1, r2)):
            if p is not None:
                p.write_bytes(bytes(d))
    s, outs = file_call(scfq, tmp_path, str(files[0]), None if files[1] is None else str(files[1]), opts, (True, r2 is not None))
    assert_stats(s, want, (ctx, "file"))
    assert outs[0] == want["out1"] and (r2 is None or outs[1] == want["out2"]), (ctx, "file", interleaved)


def test_fixtures_every_entry_point(gpu, scfq, tmp_path):
    torch = gpu
    r1, r2, il = (open(p, "rb").read() for p in (R1, R2, IL))
    gold = {k: open(p, "rb").read() for k, p in GOLD.items()}
    single, two, one = trim_of(r1, **FIXTURE), trim_of(r1, r2, **FIXTURE), trim_of(il, interleaved=True, **FIXTURE)
    assert same(two, trim_of_np(as_array(r1), as_array(r2), **FIXTURE)) and same(one, trim_of_np(as_array(il), interleaved=True, **FIXTURE))
    assert (single["out1"], two["out1"], two["out2"], one["out1"]) == (gold["single"], gold["out1"], gold["out2"], gold["interleaved"])
    assert min(two[k] for k in ("cut_overlap", "cut_adapter", "cut_polyg", "cut_quality", "dropped_reads")) > 0
    every_entry_point(torch, scfq, tmp_path, r1, None, FIXTURE, single, "single", (R1, None))
    every_entry_point(torch, scfq, tmp_path, r1, r2, FIXTURE, two, "two", (R1, R2))
    every_entry_point(torch, scfq, tmp_path, r1, r2, FIXTURE, two, "two, gz", (R1, R2GZ))
    every_entry_point(torch, scfq, tmp_path, il, None, dict(FIXTURE, interleaved=True), one, "interleaved", (IL, None))
    opts = scfq.trim_opts(**FIXTURE)
    # only one output asked for; none at all
    s, o1, o2 = scfq.trim_host(r1, r2, opts, caps=(None, len(two["out2"]) + 9))
    assert_stats(s, two, "host, one output")
    assert (o1, o2) == (None, two["out2"])
    s, outs = file_call(scfq, tmp_path, R1, R2, opts, (False, True))
    assert_stats(s, two, "file, one output")
    assert outs == [None, two["out2"]]
    assert_stats(scfq.trim_file(R1, R2GZ, opts), two, "file, no output")
    assert len(scfq.trim_stages()) == 4
    # an output that is one byte too small: SCFQ_EARG that names it, the statistics complete, no byte written anywhere
    t1, p1 = to_dev(torch, as_array(r1))
    t2, p2 = to_dev(torch, as_array(r2), 3)
    for name in ("out1", "out2"):
        outs = [Out(torch, len(two[o]) - (1 if o == name else 0), 1 + 2 * j) for j, o in enumerate(("out1", "out2"))]
        with pytest.raises(scfq.ScfqError) as e:
            scfq.trim_device(p1, len(r1), p2, len(r2), opts, *[o.arg() for o in outs])
        assert e.value.rc == scfq.SCFQ_EARG and name in str(e.value), (name, str(e.value))
        assert str(len(two[name])) in str(e.value) and str(len(two[name]) - 1) in str(e.value), str(e.value)
        assert_stats(e.value.stats, two, ("too small", name))
        for o in outs:
            assert o.bytes(0) == b""
        with pytest.raises(scfq.ScfqError) as e:
            scfq.trim_host(r1, r2, opts, caps=tuple(len(two[o]) - (1 if o == name else 0) for o in ("out1", "out2")))
        assert e.value.rc == scfq.SCFQ_EARG and name in str(e.value)
        assert_stats(e.value.stats, two, ("too small, host", name))
    ti, pi = to_dev(torch, as_array(il))
    out = Out(torch, len(one["out1"]) - 1, 5)
    with pytest.raises(scfq.ScfqError) as e:
        scfq.trim_device(pi, len(il), None, 0, scfq.trim_opts(interleaved=True, **FIXTURE), out.arg())
    assert e.value.rc == scfq.SCFQ_EARG and "out1" in str(e.value)
    assert_stats(e.value.stats, one, "too small, interleaved")
    assert out.bytes(0) == b""


def quals(rng, n, lo=30, hi=40):
    return (rng.integers(lo, hi + 1, n) + 33).astype(np.uint8).tobytes()


def fastq(seqs, quals_, names=None, eol=b"\n", plus=None):
    names = names or [b"r%d" % i for i in range(len(seqs))]
    plus = plus or [b"+"] * len(seqs)
    return b"".join(b"@" + n + eol + s + eol + p + eol + q + eol for n, s, q, p in zip(names, seqs, quals_, plus))


def shaped(rng, ln, kind):
    """a read of ln bases and its quality text: 0 plain, 1 an adapter (whole, or cut by the read's end) at a random place, 2 a G tail,
    3 quality that falls at a random place, 4 all of them"""
    s, q = bytearray(random_dna(rng, ln)), bytearray(quals(rng, ln))
    if ln and kind in (3, 4):
        at = int(rng.integers(0, ln))
        q[at:] = quals(rng, ln - at, 2, 12)
    if ln and kind in (2, 4):
        g = int(rng.integers(1, min(ln, 80) + 1))
        s[ln - g:] = b"G" * g
    if ln and kind in (1, 4):
        at = int(rng.integers(0, ln))
        s[at:] = LONG_ADAPTER[:ln - at] + s[at + len(LONG_ADAPTER):]
    return bytes(s), bytes(q)


def test_read_lengths(gpu, scfq):
    """every length of LENGTHS in every shape, as single-end reads and as mates of planted pairs"""
    rng = np.random.default_rng(311)
    seqs, qs = [], []
    for ln in LENGTHS:
        for kind in range(5):
            for _ in range(3):
                s, q = shaped(rng, ln, kind)
                seqs.append(s), qs.append(q)
    data = fastq(seqs, qs)
    want, got = check_device(gpu, scfq, data, None, ALL, ctx="lengths, single")
    assert got.too_long == 15 and min(got.cut_adapter, got.cut_polyg, got.cut_quality, got.short_reads) > 10
    assert same(want, trim_of(data, **ALL))
    check_device(gpu, scfq, data, None, dict(ALL, window=1, poly_g=1, min_adapter_overlap=1, min_length=0), ctx="lengths, single, smallest")
    m1, m2, q1, q2 = [], [], [], []
    for la in LENGTHS:
        for lb in LENGTHS:
            for ins in (max(la, lb) + 20, min(la, lb) - 7, 40):
                if la and lb and 0 < ins < la + lb and la <= 512 and lb <= 512:
                    a, b = planted(rng, la, lb, ins)
                else:
                    a, b = random_dna(rng, la), random_dna(rng, lb)
                m1.append(a), m2.append(b), q1.append(quals(rng, la, 15, 40)), q2.append(quals(rng, lb, 15, 40))
    r1, r2 = fastq(m1, q1), fastq(m2, q2)
    want, got = check_device(gpu, scfq, r1, r2, ALL, ctx="lengths, pairs")
    assert got.cut_overlap > 50 and got.too_long > 20 and got.overlapped_pairs > 50


def test_adapter_positions(gpu, scfq):
    rng = np.random.default_rng(313)
    probes31 = (random_dna(rng, 31), random_dna(rng, 32), random_dna(rng, 1))
    eight = tuple(random_dna(rng, int(n)) for n in (12, 20, 32, 7, 16, 31, 9, 25))
    for what, probes in (("default", None), ("1 31 32", probes31), ("eight", eight)):
        used = probes or DEFAULT_PROBES
        seqs = []
        for pr in used:
            for ln in (100, 200):
                for p in (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, ln - len(pr)):
                    if p + len(pr) <= ln:            # the whole probe at p, with one mismatch in every third read
                        s = bytearray(random_dna(rng, ln))
                        s[p:p + len(pr)] = pr
                        if len(seqs) % 3 == 2 and len(pr) >= 10:
                            k = p + int(rng.integers(0, len(pr)))
                            s[k] = ord("N") if len(seqs) % 2 else s[k] ^ 0x20      # N, or the right letter in lower case
                        seqs.append(bytes(s))
            for ln in (70, 66, 64, 130):             # a partial probe at the read's end, across a 64-base word where the lengths allow
                for t in range(1, min(len(pr), 12) + 1):
                    seqs.append(random_dna(rng, ln - t) + pr[:t])
        data = fastq(seqs, [quals(rng, len(s)) for s in seqs])
        kw = dict(probes=probes, min_length=0, min_adapter_overlap=1 if what == "1 31 32" else 3)
        want, got = check_device(gpu, scfq, data, None, kw, ctx=("adapters", what))
        assert got.cut_adapter > len(seqs) // 2 and all(got.adapter_reads[j] > 0 for j in range(len(used))), (what, list(got.adapter_reads))
        if what == "default":
            assert same(want, trim_of(data, **kw))
    # thresholds: t = min_adapter_overlap - 1 against t; one mismatch at t = 10 and at t = 9 with 10 percent; a tie between two probes
    body = b"ACCA" * 20
    cases = [body + UNIVERSAL[:4], body + UNIVERSAL[:5], body + UNIVERSAL[:4] + b"T" + UNIVERSAL[5:10], body + UNIVERSAL[:4] + b"T" + UNIVERSAL[5:9]]
    data = fastq(cases, [quals(rng, len(s)) for s in cases])
    want, got = check_device(gpu, scfq, data, None, dict(probes=(UNIVERSAL,)), checker=trim_of, ctx="thresholds")
    assert (got.cut_adapter, got.bases_adapter) == (2, 15)
    tie = (b"ACGTACGTAC", b"ACGTACGTACGG")
    data = fastq([body + tie[1]], [quals(rng, 92)])
    want, got = check_device(gpu, scfq, data, None, dict(probes=tie[::-1]), checker=trim_of, ctx="tie")
    assert list(got.adapter_reads)[:2] == [1, 0]
    want, got = check_device(gpu, scfq, data, None, dict(probes=tie), checker=trim_of, ctx="tie, other order")
    assert list(got.adapter_reads)[:2] == [1, 0] and got.bases_adapter == 12


def test_quality_window(gpu, scfq):
    rng = np.random.default_rng(317)
    for window in (1, 4, 32):
        seqs, qs = [], []
        for ln in (64, 67, 100, 130, 200):
            for p in (60, 61, 62, 63, 64, 65, 66):
                if p + window > ln:
                    continue
                for depth in (0, 1):             # the window at p is the first one under the threshold, by a little or by a lot
                    q = np.full(ln, 33 + 30, np.uint8)
                    q[p + window - 1:] = 33 + (29 if depth == 0 else 2)
                    seqs.append(random_dna(rng, ln)), qs.append(q.tobytes())
        # a sum that equals the threshold is no cut; a byte below the offset counts as a negative number
        q = np.full(80, 33 + 20, np.uint8)
        seqs.append(random_dna(rng, 80)), qs.append(q.tobytes())
        data = fastq(seqs, qs)
        kw = dict(no_adapters=True, window=window, min_length=0)
        want, got = check_device(gpu, scfq, data, None, dict(kw, window_quality=20), ctx=("window, equal", window))
        want, got = check_device(gpu, scfq, data, None, dict(kw, window_quality=30), ctx=("window", window))
        assert got.cut_quality >= len(seqs) - 1
        assert same(want, trim_of(data, **dict(kw, window_quality=30)))
    low = fastq([random_dna(rng, 70)] * 2, [b"h" * 66 + b"!" + b"h" * 3, (b"h" * 70)[:40]], plus=[b"+", b"+name"])
    for q0 in (33, 64):
        check_device(gpu, scfq, low, None, dict(no_adapters=True, window=8, window_quality=35, phred_offset=q0, min_length=0), checker=trim_of, ctx=("offset", q0))


def test_poly_g(gpu, scfq):
    rng = np.random.default_rng(331)
    seqs = []
    for ln in (64, 65, 100, 128, 129, 200, 512):
        for g in (1, 9, 10, 11, 36, 37, 63, 64, 65, 100, 128, 129, ln):
            if g <= ln:
                head = bytearray(random_dna(rng, ln - g))
                if head:
                    head[-1] = ord("A")
                seqs.append(bytes(head) + b"G" * g)
    seqs += [b"G" * 30 + b"g" + b"G" * 12, b"G" * 30 + b"N" + b"G" * 9]
    data = fastq(seqs, [quals(rng, len(s)) for s in seqs])
    kw = dict(no_adapters=True, poly_g=10, min_length=0)
    want, got = check_device(gpu, scfq, data, None, kw, ctx="poly-G")
    assert got.cut_polyg == sum(1 for s in seqs if s.endswith(b"G" * 10)) and same(want, trim_of(data, **kw))
    check_device(gpu, scfq, data, None, dict(kw, poly_g=512), ctx="poly-G, 512")
    check_device(gpu, scfq, data, None, dict(kw, poly_g=1, probes=(b"GGGG",), no_adapters=False, min_adapter_overlap=2), ctx="poly-G behind an adapter of G")


def test_read_counts(gpu, scfq):
    """the group of the write kernel and the four groups of its block: kept and dropped reads in every pattern"""
    rng = np.random.default_rng(337)
    keep, drop = shaped(rng, 50, 0), (b"ACGTA" + LONG_ADAPTER[:45], quals(rng, 50))
    cut = (random_dna(rng, 30) + LONG_ADAPTER[:20], quals(rng, 50))
    for count in (1, G - 1, G, G + 1, WAVES * G - 1, WAVES * G, WAVES * G + 1):
        for what, pattern in (("all", lambda k: 0), ("none", lambda k: 1), ("alternating", lambda k: k % 3), ("groups", lambda k: (k // G) % 2)):
            reads = [(keep, drop, cut)[pattern(k)] for k in range(count)]
            data = fastq([r[0] for r in reads], [r[1] for r in reads])
            want, got = check_device(gpu, scfq, data, None, {}, ctx=("count", count, what))
            assert got.dropped_reads == sum(1 for k in range(count) if pattern(k) == 1)
            other = [(keep, keep, drop)[pattern(k)] for k in range(count)]
            r2 = fastq([r[0] for r in other], [r[1] for r in other])
            check_device(gpu, scfq, data, r2, dict(no_overlap=True), ctx=("count, pairs", count, what))
    # empty inputs
    for a, b, kw in ((b"", None, {}), (b"", b"", {}), (b"", None, dict(interleaved=True)), (data, b"", {}), (b"", data, {}), (b"\n", None, {})):
        want, got = check_device(gpu, scfq, a, b, kw, checker=trim_of, ctx="empty")
        assert got.out2_bytes == 0


def short_pairs(rng, count, pattern):
    """`count` pairs of 40-base mates: pattern(k) says whether pair k is a fragment of 34 bases (read through by 6) or unrelated"""
    hit, miss = planted(rng, 40, 40, 34), (random_dna(rng, 40), random_dna(rng, 40))
    m = [hit if pattern(k) else miss for k in range(count)]
    qa, qb = quals(rng, 40), quals(rng, 40)
    names = [b"%d" % k for k in range(count)]
    return fastq([p[0] for p in m], [qa] * count, names), fastq([p[1] for p in m], [qb] * count, names)


def test_second_round_of_the_wave_per_read_kernels(gpu, scfq):
    count = P1_WAVES * P1_MAX_BLOCKS + 1
    r1, r2 = short_pairs(np.random.default_rng(347), count, lambda k: k % 3 != 1)
    want, got = check_device(gpu, scfq, r1, r2, dict(no_adapters=True), ctx="second round")
    assert got.cut_overlap == 2 * (count - (count + 1) // 3) and got.bases_overlap == 6 * got.cut_overlap


def split_records(data):
    lines = data.split(b"\n")[:-1]
    return [b"".join(x + b"\n" for x in lines[k:k + 4]) for k in range(0, len(lines), 4)]


def test_pairing(gpu, scfq):
    rng = np.random.default_rng(349)
    long_ = shaped(rng, 60, 0)
    short = (b"ACGT" + LONG_ADAPTER[:56], quals(rng, 60))
    big = (random_dna(rng, 600), quals(rng, 600))
    kinds = ((long_, long_), (short, long_), (long_, short), (short, short), (big, short), (short, big), (big, big), (big, long_))
    pairs = [kinds[k % len(kinds)] for k in range(2 * G + 5)]
    r1 = fastq([p[0][0] for p in pairs], [p[0][1] for p in pairs])
    r2 = fastq([p[1][0] for p in pairs], [p[1][1] for p in pairs])
    kw = dict(no_overlap=True)
    want, got = check_device(gpu, scfq, r1, r2, kw, checker=trim_of, ctx="one mate short")
    n = len(pairs)
    assert got.dropped_reads == 2 * sum(1 for p in pairs if short in p) and got.short_reads < got.dropped_reads and got.too_long > n // 4
    recs1, recs2 = split_records(r1), split_records(r2)
    for a, b in ((r1, b"".join(recs2[:41])), (b"".join(recs1[:33]), r2)):
        want, got = check_device(gpu, scfq, a, b, kw, checker=trim_of, ctx="uneven")
        assert got.unpaired == n - got.pairs > 0 and got.reads_in == 2 * got.pairs
    il = b"".join(x for pair in zip(recs1, recs2) for x in pair)
    check_device(gpu, scfq, il, None, dict(kw, interleaved=True), checker=trim_of, ctx="interleaved")
    il_odd = b"".join(split_records(il)[:2 * 38 + 1])
    want, got = check_device(gpu, scfq, il_odd, None, dict(kw, interleaved=True), checker=trim_of, ctx="odd interleaved")
    assert (got.pairs, got.unpaired, got.reads_in) == (38, 1, 76)


def test_record_shapes(gpu, scfq):
    rng = np.random.default_rng(353)
    seqs, qs, names, plus = [], [], [], []
    for k in range(3 * G + 3):
        s, q = shaped(rng, int(rng.integers(20, 140)), k % 5)
        ln = HEADERS[k % len(HEADERS)]
        names.append((b"%d" % k).ljust(ln - 1, b"x")[:ln - 1])
        plus.append(b"+" if k % 3 else b"+" + names[-1])
        if k % 7 == 3:
            q = q[:len(q) // 2]                  # LQ < L
        if k % 7 == 5:
            q = q + b"IIII"                      # LQ > L: the quality text is cut to the sequence's
        seqs.append(s), qs.append(q)
    data = fastq(seqs, qs, names, plus=plus)
    want, got = check_device(gpu, scfq, data, None, ALL, checker=trim_of, ctx="shapes")
    crlf = fastq(seqs, qs, names, eol=b"\r\n", plus=plus)
    wc = dict(want, input_bytes1=len(crlf))
    check_device(gpu, scfq, crlf, None, ALL, want=wc, ctx="shapes, crlf")
    assert same(wc, trim_of(crlf, **ALL))
    for cut in (1, 2):                           # no final newline; a final "\r" that is no line end
        check_device(gpu, scfq, crlf[:-cut], None, ALL, checker=trim_of, ctx=("shapes, crlf, cut", cut))
    check_device(gpu, scfq, data[:-1], None, OFF, checker=trim_of, ctx="no final newline, nothing cut")
    # the last record cut short after each of its lines, with and without the newline, alone and as a mate
    last = split_records(data)[-1]
    ends = [i + 1 for i, ch in enumerate(last) if ch == 10]
    for e in ends[:3]:
        for drop in (len(last) - e, len(last) - e + 1):
            for kw in (ALL, OFF):
                check_device(gpu, scfq, data[:len(data) - drop], None, kw, checker=trim_of, ctx=("cut short", drop))
            check_device(gpu, scfq, data, data[:len(data) - drop], dict(ALL, no_overlap=True), checker=trim_of, ctx=("cut short, mate 2", drop))
            check_device(gpu, scfq, data[:len(data) - drop], None, dict(OFF, interleaved=True), checker=trim_of, ctx=("cut short, interleaved", drop))
    # every alignment of the input and of the output
    small = b"".join(split_records(data)[:9])
    w = trim_of(small, **ALL)
    for off in range(16):
        check_device(gpu, scfq, small, None, ALL, want=w, offs=(off, 0), out_offs=(15 - off, 0), ctx=("alignment", off))


def test_too_long_reads_are_echoed(gpu, scfq):
    rng = np.random.default_rng(359)
    big = random_dna(rng, 700_000)
    seqs = [random_dna(rng, 100), random_dna(rng, 513), big, random_dna(rng, 30) + LONG_ADAPTER, b"ACG" + LONG_ADAPTER[:40], random_dna(rng, 512)]
    qs = [quals(rng, 100), quals(rng, 513) + b"III", b"I" * 5, quals(rng, 30 + len(LONG_ADAPTER)), quals(rng, 43), quals(rng, 512)]
    data = fastq(seqs, qs)
    want, got = check_device(gpu, scfq, data, None, {}, checker=trim_of, ctx="too long")
    assert (got.too_long, got.dropped_reads, got.cut_adapter) == (2, 1, 2)
    assert split_records(data)[1] + split_records(data)[2] in want["out1"]
    check_device(gpu, scfq, data.replace(b"\n", b"\r\n"), None, {}, checker=trim_of, ctx="too long, crlf")
    check_device(gpu, scfq, data, None, dict(interleaved=True), checker=trim_of, ctx="too long, interleaved")
    check_device(gpu, scfq, data, data, {}, checker=trim_of, ctx="too long, two")


@pytest.fixture(scope="module")
def planted_block():
    """a few thousand pairs in which every step has work: fragments around the read length (overlap, read-through into a real adapter), G
    tails, quality that falls; the checker's result, computed once"""
    rng = np.random.default_rng(367)
    r1, r2 = paired_block(rng, 3000, 100, 90)
    r1, r2 = with_random_qualities(rng, r1, 33 + 2, 33 + 40), with_random_qualities(rng, r2, 33 + 2, 33 + 40)
    a1, a2 = r1.reshape(3000, -1), r2.reshape(3000, -1)          # records of one length each: "@p\n" S "\n+\n" Q "\n"
    for k in range(0, 3000, 7):                                  # adapters in mate 1, whole and cut by the read's end
        at = int(rng.integers(20, 100))
        a1[k, 3 + at:3 + 100] = np.frombuffer((LONG_ADAPTER + b"A" * 50)[:100 - at], np.uint8)
    for k in range(3, 3000, 11):                                 # G tails in mate 2
        g = int(rng.integers(5, 40))
        a2[k, 3 + 90 - g:3 + 90] = ord("G")
    for k in range(5, 3000, 13):                                 # high quality all along: nothing for the window to find
        a1[k, 6 + 100:6 + 200] = ord("I")
        a2[k, 6 + 90:6 + 180] = ord("I")
    kw = dict(poly_g=5, window_quality=12, window=8, min_length=20)
    return r1, r2, kw, trim_of_np(r1, r2, **kw)


def test_every_step_in_one_run(gpu, scfq, tmp_path, planted_block):
    r1, r2, kw, want = planted_block
    for k in ("cut_overlap", "cut_adapter", "cut_polyg", "cut_quality", "dropped_reads", "reads_out"):
        assert want[k] >= 20, (k, want[k])
    assert sum(1 for v in want["adapter_reads"] if v) >= 1 and want["bases_dropped"] > 0
    every_entry_point(gpu, scfq, tmp_path, r1, r2, kw, want, "planted")
    gz = tmp_path / "r2.fq.gz"
    import gzip
    with gzip.open(gz, "wb") as f:
        f.write(r2.tobytes())
    (tmp_path / "r1.fq").write_bytes(r1.tobytes())
    s, outs = file_call(scfq, tmp_path, str(tmp_path / "r1.fq"), str(gz), scfq.trim_opts(**kw))
    assert_stats(s, want, "planted, gz")
    assert outs == [want["out1"], want["out2"]]
    recs1, recs2 = r1.reshape(3000, -1), r2.reshape(3000, -1)
    il = b"".join(a.tobytes() + b.tobytes() for a, b in zip(recs1, recs2))
    wi = trim_of_np(as_array(il), interleaved=True, **kw)
    assert wi["out1"] == b"".join(x for pair in zip(split_records(want["out1"]), split_records(want["out2"])) for x in pair)
    every_entry_point(gpu, scfq, tmp_path, il, None, dict(kw, interleaved=True), wi, "planted, interleaved")
    # twice the same, and no pool memory kept
    t1, p1 = to_dev(gpu, r1)
    t2, p2 = to_dev(gpu, r2, 5)
    opts = scfq.trim_opts(**kw)

    def call():
        outs = [Out(gpu, len(want[k]), 1) for k in ("out1", "out2")]
        s = scfq.trim_device(p1, r1.size, p2, r2.size, opts, *[o.arg() for o in outs])
        return bytes(s), [o.bytes(len(want[k])) for o, k in zip(outs, ("out1", "out2"))]

    first = call()
    before = scfq.lib().scfq_device_bytes_now()
    assert first == call() and scfq.lib().scfq_device_bytes_now() == before


def test_equivalences(gpu, scfq, planted_block):
    torch = gpu
    r1, r2, _, _ = planted_block
    # every step off and min_length = 0: the echo of every record, which for these records is the input
    want, got = check_device(torch, scfq, r1, r2, OFF, ctx="echo")
    assert want["out1"] == r1.tobytes() and want["out2"] == r2.tobytes() and got.bases_out == got.bases_in
    names = [b"n%d" % k for k in range(200)]
    seqs = [random_dna(np.random.default_rng(k), 20 + k) for k in range(200)]
    crlf = fastq(seqs, [b"I" * len(s) for s in seqs], names, eol=b"\r\n")[:-2]
    want, got = check_device(torch, scfq, crlf, None, OFF, checker=trim_of, ctx="echo, crlf")
    echoed, st = scfq.dedup_host(crlf)
    assert st.records_out == 200 and want["out1"] == echoed
    # only the overlap step: what fq-insert-size finds on the same buffers
    t1, p1 = to_dev(torch, r1)
    t2, p2 = to_dev(torch, r2)
    table = torch.zeros((3000, 2), dtype=torch.int32, device="cuda")
    ins, _ = scfq.insert_size_device(p1, r1.size, p2, r2.size, None, table.data_ptr(), 3000)
    rec = table.cpu().numpy()
    d, ov = rec[:, 0].astype(np.int64), rec[:, 1].astype(np.int64) & 0xFFFF
    s = d + 90
    removed = int((np.maximum(0, 100 - s) + np.maximum(0, 90 - s))[ov > 0].sum())
    got = scfq.trim_device(p1, r1.size, p2, r2.size, scfq.trim_opts(no_adapters=True, min_length=0))
    assert (got.overlapped_pairs, got.bases_overlap) == (ins.overlapped, removed) and removed > 0
    assert got.cut_overlap >= ins.read_through and got.cut_adapter == got.cut_polyg == got.cut_quality == 0


def sc(*args):
    r = subprocess.run([SC, "fq-trim"] + list(args), capture_output=True, stdin=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr
    return r.stdout, r.stderr.decode()


def test_cli(gpu, scfq, tmp_path):
    r1, r2, il = (open(p, "rb").read() for p in (R1, R2, IL))
    gold = {k: open(p, "rb").read() for k, p in GOLD.items()}
    flags = ("--poly-g=10", "--window-quality=20")
    out, err = sc(*flags, R1)
    assert out == gold["single"] and err == ""
    o1, o2 = tmp_path / "o1.fq", tmp_path / "o2.fq"
    out, err = sc(*flags, "--out1=%s" % o1, "--out2=%s" % o2, "--stats", R1, R2GZ)
    assert out == b"" and o1.read_bytes() == gold["out1"] and o2.read_bytes() == gold["out2"]
    assert err == STATS_HEADER + "\n" + stats_text(trim_of(r1, r2, **FIXTURE)) + "\n"
    out, err = sc(*flags, "--interleaved", "--stats", IL)
    assert out == gold["interleaved"] and err.splitlines()[1] == stats_text(trim_of(il, interleaved=True, **FIXTURE))
    kw = dict(probes=(b"AGATCGGAAGAGC", b"CTGTCTCTTATACACATCT"), min_adapter_overlap=3, adapter_mismatch_pct=20, window=6, window_quality=25, min_length=30,
              no_overlap=True, phred_offset=33, poly_g=12)
    out, err = sc("--adapter=truseq:AGATCGGAAGAGC", "--adapter=nextera:CTGTCTCTTATACACATCT", "--min-adapter-overlap=3", "--adapter-mismatch-pct=20", "--window=6",
                  "--window-quality=25", "--min-length=30", "--no-overlap-trim", "--phred-offset=33", "--poly-g=12", "--out1=%s" % o1, "--out2=%s" % o2, R1, R2)
    want = trim_of(r1, r2, **kw)
    assert o1.read_bytes() == want["out1"] and o2.read_bytes() == want["out2"] and want["out1"] != gold["out1"]
    out, _ = sc("--no-adapters", "--min-overlap=40", "--max-mismatches=0", "--max-mismatch-pct=0", "--interleaved", IL)
    assert out == trim_of(il, interleaved=True, no_adapters=True, min_overlap=40, max_mismatches=0, max_mismatch_pct=0)["out1"]
    # a reader of stdout that goes away ends the command quietly
    p = subprocess.Popen([SC, "fq-trim", R1], stdout=subprocess.PIPE, stderr=subprocess.PIPE, stdin=subprocess.DEVNULL)
    p.stdout.close()
    assert p.wait(timeout=60) == 0 and p.stderr.read() == b""
    p.stderr.close()

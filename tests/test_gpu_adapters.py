"""fq-adapters on the device (csrc/scfq_adapters.hip) against the checkers of tests/_adapters_check.py: every row, the tail, the total, the
hits and every field of the summary, compared with ==."""
import glob
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG
from _adapters_check import COLS, MAX_PROBES, adapters_of, adapters_of_np, assert_result, cli_text, row_of, same, totals_text
from _kmers_check import index_of
from test_gpu_hist_spec import make_fastq
from test_gpu_parity import random_fastq_like, to_dev

pytestmark = pytest.mark.gpu

SC = os.path.join(PKG, "sc")
SENTINEL = np.uint64(0xDEADBEEF12345678)
EXTRA = 3
BUILTIN = [("illumina_universal", "AGATCGGAAGAG"), ("illumina_small_rna_3p", "TGGAATTCTCGG"), ("illumina_small_rna_5p", "GATCGTCGGACT"),
           ("nextera", "CTGTCTCTTATA"), ("polya", "AAAAAAAAAAAA"), ("polyg", "GGGGGGGGGGGG"), ("solid_small_rna", "CGCCTTGGCCGT")]
BUILTIN_SEQS = [s for _, s in BUILTIN]
MIXED = ("A", "AC", "ACGT", "ACGTACGTACGTACGTA")


def fixed(s):
    """the fields of a summary that do not depend on cap, as bytes"""
    return bytes(np.array([s.reads, s.lines, s.input_bytes, s.n_probes, s.max_seq_len] + list(s.probe_len) + list(s.hits) + row_of(s.total),
                          dtype=np.uint64))


def check_call(call, want, probes, n, ctx, caps=None):
    """one entry point at every cap: call(cap or a rows array) -> (summary, rows)"""
    max_len = want[3]
    if caps is None:
        caps = sorted({0, 1, max(max_len - 1, 0), max_len, max_len + 3})
    ref = None
    for cap in caps:
        if cap == 0:
            got = call(0)
        else:
            buf = np.full((cap + EXTRA, COLS), SENTINEL, dtype=np.uint64)      # sentinel rows behind `positions` stay untouched
            got = call(buf[:cap])
            assert (buf[int(got[0].positions):] == SENTINEL).all(), (ctx, cap, "rows behind positions were written")
        assert_result(got, want, probes, cap, n, (ctx, "cap", cap))
        ref = ref or fixed(got[0])
        assert fixed(got[0]) == ref, (ctx, cap, "a cap-independent field depends on cap")


def check_buffer(torch, scfq, a, probe_sets, ctx, offset=0, host=False, checker=adapters_of_np, caps=None):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    t, ptr = to_dev(torch, a, offset)
    for probes in probe_sets:
        want = checker(a, probes)
        check_call(lambda cap: scfq.adapters_device(ptr, a.size, probes, cap), want, probes, a.size, (ctx, probes, "device"), caps)
        if host:
            check_call(lambda cap: scfq.adapters_host(a, probes, cap), want, probes, a.size, (ctx, probes, "host"), (0, want[3]))
    return want


def golden_files():
    files = sorted(glob.glob(os.path.join(GOLDEN, "*.fq")) + glob.glob(os.path.join(GOLDEN, "edge", "*.fq")))
    assert len(files) >= 30
    return files


@pytest.mark.parametrize("probes", [None, MIXED], ids=["builtin", "mixed"])
def test_golden_files_every_entry_point(gpu, scfq, probes):
    plist = BUILTIN_SEQS if probes is None else probes
    for path in golden_files():
        data = open(path, "rb").read()
        a = np.frombuffer(data, dtype=np.uint8)
        t, ptr = to_dev(gpu, a)
        want = adapters_of_np(a, plist)
        if len(data) < 20_000:
            assert same(adapters_of(data, plist), want), path
        caps = sorted({0, 1, max(want[3] - 1, 0), want[3], want[3] + 3})
        check_call(lambda cap: scfq.adapters_device(ptr, a.size, probes, cap), want, plist, a.size, (path, "device"))
        check_call(lambda cap: scfq.adapters_host(a, probes, cap), want, plist, a.size, (path, "host"), caps)
        check_call(lambda cap: scfq.adapters_file(path, probes, cap), want, plist, a.size, (path, "file"), caps)


def sc(*args):
    r = subprocess.run([SC, "fq-adapters"] + list(args), capture_output=True, text=True, stdin=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_cli(gpu, scfq):
    """Seen to fail now and then (two of five runs while this test was written): one of the processes that take all golden files
    ends with "a sequence line of 18446744073709551615 bytes", that is line_off[j + 1] == line_off[j] == 0 for a sequence line in
    the line index a file call got.  The same shape of process (`sc fq-cycles` over all golden files) failed once in
    tests/test_gpu_cycles.py in the same runs, and no in-process call of this file ever did; the cause is not found."""
    files = golden_files()
    arrays = [np.frombuffer(open(p, "rb").read(), dtype=np.uint8) for p in files]
    header = "position\t" + "\t".join(n for n, _ in BUILTIN) + "\tany\n"
    wants = [adapters_of_np(a, BUILTIN_SEQS) for a in arrays]
    # every file in one process, rows in argument order
    assert sc("-t", "-b", *files) == header[:-1] + "\tbasename\n" + "".join(cli_text(w, 7, suffix="\t" + os.path.basename(p)) for p, w in zip(files, wants))
    assert sc("--totals", *files) == "".join(totals_text(w, [n for n, _ in BUILTIN], BUILTIN_SEQS) for w in wants)
    custom = ["--adapter=four:ACGT", "--adapter=two:AC", "--adapter=long:ACGTACGTACGTACGTA"]
    plist = ["ACGT", "AC", "ACGTACGTACGTACGTA"]
    wants = [adapters_of_np(a, plist) for a in arrays]
    assert any(w[2][0] for w in wants)
    assert sc("--counts", "-b", *custom, *files) == "".join(cli_text(w, 3, counts=True, suffix="\t" + os.path.basename(p)) for p, w in zip(files, wants))
    assert sc("--max-positions=3", *custom, *files) == "".join(cli_text(w, 3, max_positions=3) for w in wants)
    assert sc("--totals", "-t", "-b", *custom, *files) == "adapter\tsequence\treads\treads_with\tpercent\thits\tbasename\n" + "".join(
        totals_text(w, ["four", "two", "long"], plist, "\t" + os.path.basename(p)) for p, w in zip(files, wants))
    # the literal rows
    many = os.path.join(GOLDEN, "edge", "many_short.fq")
    rest = "".join("%d\t100.0\t100.0\n" % p for p in range(2, 9))
    assert sc("--adapter=x:ACGT", many) == "1\t100.0\t100.0\n" + rest
    assert sc("--adapter=x:ACGT", "-t", "-b", "--counts", "--max-positions=2", many) == "position\tx\tany\tbasename\n1\t300\t300\tmany_short.fq\n2\t0\t0\tmany_short.fq\n"
    assert sc("--adapter=x:CGT", "--adapter=y:T", "--max-positions=3", many) == "1\t0.0\t0.0\t0.0\n2\t100.0\t0.0\t100.0\n3\t100.0\t0.0\t100.0\n>3\t100.0\t100.0\t100.0\n"
    assert sc("--adapter=x:CGT", "--adapter=y:T", "--max-positions=3", "--counts", many) == "1\t0\t0\t0\n2\t300\t0\t300\n3\t0\t0\t0\n>3\t0\t300\t0\n"
    assert sc("--adapter=x:ACGT", "--totals", many) == "x\tACGT\t300\t300\t100.0\t300\nany\t*\t300\t300\t100.0\t300\n"
    assert sc("--totals", "-b", many) == "".join("%s\t%s\t300\t0\t0.0\t0\tmany_short.fq\n" % (n, s) for n, s in BUILTIN + [("any", "*")])


def test_literal_tables(gpu, scfq):
    gold = lambda *parts: os.path.join(GOLDEN, *parts)
    firsts = lambda rows, col: {int(p): int(rows[p, col]) for p in np.flatnonzero(rows[:, col])}
    s, rows = scfq.adapters_file(gold("edge", "many_short.fq"), ["ACGT"], 100)
    assert (firsts(rows, 0), firsts(rows, 8), s.hits[0], s.total.first[0], s.total.any, s.reads, s.positions, s.max_seq_len) == ({0: 300}, {0: 300}, 300, 300, 300, 300, 8, 8)
    s, rows = scfq.adapters_file(gold("edge", "n_rich.fq"), ["ACGT"], 100)
    assert (firsts(rows, 0), s.hits[0], s.total.first[0]) == ({4: 1}, 1, 1)
    s, rows = scfq.adapters_file(gold("edge", "long_line_50k.fq"), ["ACGT"], 100)
    assert (firsts(rows, 0), s.hits[0], s.total.first[0], row_of(s.tail)) == ({0: 1}, 5000, 1, [0] * 9)
    s, rows = scfq.adapters_file(gold("sra.fq"), ["ACGT", "AC"], 100)
    assert (firsts(rows, 0), firsts(rows, 1), firsts(rows, 8), s.hits[1], s.total.first[1]) == ({13: 1}, {10: 1, 33: 1}, {10: 1, 33: 1}, 7, 2)
    # A C G T are legal quality bytes: nothing comes from the quality line, the header or the separator
    s, rows = scfq.adapters_host(b"@h\nAAAAAAAAAAAAAAAAAAAA\n+\nAAAAAAAAAAAAAAAAAAAA\n", None, 20)
    assert (firsts(rows, 4), firsts(rows, 8), list(s.hits), row_of(s.total)) == ({0: 1}, {0: 1}, [0, 0, 0, 0, 9, 0, 0, 0], [0, 0, 0, 0, 1, 0, 0, 0, 1])
    s, rows = scfq.adapters_host(b"@AAAAAAAAAAAAAAAA\nCCCC\n+AAAAAAAAAAAAAAAA\nIIII\n", ["AAAAAAAAAAAA", "AAAA"], 4)
    assert not rows.any() and list(s.hits) == [0] * 8 and row_of(s.total) == [0] * 9 and (s.reads, s.max_seq_len, s.positions) == (1, 4, 4)


def test_gzip_inputs(gpu, scfq):
    for name in ("dup.fq.gz", os.path.join("edge", "two_member.fq.gz")):
        path = os.path.join(GOLDEN, name)
        data = gzip.open(path, "rb").read()
        for probes in (None, MIXED):
            plist = BUILTIN_SEQS if probes is None else probes
            want = adapters_of(data, plist)
            check_call(lambda cap: scfq.adapters_file(path, probes, cap), want, plist, len(data), name)


@pytest.mark.parametrize("kind", ["uniform", "ascii", "dense_nl", "sparse_nl", "crlf"])
def test_random_buffers(gpu, scfq, kind):
    """tile and chunk boundaries inside windows: sizes around the 8 KiB step and its multiples; random bytes hold no long probes"""
    rng = np.random.default_rng(89)
    sets = (("A", "GC", "ACGTA"), ("T", "TT", "GGCAT"))
    for n in (1, 2, 15, 16, 17, 255, 4096, 32767, 32768, 32769, 65535, 65536, 65537, 1_000_000):
        a = random_fastq_like(rng, n, kind)
        caps = None if n <= 65537 else (0, 40)
        check_buffer(gpu, scfq, a, sets, (kind, n), host=n <= 4096, caps=caps)
        if n > 3:
            check_buffer(gpu, scfq, a[:-1], sets[:1], (kind, n, "last byte removed"), caps=caps)
            check_buffer(gpu, scfq, a[:2 * n // 3], sets[:1], (kind, n, "cut at two thirds"), caps=caps)


FAMILY = "AG" * 16                      # its prefixes overlap themselves two letters on
OTHER = "GAATGCAAGTCAGGATACGATTGACCAGTAAG"


def planted(rng, m, crlf, probe):
    """records of 80 letters of C T N (no letter of the probes' A and G) with `probe[:m]` written into them; returns the bytes"""
    eol = b"\r\n" if crlf else b"\n"
    L, p = 80, probe[:m].encode()
    ov = (probe[:m] + probe[m - 2:m] if probe is FAMILY and m >= 2 else probe[:m] + "C" + probe[:m][:1]).encode()

    def seq(*at):
        s = bytearray(rng.choice(np.frombuffer(b"CCTTN", dtype=np.uint8), L).tobytes())
        for pos, text in at:
            text = text[:L - pos]
            s[pos:pos + len(text)] = text
        return bytes(s)

    recs = [seq((0, p)),                                   # position 0
            seq((L - m, p)),                               # the last possible start
            seq((L - m + 1, p)),                           # one byte too far: cut by the line end, must not count
            seq((5, p), (5 + m + 3, p)),                   # twice
            seq((5, ov)),                                  # overlapping itself (length 1: twice, one letter apart)
            seq(), seq()]
    out = []
    for i, s in enumerate(recs):
        decoy = i >= 5                                     # the same text in the header, separator and quality line of other reads
        head = b"@" + (p * 2 if decoy else b"r%d" % i)
        plus = b"+" + (p if decoy else b"")
        qual = (p + b"I" * L)[:L] if decoy else b"I" * L
        out += [head, eol, s, eol, plus, eol, qual, eol]
    return b"".join(out)


@pytest.mark.parametrize("crlf", [False, True])
@pytest.mark.parametrize("m", [1, 12, 16, 17, 32])
def test_planted_adapters(gpu, scfq, m, crlf):
    rng = np.random.default_rng(100 + m)
    for probe in (FAMILY, OTHER):
        data = planted(rng, m, crlf, probe)
        a = np.frombuffer(data, dtype=np.uint8)
        p = probe[:m]
        want = check_buffer(gpu, scfq, a, ([p],), ("planted", m, crlf), host=True, checker=lambda b, pr: adapters_of(bytes(b), pr))
        rows, hits, total, max_len, lines = want
        assert (max_len, lines, total[0], total[8]) == (80, 28, 4, 4)
        firsts = {int(q): int(rows[q, 0]) for q in np.flatnonzero(rows[:, 0])}
        assert firsts == {0: 1, 80 - m: 1, 5: 2}, firsts
        assert hits[0] == (6 if probe is FAMILY or m == 1 else 5), hits
        for offset in (1, 9, 15):
            check_buffer(gpu, scfq, a, ([p],), ("planted", m, crlf, offset), offset=offset, caps=(0, 80))
    # all lengths in one input: a probe and its prefixes, the same probe twice, eight probes
    data = b"".join(planted(rng, k, crlf, probe) for k in (1, 12, 16, 17, 32) for probe in (FAMILY, OTHER))
    a = np.frombuffer(data, dtype=np.uint8)
    sets = ([FAMILY[:12], FAMILY[:m]], [OTHER[:m], OTHER[:m]],
            [FAMILY[:1], FAMILY[:12], FAMILY[:16], FAMILY[:17], FAMILY[:32], OTHER[:m], OTHER[:12], OTHER[:32]])
    check_buffer(gpu, scfq, a, sets, ("planted together", m, crlf), checker=lambda b, pr: adapters_of(bytes(b), pr), caps=(0, 7, 80))
    s, rows = scfq.adapters_host(data, [OTHER[:m], OTHER[:m]], 80)
    assert (rows[:, 0] == rows[:, 1]).all() and s.hits[0] == s.hits[1] > 0 and s.total.first[0] == s.total.first[1] == s.total.any


PAT = "".join("ACGT"[(p * 7 + p // 5 + p // 11) & 3] for p in range(40))


@pytest.mark.parametrize("m", [1, 4, 12, 32])
def test_every_line_length_and_alignment(gpu, scfq, m):
    """sequence lines of every length 0 .. 40 with mixed line ends, the device pointer at offsets 0 .. 15; the probe is the start of
    the lines' own pattern, which the header and quality lines hold too"""
    alpha, parts = b"ACGTNacgtX", []
    for rep in range(3):                   # any letter / the pattern with another letter every 17 / the pattern
        for L in range(41):
            eol = b"\r\n" if (L + rep) % 3 == 0 else b"\n"
            if rep == 0:
                seq = bytes(alpha[(p * p + L) % len(alpha)] for p in range(L))
            else:
                seq = bytes(alpha[4 + p % 6] if rep == 1 and (p + L) % 17 == 0 else ord(PAT[p]) for p in range(L))
            parts += [b"@" + PAT[:L % 23].encode(), eol, seq, eol, b"+" + PAT[:L % 7].encode(), eol, PAT[:L].encode(), eol]
    data = b"".join(parts)
    a = np.frombuffer(data, dtype=np.uint8)
    probes = [PAT[:m]]
    want = adapters_of(data, probes)
    assert same(want, adapters_of_np(a, probes)) and want[2][0] >= 41 - m and want[3] == 40
    for offset in range(16):
        t, ptr = to_dev(gpu, a, offset)
        check_call(lambda cap: scfq.adapters_device(ptr, a.size, probes, cap), want, probes, a.size, ("every line length", offset), caps=(0, 40))
    both = [PAT[:1], PAT[:4], PAT[:12], PAT[:32]]
    check_buffer(gpu, scfq, a, (both,), "every line length, four probes", offset=m % 16, caps=(0, 3, 40), checker=lambda b, pr: adapters_of(bytes(b), pr))


def test_degenerate_inputs(gpu, scfq):
    plain = lambda b, pr: adapters_of(bytes(b), pr)
    for data in (b"", b"\n", b"x", b"@h\n", b"@h\nACGT", b"@h\nACGT\r", b"@h\r\nACGT\r\n+", b"@h\nACGT\n+\nIIII\n@g\nAC", b"\r\n" * 1000,
                 b"@h\nACGT\n", b"@h\nA", b"@h\n\n+\n\n@g\n\r\n", b"ACGT", b"ACGT\nACGT\nACGT\nACGT\nACGT\nACGT"):
        a = np.frombuffer(data, dtype=np.uint8)
        check_buffer(gpu, scfq, a, (["ACGT"], ["A", "ACGT", "CGT", "ACGTA"], BUILTIN_SEQS), data[:16], host=True, checker=plain)
    s, rows = scfq.adapters_host(b"", ["ACGT"], 5)
    assert (s.reads, s.lines, s.input_bytes, s.n_probes, s.max_seq_len, s.positions, list(s.probe_len)) == (0, 0, 0, 1, 0, 0, [4, 0, 0, 0, 0, 0, 0, 0])
    assert rows.shape == (0, 9) and row_of(s.tail) == row_of(s.total) == [0] * 9 and list(s.hits) == [0] * 8
    for data, hits, first in ((b"@h\nACGT", 1, 0), (b"@h\nACGT\r", 1, 0), (b"@h\r\nACGT\r\n+", 1, 0), (b"@h\nACGT\n+\nIIII\n@g\nAC", 1, 0), (b"@h\n", 0, None),
                              (b"x", 0, None), (b"\n", 0, None), (b"\r\n" * 1000, 0, None), (b"ACGT", 0, None), (b"@h\nTACGT\n+\nACGT\n@ACGT\nACG\n+ACGT\nACGT", 1, 1)):
        s, rows = scfq.adapters_host(data, ["ACGT"], 8)
        assert (s.hits[0], s.total.first[0], s.total.any) == (hits, hits, hits), data
        assert [int(p) for p in np.flatnonzero(rows[:, 0])] == ([] if first is None else [first]), data


def test_long_lines(gpu, scfq):
    """lines that run through many steps and blocks: the first occurrence is found whichever block sees which occurrence"""
    rng = np.random.default_rng(21)
    probe = "AGAGAGAGAGAG"                 # (overlaps itself two letters on: the plants at 8190 and 8192 are both occurrences)
    L = 100_000
    plants = ((5, 8190, 8192, 65_530, 99_988), (8192, 65_530, 99_988), (99_988,))
    parts = []
    for r, at in enumerate(plants):
        seq = bytearray(rng.choice(np.frombuffer(b"CCTTTN", dtype=np.uint8), L).tobytes())
        for p in at:
            seq[p:p + 12] = probe.encode()
        parts += [b"@long%d\n" % r, bytes(seq), b"\n+\n", bytes(rng.choice(np.frombuffer(b"ACGTFI#", dtype=np.uint8), L)), b"\n"]
    a = np.frombuffer(b"".join(parts), dtype=np.uint8)
    for offset in (0, 5):
        want = check_buffer(gpu, scfq, a, ([probe], [probe[:1], probe, probe[:7]]), ("three records of 100 kB lines", offset), offset=offset,
                            caps=(0, 6, 8193, L))
    t, ptr = to_dev(gpu, a)
    s, rows = scfq.adapters_device(ptr, a.size, [probe], L)
    assert [int(p) for p in np.flatnonzero(rows[:, 0])] == [5, 8192, 99_988] and s.hits[0] == 9 and s.total.any == 3
    big = rng.choice(np.frombuffer(b"CCTTTN", dtype=np.uint8), 3_000_000)
    big[-12:] = np.frombuffer(probe.encode(), dtype=np.uint8)
    rec = np.concatenate([np.frombuffer(b"@big\n", dtype=np.uint8), big, np.frombuffer(b"\n+\n", dtype=np.uint8),
                          rng.choice(np.frombuffer(b"ACGT5#~", dtype=np.uint8), 2_999_990), np.frombuffer(b"\n", dtype=np.uint8)])
    a = np.concatenate([make_fastq(rng, 40), rec, make_fastq(rng, 40)])
    t, ptr = to_dev(gpu, a, 3)
    want = adapters_of_np(a, [probe])
    assert want[1][0] == 1 and want[2][0] == 1 and want[3] == 3_000_000
    check_call(lambda cap: scfq.adapters_device(ptr, a.size, [probe], cap), want, [probe], a.size, "a 3 MB line among short ones", (0, 1000, 3_000_000))
    s, _ = scfq.adapters_device(ptr, a.size, [probe], 1000)
    assert s.tail.first[0] == 1 and s.tail.any == 1


@pytest.mark.parametrize("probe", ["AAAAAAAAAAAA", "A"])
def test_contention(gpu, scfq, probe):
    """8 MiB of one letter: every chunk holds the probe, and all of them belong to one word of the first-occurrence table"""
    L, m = 8 << 20, len(probe)
    poly_a = np.concatenate([np.frombuffer(b"@a\n", dtype=np.uint8), np.full(L, ord("A"), np.uint8), np.frombuffer(b"\n+\n", dtype=np.uint8),
                             np.full(L, ord("A"), np.uint8), np.frombuffer(b"\n", dtype=np.uint8)])
    t, ptr = to_dev(gpu, poly_a, 7)
    for probes, col in (([probe], 0), (None, 4)) if m == 12 else (([probe], 0),):
        s, rows = scfq.adapters_device(ptr, poly_a.size, probes, 16)
        assert (s.hits[col], s.total.first[col], s.total.any, s.reads, s.lines, s.max_seq_len, s.positions) == (L - m + 1, 1, 1, 1, 4, L, 16)
        assert int(rows[0, col]) == 1 and int(rows[0, 8]) == 1 and int(rows.sum()) == 2 and row_of(s.tail) == [0] * 9
        assert sum(s.hits) == L - m + 1


def test_everything_hits(gpu, scfq):
    """20 000 short reads that all begin with the probe: every thread of the row pass adds to one counter"""
    probe = "AGATCGGAAGAG"
    rng = np.random.default_rng(3)
    tails = rng.choice(np.frombuffer(b"CT", dtype=np.uint8), (20_000, 18))
    data = b"".join(b"@r\n" + probe.encode() + bytes(tails[i]) + b"\n+\n" + b"I" * 30 + b"\n" for i in range(20_000))
    a = np.frombuffer(data, dtype=np.uint8)
    t, ptr = to_dev(gpu, a)
    for probes, col in (([probe], 0), (None, 0), (["CC", probe], 1)):
        s, rows = scfq.adapters_device(ptr, a.size, probes, 30)
        assert (int(rows[0, col]), int(rows[0, 8]), s.hits[col], s.total.first[col], s.total.any, s.reads) == (20_000,) * 6, probes
        assert int(rows[:, col].sum()) == 20_000 and int(rows[:, 8].sum()) == 20_000
    assert_result(scfq.adapters_device(ptr, a.size, ["CC", probe, "T"], 30), adapters_of_np(a, ["CC", probe, "T"]), ["CC", probe, "T"], 30, a.size, "everything hits")


@pytest.mark.parametrize("kind,seed", [(0, 20260101), (1, 20260103)])
def test_synthetic_64mib_against_the_counters(gpu, scfq, kind, seed):
    """no pass over the data outside the library: hits against scfq_cycles_buffer and the plain table of scfq_kmers_buffer"""
    torch = gpu
    plan = scfq.synth_plan(kind, seed, 64 << 20)
    buf = torch.empty(plan.bytes + 4096, dtype=torch.uint8, device="cuda")
    scfq.synth_device(kind, seed, plan.records, buf.data_ptr(), plan.bytes)
    ptr, n = buf.data_ptr(), plan.bytes
    cy, _ = scfq.cycles_device(ptr, n, 0)
    s, _ = scfq.adapters_device(ptr, n, ["A"], 0)
    assert s.hits[0] == cy.total.a and (s.reads, s.lines, s.max_seq_len) == (cy.reads, cy.lines, cy.max_seq_len)
    head = bytes(buf[:4096].cpu().numpy())
    read0 = head.split(b"\n")[1].rstrip(b"\r")
    assert len(read0) >= 40
    for k in (1, 4, 7, 8, 12):
        words = []
        for at in (0, 3, 11, 17, 26):
            w = read0[at:at + k]
            if set(w) <= set(b"ACGT") and w not in words:
                words.append(w)
        assert words
        ks, table = scfq.kmers_device(ptr, n, k, 0, True)
        cap = 64
        s, rows = scfq.adapters_device(ptr, n, [w.decode() for w in words], cap)
        for j, w in enumerate(words):
            assert s.hits[j] == int(table[index_of(w)]) > 0, (k, w)
            assert int(rows[:, j].sum()) + s.tail.first[j] == s.total.first[j] and s.hits[j] >= s.total.first[j] > 0, (k, w)
        assert int(rows[:, 8].sum()) + s.tail.any == s.total.any
        tf = list(s.total.first)[:len(words)]
        assert max(tf) <= s.total.any <= min(s.reads, sum(tf)), (k, tf, s.total.any)
        assert list(s.hits)[len(words):] == [0] * (8 - len(words)) and not rows[:, len(words):8].any()


@pytest.mark.parametrize("kind,seed", [(0, 20260101), (1, 20260103)])
def test_synthetic_16mib_against_numpy(gpu, scfq, kind, seed):
    torch = gpu
    plan = scfq.synth_plan(kind, seed, 16 << 20)
    buf = torch.empty(plan.bytes + 4096, dtype=torch.uint8, device="cuda")
    scfq.synth_device(kind, seed, plan.records, buf.data_ptr(), plan.bytes)
    a = buf[:plan.bytes].cpu().numpy()
    probes = ["ACG", "GATTC", "TTAGGC"]
    want = adapters_of_np(a, probes)
    assert all(h > 0 for h in want[1][:3])
    check_call(lambda cap: scfq.adapters_device(buf.data_ptr(), plan.bytes, probes, cap), want, probes, plan.bytes, ("synthetic", kind),
               (0, 100, min(want[3], 5000)))


def test_repeatability_and_memory(gpu, scfq):
    torch = gpu
    rng = np.random.default_rng(5)
    a, b = make_fastq(rng, 2000), make_fastq(rng, 1500, read_len=(400, 2500))
    ta, pa = to_dev(torch, a)
    tb, pb = to_dev(torch, b)
    for probes in (["ACG", "TTAG"], ["ACGTA", "C" * 17]):
        wa, wb = adapters_of_np(a, probes), adapters_of_np(b, probes)
        first = scfq.adapters_device(pa, a.size, probes, 200)
        assert_result(first, wa, probes, 200, a.size, "first buffer")
        before = scfq.lib().scfq_device_bytes_now()
        again = scfq.adapters_device(pa, a.size, probes, 200)
        assert bytes(first[0]) == bytes(again[0]) and first[1].tobytes() == again[1].tobytes()
        assert_result(scfq.adapters_device(pb, b.size, probes, 2500), wb, probes, 2500, b.size, "second buffer")
        scfq.kmers_device(pa, a.size, 7)
        third = scfq.adapters_device(pa, a.size, probes, 200)
        assert bytes(first[0]) == bytes(third[0]) and first[1].tobytes() == third[1].tobytes()
        assert scfq.lib().scfq_device_bytes_now() == before

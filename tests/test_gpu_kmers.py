"""fq-kmers on the device (csrc/scfq_kmers.hip) against the checkers of tests/_kmers_check.py: every entry of the table and every
field of the summary, compared with ==."""
import glob
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG
from _kmers_check import CANONICAL, assert_result, cli_text, index_of, kmers_of, kmers_of_np, totals_text
from test_gpu_hist_spec import make_fastq
from test_gpu_parity import random_fastq_like, to_dev

pytestmark = pytest.mark.gpu

SC = os.path.join(PKG, "sc")
SENTINEL = np.uint64(0xDEADBEEF12345678)
EXTRA = 3
_tables = {}


def table_buf(k):
    """one table per k with sentinel entries behind 4^k; a full call overwrites [0, 4^k) and nothing else"""
    if k not in _tables:
        _tables[k] = np.full(4 ** k + EXTRA, SENTINEL, dtype=np.uint64)
    return _tables[k]


def check_call(scfq, call, want, k, flags, n, ctx):
    """the sizing call and the full call of one entry point: call(table) -> (summary, table)"""
    s0, none = call(None)
    assert none is None
    assert_result((s0, None), want, k, flags, n, (ctx, "sizing"))
    buf = table_buf(k)
    s, table = call(buf)
    assert_result((s, table), want, k, flags, n, ctx)
    assert bytes(s0) == bytes(s), (ctx, "the summary depends on cap")
    assert (buf[4 ** k:] == SENTINEL).all(), (ctx, "entries behind 4^k were written")


def check_buffer(torch, scfq, a, ks, ctx, offset=0, host=False, modes=(0, CANONICAL), checker=kmers_of_np):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    t, ptr = to_dev(torch, a, offset)
    for k in ks:
        for flags in modes:
            want = checker(a, k, flags != 0)
            check_call(scfq, lambda tb: scfq.kmers_device(ptr, a.size, k, flags, tb), want, k, flags, a.size, (ctx, "device"))
            if host:
                check_call(scfq, lambda tb: scfq.kmers_host(a, k, flags, tb), want, k, flags, a.size, (ctx, "host"))


def golden_files():
    files = sorted(glob.glob(os.path.join(GOLDEN, "*.fq")) + glob.glob(os.path.join(GOLDEN, "edge", "*.fq")))
    assert len(files) >= 30
    return files


@pytest.mark.parametrize("k", [1, 3, 7, 8, 12])
def test_golden_files_every_entry_point(gpu, scfq, k):
    for path in golden_files():
        data = open(path, "rb").read()
        a = np.frombuffer(data, dtype=np.uint8)
        t, ptr = to_dev(gpu, a)
        for flags in (0, CANONICAL):
            want = kmers_of_np(a, k, flags != 0)
            if len(data) < 20_000:
                assert kmers_of(data, k, flags != 0) == want, path
            check_call(scfq, lambda tb: scfq.kmers_device(ptr, a.size, k, flags, tb), want, k, flags, a.size, (path, "device"))
            if k < 12:
                check_call(scfq, lambda tb: scfq.kmers_host(a, k, flags, tb), want, k, flags, a.size, (path, "host"))
                check_call(scfq, lambda tb: scfq.kmers_file(path, k, flags, tb), want, k, flags, a.size, (path, "file"))
            else:                               # (128 MiB of table per full call: the sizing call carries the whole summary)
                assert_result(scfq.kmers_host(a, k, flags), want, k, flags, a.size, (path, "host"))
                assert_result(scfq.kmers_file(path, k, flags), want, k, flags, a.size, (path, "file"))


def sc(*args):
    r = subprocess.run([SC, "fq-kmers"] + list(args), capture_output=True, text=True, stdin=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_cli(gpu, scfq):
    files = golden_files()
    data = [open(p, "rb").read() for p in files]
    for k, canonical in ((7, False), (3, True), (8, False)):
        wants = [kmers_of_np(np.frombuffer(d, dtype=np.uint8), k, canonical) for d in data]
        opts = ["--k=%d" % k] + (["--canonical"] if canonical else [])
        # every file in one process, rows in argument order
        assert sc("-b", *opts, *files) == "".join(cli_text(w[0], k, "\t" + os.path.basename(p)) for p, w in zip(files, wants))
        assert sc("--top=3", *opts, *files) == "".join(cli_text(w[0], k, top=3) for w in wants)
        assert sc("--totals", "-t", *opts, *files) == "k\twindows\tkmers\tskipped\tshort_lines\tdistinct\tmax_count\n" + "".join(totals_text(w, k) for w in wants)
    dup = os.path.join(GOLDEN, "dup.fq")
    assert sc(dup) == sc("--k=7", dup) == cli_text(kmers_of(open(dup, "rb").read(), 7)[0], 7)                    # the default k
    assert sc("--k=2", "--top=0", dup) == ""
    # the literal tables
    many = os.path.join(GOLDEN, "edge", "many_short.fq")
    assert sc("--k=2", many) == "AC\t300\nCG\t300\nGC\t300\nGT\t300\n"
    assert sc("--k=2", "-t", "-b", "--top=3", many) == "kmer\tcount\tbasename\nAC\t300\tmany_short.fq\nCG\t300\tmany_short.fq\nGC\t300\tmany_short.fq\n"
    assert sc("--k=2", "--canonical", many) == "AC\t600\nCG\t300\nGC\t300\n"
    assert sc("--k=2", "--totals", many) == "2\t2100\t1200\t900\t0\t4\t300\n"
    assert sc("--k=8", "--totals", "-b", many) == "8\t300\t0\t300\t0\t0\t0\tmany_short.fq\n"
    assert sc("--k=9", "--totals", many) == "9\t0\t0\t0\t300\t0\t0\n"
    assert sc("--k=8", many) == sc("--k=9", many) == ""


def test_literal_tables(gpu, scfq):
    ix = index_of
    data = b"@h\nACGTN\n+\nIIIII\n"
    s, t = scfq.kmers_host(data, 2, 0, True)
    assert {int(v): int(t[v]) for v in np.flatnonzero(t)} == {ix(b"AC"): 1, ix(b"CG"): 1, ix(b"GT"): 1}
    assert (s.windows, s.kmers, s.skipped, s.short_lines, s.distinct, s.max_count, s.table_entries, s.lines, s.reads) == (4, 3, 1, 0, 3, 1, 16, 4, 1)
    s, t = scfq.kmers_host(data, 2, CANONICAL, True)
    assert {int(v): int(t[v]) for v in np.flatnonzero(t)} == {ix(b"AC"): 2, ix(b"CG"): 1} and (s.windows, s.kmers, s.skipped, s.distinct, s.max_count) == (4, 3, 1, 2, 2)
    many = os.path.join(GOLDEN, "edge", "many_short.fq")
    s, t = scfq.kmers_file(many, 2, 0, True)
    assert {int(v): int(t[v]) for v in np.flatnonzero(t)} == {ix(b"AC"): 300, ix(b"CG"): 300, ix(b"GC"): 300, ix(b"GT"): 300}
    assert (s.windows, s.kmers, s.skipped, s.short_lines) == (2100, 1200, 900, 0)
    s, t = scfq.kmers_file(many, 8, 0, True)
    assert (s.windows, s.kmers, s.skipped, s.short_lines, s.distinct, s.max_count, int(t.sum())) == (300, 0, 300, 0, 0, 0, 0)
    s, t = scfq.kmers_file(many, 9, 0, True)
    assert (s.windows, s.kmers, s.skipped, s.short_lines, s.distinct, s.max_count, int(t.sum())) == (0, 0, 0, 300, 0, 0, 0)


def test_gzip_inputs(gpu, scfq):
    for name in ("dup.fq.gz", os.path.join("edge", "two_member.fq.gz")):
        path = os.path.join(GOLDEN, name)
        data = gzip.open(path, "rb").read()
        for k in (1, 7, 8):
            for flags in (0, CANONICAL):
                want = kmers_of(data, k, flags != 0)
                check_call(scfq, lambda tb: scfq.kmers_file(path, k, flags, tb), want, k, flags, len(data), name)


@pytest.mark.parametrize("kind", ["uniform", "ascii", "dense_nl", "sparse_nl", "crlf"])
def test_random_buffers(gpu, scfq, kind):
    """tile and chunk boundaries inside windows: sizes around the 8 KiB step and its multiples"""
    rng = np.random.default_rng(83)
    for n in (1, 2, 15, 16, 17, 255, 4096, 32767, 32768, 32769, 65535, 65536, 65537, 1_000_000):
        a = random_fastq_like(rng, n, kind)
        modes = (0, CANONICAL) if n <= 65537 else (0,)
        check_buffer(gpu, scfq, a, (1, 7, 8, 12), (kind, n), host=n <= 4096, modes=modes)
        if n > 3:
            check_buffer(gpu, scfq, a[:-1], (1, 7, 8, 12), (kind, n, "last byte removed"), modes=modes)
            check_buffer(gpu, scfq, a[:2 * n // 3], (1, 7, 8, 12), (kind, n, "cut at two thirds"), modes=modes)


@pytest.mark.parametrize("crlf", [False, True])
def test_wellformed_records(gpu, scfq, crlf):
    rng = np.random.default_rng(9 + crlf)
    a = make_fastq(rng, 3000, crlf=crlf)
    check_buffer(gpu, scfq, a, (2, 7, 8), ("make_fastq", crlf), host=True)
    check_buffer(gpu, scfq, a[:-1], (7, 8), ("make_fastq", crlf, "last byte removed"))
    check_buffer(gpu, scfq, a[:2 * a.size // 3], (7, 8), ("make_fastq", crlf, "cut at two thirds"))


@pytest.mark.parametrize("k", [1, 2, 11, 12])
def test_every_line_length_and_alignment(gpu, scfq, k):
    """sequence lines of every length 0 .. 40 with mixed line ends, letters that depend on the position, the device pointer at offsets
    0 .. 15: the halo, the "\\r\\n" rule and short_lines"""
    alpha, parts = b"ACGTNacgtX", []
    for rep in range(3):                   # any letter / A C G T with another letter every 17 / A C G T only
        for L in range(41):
            eol = b"\r\n" if (L + rep) % 3 == 0 else b"\n"
            if rep == 0:
                seq = bytes(alpha[(p * p + L) % len(alpha)] for p in range(L))
            else:
                seq = bytes(alpha[4 + p % 6] if rep == 1 and (p + L) % 17 == 0 else b"ACGT"[(p * 7 + L + p // 5) & 3] for p in range(L))
            parts += [b"@" + b"h" * (L % 23), eol, seq, eol, b"+", eol, b"I" * L, eol]
    data = b"".join(parts)
    a = np.frombuffer(data, dtype=np.uint8)
    want = {flags: kmers_of(data, k, flags != 0) for flags in (0, CANONICAL)}
    assert want[0] == kmers_of_np(a, k) and want[0][4] == 3 * min(k, 41) and want[0][2] > 0 and want[0][3] > 0
    for offset in range(16):
        t, ptr = to_dev(gpu, a, offset)
        for flags in (0, CANONICAL):
            check_call(scfq, lambda tb: scfq.kmers_device(ptr, a.size, k, flags, tb), want[flags], k, flags, a.size, ("every line length", offset))


def test_degenerate_inputs(gpu, scfq):
    ix = index_of
    for data in (b"", b"\n", b"x", b"@a\r", b"\r\n" * 1000, b"@h\n", b"@h\nACGT\n", b"@h\nACGT\n+\n", b"@h\nACGT", b"@h\nACGT\r",
                 b"@h\r\nACGT\r\n+", b"@h\nAC\n+\nII\n@g\nACGTA\n+\n", b"@h\nA", b"@h\n\n+\n\n@g\n\r\n"):
        a = np.frombuffer(data, dtype=np.uint8)
        check_buffer(gpu, scfq, a, (1, 4, 5, 8), data[:16], host=True, checker=lambda b, k, c: kmers_of(bytes(b), k, c))
    s, t = scfq.kmers_host(b"", 5, 0, True)
    assert (s.reads, s.lines, s.windows, s.kmers, s.skipped, s.short_lines, s.distinct, s.max_count, s.table_entries) == (0, 0, 0, 0, 0, 0, 0, 0, 1024)
    assert t.shape == (1024,) and not t.any()
    for data, k, kmers, skipped in ((b"@h\nACGT", 4, 1, 0), (b"@h\nACGT\r", 4, 1, 1), (b"@h\nACGT\r", 5, 0, 1), (b"@h\r\nACGT\r\n+", 4, 1, 0)):
        s, t = scfq.kmers_host(data, k, 0, True)
        assert (s.kmers, s.skipped, s.windows) == (kmers, skipped, kmers + skipped), (data, k)
        assert int(t[ix(b"ACGT")]) == kmers if k == 4 else not t.any()


def test_long_lines(gpu, scfq):
    """lines that run through many steps and blocks, and one of 3 MB among short ones"""
    rng = np.random.default_rng(15)
    parts = []
    for r in range(3):
        parts += [b"@long%d\n" % r, bytes(rng.choice(np.frombuffer(b"ACGTACGTACGTNn", dtype=np.uint8), 100_000)), b"\n+\n",
                  bytes(rng.integers(33, 127, 100_000, dtype=np.uint8)), b"\n"]
    a = np.frombuffer(b"".join(parts), dtype=np.uint8)
    check_buffer(gpu, scfq, a, (7, 12), "three records of 100 kB lines")
    check_buffer(gpu, scfq, a, (7, 12), "three records of 100 kB lines, unaligned", offset=5, modes=(0,))
    letters = np.frombuffer(b"ACGT" * 50 + b"N", dtype=np.uint8)
    big = np.concatenate([np.frombuffer(b"@big\n", dtype=np.uint8), rng.choice(letters, 3_000_000), np.frombuffer(b"\n+\n", dtype=np.uint8),
                          rng.choice(np.frombuffer(b"FI5#~", dtype=np.uint8), 2_999_990), np.frombuffer(b"\n", dtype=np.uint8)])
    a = np.concatenate([make_fastq(rng, 40), big, make_fastq(rng, 40)])
    check_buffer(gpu, scfq, a, (7, 12), "a 3 MB line among short ones", offset=3)


@pytest.mark.parametrize("k", [1, 7, 8, 12])
def test_contention(gpu, scfq, k):
    """8 MiB of one letter: every window is the same k-mer"""
    L = 8 << 20
    poly_a = np.concatenate([np.frombuffer(b"@a\n", dtype=np.uint8), np.full(L, ord("A"), np.uint8), np.frombuffer(b"\n+\n\n", dtype=np.uint8)])
    t, ptr = to_dev(gpu, poly_a)
    for flags in (0, CANONICAL):
        s, table = scfq.kmers_device(ptr, poly_a.size, k, flags, table_buf(k))
        assert (s.windows, s.kmers, s.skipped, s.short_lines, s.distinct, s.max_count, s.lines) == (L - k + 1, L - k + 1, 0, 0, 1, L - k + 1, 4), (k, flags)
        assert int(table[0]) == L - k + 1 and int(table[4 ** k - 1]) == 0 and int(table.sum()) == L - k + 1, (k, flags)      # AAAA, not TTTT
    poly_g = np.full(L, ord("G"), np.uint8)
    poly_g[999::1000] = ord("N")
    a = np.concatenate([np.frombuffer(b"@g\n", dtype=np.uint8), poly_g, np.frombuffer(b"\n+\n\n", dtype=np.uint8)])
    runs, last = L // 1000, L % 1000                      # 999 G and an N, and a last run without one
    kmers = runs * max(0, 999 - k + 1) + max(0, last - k + 1)
    t, ptr = to_dev(gpu, a, 7)
    for flags in (0, CANONICAL):
        s, table = scfq.kmers_device(ptr, a.size, k, flags, table_buf(k))
        at = index_of(b"C" * k) if flags else index_of(b"G" * k)
        assert (s.windows, s.kmers, s.skipped, s.distinct, s.max_count) == (L - k + 1, kmers, L - k + 1 - kmers, 1, kmers), (k, flags)
        assert int(table[at]) == kmers and int(table.sum()) == kmers, (k, flags)
    if k == 8:
        assert_result(scfq.kmers_device(ptr, a.size, k, 0, table_buf(k)), kmers_of_np(a, k), k, 0, a.size, "poly-G against numpy")


@pytest.mark.parametrize("kind,seed", [(0, 20260101), (1, 20260103)])
def test_synthetic_16mib_against_numpy(gpu, scfq, kind, seed):
    torch = gpu
    plan = scfq.synth_plan(kind, seed, 16 << 20)
    buf = torch.empty(plan.bytes + 4096, dtype=torch.uint8, device="cuda")
    scfq.synth_device(kind, seed, plan.records, buf.data_ptr(), plan.bytes)
    a = buf[:plan.bytes].cpu().numpy()
    for k, flags in ((4, 0), (4, CANONICAL), (7, 0), (7, CANONICAL), (8, 0), (8, CANONICAL), (12, 0), (12, CANONICAL)):
        want = kmers_of_np(a, k, flags != 0, dense=True)
        check_call(scfq, lambda tb: scfq.kmers_device(buf.data_ptr(), plan.bytes, k, flags, tb), want, k, flags, plan.bytes, ("synthetic", kind))


@pytest.mark.parametrize("kind,seed", [(0, 20260101), (1, 20260103)])
def test_synthetic_64mib_against_the_counters(gpu, scfq, kind, seed):
    """no pass over the data outside the library: the totals against scfq_count_buffer and scfq_cycles_buffer"""
    torch = gpu
    plan = scfq.synth_plan(kind, seed, 64 << 20)
    buf = torch.empty(plan.bytes + 4096, dtype=torch.uint8, device="cuda")
    scfq.synth_device(kind, seed, plan.records, buf.data_ptr(), plan.bytes)
    ptr, n = buf.data_ptr(), plan.bytes
    c = scfq.count_device(ptr, n)
    cy, _ = scfq.cycles_device(ptr, n, 0)
    tot = cy.total
    s, table = scfq.kmers_device(ptr, n, 1, 0, True)
    assert table.tolist() == [tot.a, tot.c, tot.g, tot.t]
    assert (s.windows, s.skipped) == (c.bases, tot.n + (tot.bases - tot.a - tot.c - tot.g - tot.t - tot.n)) and s.windows == tot.bases
    assert (s.reads, s.lines, s.input_bytes, s.short_lines) == (c.reads, c.lines, n, 0)
    prev_windows = s.windows
    for k in (1, 4, 7, 8, 12):
        plain = None
        for flags in (0, CANONICAL):
            s, table = scfq.kmers_device(ptr, n, k, flags, table_buf(k))
            assert int(table.sum()) == s.kmers and s.windows == s.kmers + s.skipped, (k, flags)
            assert s.distinct == int(np.count_nonzero(table)) and s.max_count == int(table.max()), (k, flags)
            assert s.windows <= prev_windows, (k, flags)
            if s.short_lines == 0:
                assert s.windows == c.bases - (k - 1) * c.reads, (k, flags)
            if plain is None:
                plain = (s.windows, s.kmers, s.skipped, s.short_lines)
            else:
                assert plain == (s.windows, s.kmers, s.skipped, s.short_lines), k


def test_repeatability_and_memory(gpu, scfq):
    torch = gpu
    rng = np.random.default_rng(5)
    a, b = make_fastq(rng, 2000), make_fastq(rng, 1500, read_len=(400, 2500))
    ta, pa = to_dev(torch, a)
    tb, pb = to_dev(torch, b)
    for k in (7, 8):
        wa, wb = kmers_of_np(a, k), kmers_of_np(b, k, True)
        first = scfq.kmers_device(pa, a.size, k, 0, True)
        assert_result(first, wa, k, 0, a.size, "first buffer")
        before = scfq.lib().scfq_device_bytes_now()
        again = scfq.kmers_device(pa, a.size, k, 0, True)
        assert bytes(first[0]) == bytes(again[0]) and first[1].tobytes() == again[1].tobytes()
        assert_result(scfq.kmers_device(pb, b.size, k, CANONICAL, True), wb, k, CANONICAL, b.size, "second buffer")
        scfq.cycles_device(pa, a.size, 300)
        third = scfq.kmers_device(pa, a.size, k, 0, True)
        assert bytes(first[0]) == bytes(third[0]) and first[1].tobytes() == third[1].tobytes()
        assert scfq.lib().scfq_device_bytes_now() == before

"""fq-readstats on the device (csrc/scfq_readstats.hip) against the checker of tests/_readstats_check.py: the per-read table and
every field of the summary, compared with ==."""
import glob
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG
from _readstats_check import assert_summary, lines_of, per_read, per_read_np, row_text, summary_of
from test_gpu_hist_spec import make_fastq
from test_gpu_parity import random_fastq_like, to_dev

pytestmark = pytest.mark.gpu

SC = os.path.join(PKG, "sc")
TILE = 32768          # kRsTile


def table_of(torch, scfq, ptr, n):
    """(summary, table as an int64 tensor of shape (reads, 5)) of a device-resident input: size with NULL, then fill"""
    s0 = scfq.read_stats_device(ptr, n)
    reads = s0.reads
    tab = torch.full((max(reads, 1), 5), -1, dtype=torch.int64, device="cuda")      # (not zeros: the library owes every entry)
    s = scfq.read_stats_device(ptr, n, tab.data_ptr(), reads)
    assert bytes(s0) == bytes(s), "the summary does not depend on whether a table is asked for"
    return s, tab[:reads]


def check_buffer(torch, scfq, a, ctx, offset=0, host=False, rows=None, lines=None):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if rows is None:
        rows, lines = per_read_np(a)
    elif lines is None:
        lines = len(lines_of(bytes(a)))
    t, ptr = to_dev(torch, a, offset)
    s, tab = table_of(torch, scfq, ptr, a.size)
    got = tab.cpu().numpy()
    want = np.asarray(rows, dtype=np.int64).reshape(-1, 5)
    assert got.shape == want.shape, (ctx, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).any(axis=1))
        raise AssertionError((ctx, "records differ", bad[:8].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist()))
    assert_summary(s, want, a.size, lines, ctx)
    if host:
        assert_summary(scfq.read_stats_host(a), want, a.size, lines, (ctx, "host"))
    return s


def test_golden_files_every_entry_point(gpu, scfq):
    files = sorted(glob.glob(os.path.join(GOLDEN, "*.fq")) + glob.glob(os.path.join(GOLDEN, "edge", "*.fq")))
    assert len(files) >= 30
    for path in files:
        data = open(path, "rb").read()
        rows = per_read(data)
        a = np.frombuffer(data, dtype=np.uint8)
        check_buffer(gpu, scfq, a, path, host=True, rows=rows)
        lines = len(lines_of(data))
        assert_summary(scfq.read_stats_file(path), rows, len(data), lines, (path, "file"))
        r = subprocess.run([SC, "fq-readstats", "-b", path], capture_output=True, text=True, stdin=subprocess.DEVNULL)
        assert (r.returncode, r.stdout) == (0, row_text(rows) + "\t" + os.path.basename(path) + "\n"), (path, r.stderr)
        assert scfq.format_read_stats_tsv(scfq.read_stats_file(path)) == row_text(rows)
    # the literal rows of the table in the issue
    s = scfq.read_stats_file(os.path.join(GOLDEN, "edge", "many_short.fq"))
    assert (s.reads, s.bases, s.min_len, s.max_len, s.n50, s.l50, s.n90, s.l90) == (300, 2400, 8, 8, 8, 150, 8, 270)
    s = scfq.read_stats_file(os.path.join(GOLDEN, "edge", "n_rich.fq"))
    assert (s.reads, s.bases, s.min_len, s.max_len, s.n50, s.l50, s.n90, s.l90) == (2, 18, 4, 14, 14, 1, 4, 2)
    # --hist prints the non-empty bins
    path = os.path.join(GOLDEN, "edge", "many_short.fq")
    assert subprocess.run([SC, "fq-readstats", "--hist=len", path], capture_output=True, text=True).stdout == "4\t300\n"
    want = summary_of(per_read(open(path, "rb").read()))
    for which, key in (("gc", "gc_hist"), ("qual", "meanq_hist")):
        out = subprocess.run([SC, "fq-readstats", "--hist=" + which, path], capture_output=True, text=True).stdout
        assert out == "".join("%d\t%d\n" % (k, c) for k, c in enumerate(want[key]) if c), which


def test_gzip_and_bgzf_inputs(gpu, scfq):
    for name in ("dup.fq.gz", os.path.join("edge", "two_member.fq.gz")):
        path = os.path.join(GOLDEN, name)
        data = gzip.open(path, "rb").read()
        lines = len(lines_of(data))
        assert_summary(scfq.read_stats_file(path), per_read(data), len(data), lines, name)


@pytest.mark.parametrize("kind", ["uniform", "ascii", "dense_nl", "sparse_nl", "crlf"])
def test_random_buffers(gpu, scfq, kind):
    rng = np.random.default_rng(77)
    for n in (1, 2, 15, 16, 17, 255, 4096, 32767, 32768, 32769, 100_000, 1_000_000):
        a = random_fastq_like(rng, n, kind)
        check_buffer(gpu, scfq, a, (kind, n), host=n <= 4096)
        if n > 3:
            check_buffer(gpu, scfq, a[:-1], (kind, n, "last byte removed"))
            check_buffer(gpu, scfq, a[:2 * n // 3], (kind, n, "cut at two thirds"))


@pytest.mark.parametrize("crlf", [False, True])
def test_wellformed_records(gpu, scfq, crlf):
    rng = np.random.default_rng(5 + crlf)
    a = make_fastq(rng, 3000, crlf=crlf)
    check_buffer(gpu, scfq, a, ("make_fastq", crlf), host=True)
    check_buffer(gpu, scfq, a[:-1], ("make_fastq", crlf, "last byte removed"))
    check_buffer(gpu, scfq, a[:2 * a.size // 3], ("make_fastq", crlf, "cut at two thirds"))


def test_degenerate_inputs(gpu, scfq):
    for data in (b"", b"\n", b"x", b"@a\r", b"\r\n" * 1000, b"\n" * 1_000_000):
        a = np.frombuffer(data, dtype=np.uint8)
        check_buffer(gpu, scfq, a, data[:16], host=len(data) <= 2000)
    s = scfq.read_stats_host(b"")
    assert (s.reads, s.lines, s.min_len, s.max_len, s.n50, s.l50) == (0, 0, 0, 0, 0, 0)
    rng = np.random.default_rng(8)
    big = rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), 50_000_000)
    s = check_buffer(gpu, scfq, big, "one 50 MB line without a newline")
    assert (s.reads, s.lines, s.bases) == (1, 1, 0)
    rec = np.concatenate([np.frombuffer(b"@long\n", dtype=np.uint8), big, np.frombuffer(b"\n+\n", dtype=np.uint8),
                          rng.choice(np.frombuffer(b"FI5#", dtype=np.uint8), big.size), np.frombuffer(b"\n", dtype=np.uint8)])
    a = np.concatenate([make_fastq(rng, 50), rec, make_fastq(rng, 50)])
    s = check_buffer(gpu, scfq, a, "a 50 MB sequence line inside a valid record")
    assert (s.reads, s.max_len, s.n50, s.l50) == (101, 50_000_000, 50_000_000, 1)


def test_border_stress(gpu, scfq):
    """records whose sequence lines and whose quality lines take every length from 0 to 2 tiles + 1 (16 inputs of ~270 MB, the lengths
    dealt round by residue so that every input has short and long lines next to each other and a line starts at every phase of a tile);
    then one stream at every alignment of the pointer"""
    rng = np.random.default_rng(12)
    seq_pool = bytes(rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), 4 << 20))
    qual_pool = bytes(rng.choice(np.frombuffer(b"FI5#~", dtype=np.uint8), 4 << 20))
    top = 2 * TILE + 1
    seen_seq, seen_qual = set(), set()
    first = None
    for batch in range(16):
        lengths = list(range(batch, top + 1, 16))
        rng.shuffle(lengths)
        parts = []
        for k, L in enumerate(lengths):
            Q = lengths[len(lengths) - 1 - k]
            eol = b"\r\n" if k % 3 == 0 else b"\n"
            so, qo = int(rng.integers(0, len(seq_pool) - top)), int(rng.integers(0, len(qual_pool) - top))
            parts += [b"@" + b"h" * (k % 61), eol, seq_pool[so:so + L], eol, b"+", eol, qual_pool[qo:qo + Q], eol]
        a = np.frombuffer(b"".join(parts), dtype=np.uint8)
        rows, lines = per_read_np(a)
        seen_seq |= set(rows[:, 0].tolist())
        seen_qual |= set(rows[:, 3].tolist())
        check_buffer(gpu, scfq, a, ("every line length", batch), rows=rows, lines=lines)
        if first is None:
            first = a[:3 * TILE + 1234].copy()
        del a, parts
    assert seen_seq == seen_qual == set(range(top + 1))
    for offset in range(16):
        check_buffer(gpu, scfq, first, ("unaligned", offset), offset=offset)


def test_synthetic_64mib_against_numpy(gpu, scfq):
    torch = gpu
    for kind, seed in ((scfq.SCFQ_SYNTH_ILLUMINA if hasattr(scfq, "SCFQ_SYNTH_ILLUMINA") else 0, 20260101), (1, 20260103)):
        plan = scfq.synth_plan(kind, seed, 64 << 20)
        buf = torch.empty(plan.bytes + 4096, dtype=torch.uint8, device="cuda")
        scfq.synth_device(kind, seed, plan.records, buf.data_ptr(), plan.bytes)
        a = buf[:plan.bytes].cpu().numpy()
        rows, lines = per_read_np(a)
        s, tab = table_of(torch, scfq, buf.data_ptr(), plan.bytes)
        assert np.array_equal(tab.cpu().numpy(), rows), kind
        assert_summary(s, rows, plan.bytes, lines, ("synthetic", kind))
        assert s.reads == plan.records


def test_synthetic_1gib_against_the_counters(gpu, scfq):
    """no Python pass over the data: the table reduced with torch on the device against scfq_count_buffer, N50 / N90 from torch.sort"""
    torch = gpu
    for kind, seed in ((0, 20260101), (1, 20260103)):
        plan = scfq.synth_plan(kind, seed, 1 << 30)
        buf = torch.empty(plan.bytes + 4096, dtype=torch.uint8, device="cuda")
        scfq.synth_device(kind, seed, plan.records, buf.data_ptr(), plan.bytes)
        c = scfq.count_device(buf.data_ptr(), plan.bytes, flags=scfq.SCFQ_QUAL_HIST)
        s, tab = table_of(torch, scfq, buf.data_ptr(), plan.bytes)
        hist = list(c.qual_hist)
        sums = [int(v) for v in tab.sum(dim=0).tolist()]
        assert sums == [c.bases, c.gc_bases, c.n_bases, sum(hist), sum(b * k for b, k in enumerate(hist))], kind
        assert [s.bases, s.gc_bases, s.n_bases, s.qual_bytes, s.qual_sum] == sums
        assert s.reads == c.reads == plan.records == tab.shape[0] and s.lines == c.lines and s.input_bytes == plan.bytes
        lens = tab[:, 0]
        assert (s.min_len, s.max_len) == (int(lens.min()), int(lens.max()))
        if kind == 0:
            assert s.min_len == s.max_len == 150
        desc, _ = torch.sort(lens, descending=True)
        acc = torch.cumsum(desc, 0) * 100
        for x, (nx, lx) in ((50, (s.n50, s.l50)), (90, (s.n90, s.l90))):
            k = int(torch.searchsorted(acc, torch.tensor([s.bases * x], device="cuda", dtype=torch.int64), right=False)[0])
            assert (nx, lx) == (int(desc[k]), k + 1), (kind, x)
        assert sum(s.len_hist) == s.reads and sum(s.gc_hist) == s.reads and sum(s.meanq_hist) + s.no_qual == s.reads
        del buf, tab
        torch.cuda.empty_cache()


def test_table_capacity_independence_and_memory(gpu, scfq):
    torch = gpu
    rng = np.random.default_rng(3)
    a, b = make_fastq(rng, 2000), make_fastq(rng, 1500, read_len=(400, 900))
    ta, pa = to_dev(torch, a)
    tb, pb = to_dev(torch, b)
    rows_a, lines_a = per_read_np(a)
    rows_b, lines_b = per_read_np(b)
    reads = rows_a.shape[0]
    tab = torch.full((reads, 5), -1, dtype=torch.int64, device="cuda")
    s = scfq._new_read_summary()
    import ctypes
    rc = scfq.lib().scfq_read_stats_buffer(ctypes.c_void_p(pa), a.size, 1, ctypes.c_void_p(tab.data_ptr()), reads - 1, ctypes.byref(s))
    assert rc == scfq.SCFQ_EARG and s.reads == reads
    assert int((tab != -1).sum()) == 0                       # a table that is too small is not written
    s = scfq.read_stats_device(pa, a.size, tab.data_ptr(), reads)
    assert np.array_equal(tab.cpu().numpy(), rows_a)
    # two calls in a row on different buffers, then the first again: nothing of one call is left in the next
    before = scfq.lib().scfq_device_bytes_now()
    tab_b = torch.full((rows_b.shape[0], 5), -1, dtype=torch.int64, device="cuda")
    sb = scfq.read_stats_device(pb, b.size, tab_b.data_ptr(), rows_b.shape[0])
    assert np.array_equal(tab_b.cpu().numpy(), rows_b)
    assert_summary(sb, rows_b, b.size, lines_b, "second buffer")
    tab.fill_(-1)
    sa = scfq.read_stats_device(pa, a.size, tab.data_ptr(), reads)
    assert np.array_equal(tab.cpu().numpy(), rows_a)
    assert_summary(sa, rows_a, a.size, lines_a, "first buffer again")
    assert scfq.lib().scfq_device_bytes_now() == before

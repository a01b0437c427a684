"""fq-cycles on the device (csrc/scfq_cycles.hip) against the checker of tests/_cycles_check.py: every row, the tail, the total and
every field of the summary, compared with ==."""
import glob
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG
from _cycles_check import assert_result, cli_text, row_ints, row_text, table_of, table_of_np
from test_gpu_hist_spec import make_fastq
from test_gpu_parity import random_fastq_like, to_dev

pytestmark = pytest.mark.gpu

SC = os.path.join(PKG, "sc")
SENTINEL = -7


def check_ptr(scfq, ptr, n, want, caps, ctx):
    """the device buffer at every cap: rows beyond `cycles` keep what the caller wrote, and total does not depend on cap"""
    table, lines, ms, mq = want
    totals = set()
    for cap in caps:
        buf = np.full((cap, 8), SENTINEL, dtype=np.int64)
        s, rows = scfq.cycles_device(ptr, n, buf)
        assert_result((s, rows), table, lines, ms, mq, n, cap, ctx)
        assert rows.shape[0] == s.cycles and (buf[s.cycles:] == SENTINEL).all(), (ctx, cap, "rows [cycles, cap) were written")
        totals.add(bytes(s.total))
    assert len(totals) == 1, (ctx, "total depends on cap")


def caps_of(want):
    top = max(want[2], want[3])
    return sorted({0, 1, 7, top, top + 5})


def check_buffer(torch, scfq, a, ctx, offset=0, host=False, want=None, caps=None):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if want is None:
        want = table_of_np(a)
    t, ptr = to_dev(torch, a, offset)
    check_ptr(scfq, ptr, a.size, want, caps_of(want) if caps is None else caps, ctx)
    if host:
        top = max(want[2], want[3])
        assert_result(scfq.cycles_host(a, top + 1), *want, a.size, top + 1, (ctx, "host"))
    return want


def test_golden_files_every_entry_point(gpu, scfq):
    files = sorted(glob.glob(os.path.join(GOLDEN, "*.fq")) + glob.glob(os.path.join(GOLDEN, "edge", "*.fq")))
    assert len(files) >= 30
    tables = []
    for path in files:
        data = open(path, "rb").read()
        want = table_of(data)
        table, top = want[0], max(want[2], want[3])
        check_buffer(gpu, scfq, np.frombuffer(data, dtype=np.uint8), path, host=True, want=want)
        for cap in (0, 3, top + 2):
            assert_result(scfq.cycles_file(path, cap), *want, len(data), cap, (path, "file"))
        s, rows = scfq.cycles_file(path, top)
        assert [scfq.format_cycle_row_tsv(r) for r in rows] == [row_text(r) for r in table]
        assert scfq.format_cycle_row_tsv(s.total) == row_text(row_ints(s.total)) == row_text(table.sum(axis=0))
        tables.append((path, table))
    # the CLI: every file in one process, rows in argument order
    r = subprocess.run([SC, "fq-cycles", "-b"] + files, capture_output=True, text=True, stdin=subprocess.DEVNULL)
    assert (r.returncode, r.stdout) == (0, "".join(cli_text(t, 1000, "\t" + os.path.basename(p)) for p, t in tables)), r.stderr
    r = subprocess.run([SC, "fq-cycles", "--max-cycles=5"] + files, capture_output=True, text=True, stdin=subprocess.DEVNULL)
    assert (r.returncode, r.stdout) == (0, "".join(cli_text(t, 5) for p, t in tables)), r.stderr
    # the CLI's complete output for the two literal tables
    r = subprocess.run([SC, "fq-cycles", os.path.join(GOLDEN, "edge", "n_rich.fq")], capture_output=True, text=True, stdin=subprocess.DEVNULL)
    assert r.stdout == ("1\t2\t0\t0\t0\t0\t2\t0\t2\t33.0\n2\t2\t0\t0\t0\t0\t2\t0\t2\t33.0\n3\t2\t0\t0\t0\t0\t2\t0\t2\t33.0\n4\t2\t0\t0\t0\t0\t2\t0\t2\t33.0\n"
                        "5\t1\t1\t0\t0\t0\t0\t0\t1\t33.0\n6\t1\t0\t1\t0\t0\t0\t0\t1\t33.0\n7\t1\t0\t0\t1\t0\t0\t0\t1\t33.0\n8\t1\t0\t0\t0\t1\t0\t0\t1\t33.0\n"
                        "9\t1\t0\t0\t0\t0\t1\t0\t1\t33.0\n10\t1\t0\t0\t0\t0\t1\t0\t1\t33.0\n11\t1\t0\t0\t1\t0\t0\t0\t1\t33.0\n12\t1\t0\t0\t1\t0\t0\t0\t1\t33.0\n"
                        "13\t1\t0\t1\t0\t0\t0\t0\t1\t33.0\n14\t1\t0\t1\t0\t0\t0\t0\t1\t33.0\n")
    r = subprocess.run([SC, "fq-cycles", "-t", "-b", os.path.join(GOLDEN, "edge", "many_short.fq")], capture_output=True, text=True, stdin=subprocess.DEVNULL)
    letters = ("300\t0\t0\t0\t0", "0\t300\t0\t0\t0", "0\t0\t300\t0\t0", "0\t0\t0\t300\t0", "0\t0\t0\t0\t300", "0\t0\t0\t0\t300", "0\t0\t300\t0\t0", "0\t300\t0\t0\t0")
    assert r.stdout == "cycle\tbases\tA\tC\tG\tT\tN\tother\tquals\tmean_qual\tbasename\n" + "".join(
        "%d\t300\t%s\t0\t300\t%s\tmany_short.fq\n" % (p + 1, letters[p], "35.0" if p == 4 else "73.0") for p in range(8))


def test_gzip_inputs(gpu, scfq):
    for name in ("dup.fq.gz", os.path.join("edge", "two_member.fq.gz")):
        path = os.path.join(GOLDEN, name)
        data = gzip.open(path, "rb").read()
        want = table_of(data)
        for cap in (0, 4, max(want[2], want[3]) + 1):
            assert_result(scfq.cycles_file(path, cap), *want, len(data), cap, name)


@pytest.mark.parametrize("kind", ["uniform", "ascii", "dense_nl", "sparse_nl", "crlf"])
def test_random_buffers(gpu, scfq, kind):
    rng = np.random.default_rng(79)
    for n in (1, 2, 15, 16, 17, 255, 4096, 32767, 32768, 32769, 100_000, 1_000_000):
        a = random_fastq_like(rng, n, kind)
        check_buffer(gpu, scfq, a, (kind, n), host=n <= 4096)
        if n > 3:
            check_buffer(gpu, scfq, a[:-1], (kind, n, "last byte removed"))
            check_buffer(gpu, scfq, a[:2 * n // 3], (kind, n, "cut at two thirds"))


@pytest.mark.parametrize("crlf", [False, True])
def test_wellformed_records(gpu, scfq, crlf):
    rng = np.random.default_rng(6 + crlf)
    a = make_fastq(rng, 3000, crlf=crlf)
    check_buffer(gpu, scfq, a, ("make_fastq", crlf), host=True)
    check_buffer(gpu, scfq, a[:-1], ("make_fastq", crlf, "last byte removed"))
    check_buffer(gpu, scfq, a[:2 * a.size // 3], ("make_fastq", crlf, "cut at two thirds"))


def test_degenerate_inputs(gpu, scfq):
    for data in (b"", b"\n", b"x", b"@a\r", b"\r\n" * 1000, b"\n" * 1_000_000,
                 b"@h\n", b"@h\nACGT\n", b"@h\nACGT\n+\n", b"@h\nACGT", b"@h\r\nACGT\r\n+", b"@h\nAC\n+\nII\n@g\nACGTA\n+\n"):
        a = np.frombuffer(data, dtype=np.uint8)
        want = table_of(data) if len(data) <= 2000 else None
        check_buffer(gpu, scfq, a, data[:16], host=len(data) <= 2000, want=want)
    s, rows = scfq.cycles_host(b"", 5)
    assert (s.reads, s.lines, s.cycles, s.max_seq_len, s.max_qual_len, rows.shape) == (0, 0, 0, 0, 0, (0, 8))
    assert row_ints(s.total) == row_ints(s.tail) == [0] * 8


def test_every_line_length_and_alignment(gpu, scfq):
    """records whose sequence and quality lines take every length 0 .. 300 (the quality line of a record is as long as the sequence line
    of the record from the other end), letters and quality bytes that depend on the position; the device pointer at offsets 0 .. 15"""
    seq_alpha, parts = b"ACGTNacgtX", []
    for L in range(301):
        Q = 300 - L
        eol = b"\r\n" if L % 3 == 0 else b"\n"
        seq = bytes(seq_alpha[(p * p + L) % len(seq_alpha)] for p in range(L))
        qual = bytes(33 + (7 * p + L) % 94 for p in range(Q))
        parts += [b"@" + b"h" * (L % 23), eol, seq, eol, b"+", eol, qual, eol]
    a = np.frombuffer(b"".join(parts), dtype=np.uint8)
    want = table_of_np(a)
    assert (want[2], want[3]) == (300, 300) and want[0][:, 0].tolist() == want[0][:, 6].tolist() == [300 - p for p in range(300)]
    for offset in range(16):
        check_buffer(gpu, scfq, a, ("every line length", offset), offset=offset, want=want, caps=(0, 7, 150, 300, 305))


def test_long_lines(gpu, scfq):
    """lines that run through a hundred position windows, and one of 3 MB among short ones"""
    rng = np.random.default_rng(14)
    parts = []
    for k in range(3):
        parts += [b"@long%d\n" % k, bytes(rng.choice(np.frombuffer(b"ACGTNn", dtype=np.uint8), 100_000)), b"\n+\n",
                  bytes(rng.integers(33, 127, 100_000, dtype=np.uint8)), b"\n"]
    a = np.frombuffer(b"".join(parts), dtype=np.uint8)
    want = table_of_np(a)
    assert (want[2], want[3]) == (100_000, 100_000)
    check_buffer(gpu, scfq, a, "three records of 100 kB lines", want=want, caps=(0, 1000, 65536, 99_999, 100_000, 100_001))
    check_buffer(gpu, scfq, a, "three records of 100 kB lines, unaligned", offset=5, want=want, caps=(1024, 100_000))
    big = np.concatenate([np.frombuffer(b"@big\n", dtype=np.uint8), rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), 3_000_000),
                          np.frombuffer(b"\n+\n", dtype=np.uint8), rng.choice(np.frombuffer(b"FI5#~", dtype=np.uint8), 2_999_990),
                          np.frombuffer(b"\n", dtype=np.uint8)])
    a = np.concatenate([make_fastq(rng, 40), big, make_fastq(rng, 40)])
    want = table_of_np(a)
    assert (want[2], want[3]) == (3_000_000, 2_999_990)
    check_buffer(gpu, scfq, a, "a 3 MB line among short ones", offset=3, want=want, caps=(0, 200, 2_999_995, 3_000_000))


def test_counter_width(gpu, scfq):
    """17 000 000 records of one N and one 0xff: the quality sum of position 0 is above 2^32, and every counter a block keeps is 32 bits wide"""
    torch = gpu
    rec = b"@\nN\n+\n\xff\n"
    reps = 17_000_000
    t = torch.frombuffer(bytearray(rec), dtype=torch.uint8).to("cuda").repeat(reps)
    n = reps * len(rec)
    assert t.numel() == n
    for cap in (4, 0):
        s, rows = scfq.cycles_device(t.data_ptr(), n, cap)
        want = [reps, 0, 0, 0, 0, reps, reps, 4_335_000_000]
        assert (s.reads, s.lines, s.input_bytes, s.max_seq_len, s.max_qual_len, s.cycles) == (reps, 4 * reps, n, 1, 1, min(cap, 1))
        assert row_ints(s.total) == want and row_ints(s.tail) == ([0] * 8 if cap else want)
        assert rows.tolist() == ([want] if cap else [])


def test_synthetic_16mib_against_numpy(gpu, scfq):
    torch = gpu
    for kind, seed in ((scfq.SCFQ_SYNTH_ILLUMINA, 20260101), (scfq.SCFQ_SYNTH_NANOPORE, 20260103)):
        plan = scfq.synth_plan(kind, seed, 16 << 20)
        buf = torch.empty(plan.bytes + 4096, dtype=torch.uint8, device="cuda")
        scfq.synth_device(kind, seed, plan.records, buf.data_ptr(), plan.bytes)
        want = table_of_np(buf[:plan.bytes].cpu().numpy())
        top = max(want[2], want[3])
        check_ptr(scfq, buf.data_ptr(), plan.bytes, want, (0, 100, top, top + 1), ("synthetic", kind))


def test_synthetic_1gib_against_the_counters(gpu, scfq):
    """no pass over the data outside the library: the totals against scfq_count_buffer and scfq_read_stats_buffer"""
    torch = gpu
    for kind, seed in ((scfq.SCFQ_SYNTH_ILLUMINA, 20260101), (scfq.SCFQ_SYNTH_NANOPORE, 20260103)):
        plan = scfq.synth_plan(kind, seed, 1 << 30)
        buf = torch.empty(plan.bytes + 4096, dtype=torch.uint8, device="cuda")
        scfq.synth_device(kind, seed, plan.records, buf.data_ptr(), plan.bytes)
        c = scfq.count_device(buf.data_ptr(), plan.bytes)
        rs = scfq.read_stats_device(buf.data_ptr(), plan.bytes)
        s0, _ = scfq.cycles_device(buf.data_ptr(), plan.bytes, 0)
        top = max(s0.max_seq_len, s0.max_qual_len)
        s, rows = scfq.cycles_device(buf.data_ptr(), plan.bytes, top)
        assert bytes(s0.total) == bytes(s.total) and bytes(s0.tail) == bytes(s.total) and row_ints(s.tail) == [0] * 8
        assert (s.reads, s.lines, s.input_bytes, s.cycles) == (c.reads, c.lines, plan.bytes, top) and s.reads == plan.records
        assert (s.max_seq_len, s.max_qual_len) == (rs.max_len, rs.max_len)
        t = s.total
        assert (t.bases, t.g + t.c, t.n) == (c.bases, c.gc_bases, c.n_bases), kind
        assert (t.quals, t.qual_sum) == (rs.qual_bytes, rs.qual_sum), kind
        assert rows.sum(axis=0).tolist() == row_ints(t)
        assert (np.diff(rows[:, 0]) <= 0).all() and (np.diff(rows[:, 6]) <= 0).all() and rows[0, 0] == s.reads == rows[0, 6]
        assert (rows[:, 1:6].sum(axis=1) == rows[:, 0]).all()          # the generator writes A C G T N only
        del buf
        torch.cuda.empty_cache()


def test_repeatability_and_memory(gpu, scfq):
    torch = gpu
    rng = np.random.default_rng(4)
    a, b = make_fastq(rng, 2000), make_fastq(rng, 1500, read_len=(400, 2500))
    ta, pa = to_dev(torch, a)
    tb, pb = to_dev(torch, b)
    wa, wb = table_of_np(a), table_of_np(b)
    first = scfq.cycles_device(pa, a.size, 300)
    assert_result(first, *wa, a.size, 300, "first buffer")
    before = scfq.lib().scfq_device_bytes_now()
    again = scfq.cycles_device(pa, a.size, 300)
    assert bytes(first[0]) == bytes(again[0]) and first[1].tobytes() == again[1].tobytes()
    assert_result(scfq.cycles_device(pb, b.size, 3000), *wb, b.size, 3000, "second buffer")
    scfq.read_stats_device(pa, a.size)
    third = scfq.cycles_device(pa, a.size, 300)
    assert bytes(first[0]) == bytes(third[0]) and first[1].tobytes() == third[1].tobytes()
    assert scfq.lib().scfq_device_bytes_now() == before

"""fq-kcount on the device (csrc/scfq_kcount.hip) against the checkers of tests/_kcount_check.py: every field of the summary, the
histogram, the dump and the queries, compared with ==."""
import glob
import gzip
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import GOLDEN, PKG
from _kcount_check import (CANONICAL, DUMP_HEADER, EFULL, HIST_HEADER, TOTALS_HEADER, Want, assert_summary, assert_table, dump_of, hist_of, hist_text,
                           kcount_of, kcount_of_np, rows_text, top_of, totals_text)
from _kmers_check import index_of, revcomp_index, word_of
from _partition_cases import _fq_fill, k1_behind_the_input, k2_edges_inside, k3_merge
from test_gpu_parity import to_dev

pytestmark = pytest.mark.gpu

SC = os.path.join(PKG, "sc")
HERE = os.path.dirname(os.path.abspath(__file__))
KCOUNT = os.path.join(GOLDEN, "kcount")
KS = (13, 21, 31, 32)
MODES = (0, CANONICAL)
SENTINEL = 0xDEADBEEF12345678


def kc_threads():
    text = open(os.path.join(PKG, "csrc", "scfq_kcount.hip")).read()
    return int(re.search(r"constexpr uint32_t kKcThreads = (\d+);", text).group(1))


STEP = 16 * kc_threads()


def fq(*seqs):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(seqs))


def golden_files():
    files = sorted(glob.glob(os.path.join(GOLDEN, "*.fq")) + glob.glob(os.path.join(GOLDEN, "edge", "*.fq")))
    assert len(files) >= 30
    return files


def check_device(torch, scfq, a, k, flags, ctx, offset=0, want=None, full=True):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    want = want if want is not None else kcount_of_np(a, k, flags != 0)
    t, ptr = to_dev(torch, a, offset)
    s, table = scfq.kcount_device(ptr, a.size, k=k, flags=flags)
    with table:
        assert_summary(s, want, k, flags, ctx)
        if full:
            assert_table(table, want, k, flags, ctx)
        else:
            assert [tuple(r) for r in table.dump().tolist()] == dump_of(want.table), (ctx, k, flags)
    s0, none = scfq.kcount_device(ptr, a.size, k=k, flags=flags, table=False)                  # the summary alone
    assert none is None and bytes(s0) == bytes(s), (ctx, "the summary depends on the table being asked for")
    return s


@pytest.mark.parametrize("k", KS)
def test_golden_files_every_entry_point(gpu, scfq, k):
    for path in golden_files():
        data = open(path, "rb").read()
        a = np.frombuffer(data, dtype=np.uint8)
        for flags in MODES:
            want = kcount_of_np(a, k, flags != 0)
            if len(data) < 20_000:
                assert kcount_of(data, k, flags != 0) == want, path
            check_device(gpu, scfq, a, k, flags, (path, "device"), want=want)
            for name, call in (("host", lambda: scfq.kcount_host(a, k=k, flags=flags)), ("file", lambda: scfq.kcount_files(path, k=k, flags=flags))):
                s, table = call()
                with table:
                    assert_summary(s, want, k, flags, (path, name))
                    assert_table(table, want, k, flags, (path, name))


def test_gzip_input(gpu, scfq):
    path = os.path.join(GOLDEN, "dup.fq.gz")
    data = gzip.open(path, "rb").read()
    for k in (13, 32):
        for flags in MODES:
            want = kcount_of(data, k, flags != 0)
            s, table = scfq.kcount_files(path, k=k, flags=flags)
            with table:
                assert_summary(s, want, k, flags, path)
                assert_table(table, want, k, flags, path)


# ---- load edges -------------------------------------------------------------------------------------------------------------
def letters(n, salt):
    return bytes(b"ACGT"[((i * i + salt) * 2654435761 >> 7) & 3] for i in range(n))


@pytest.mark.parametrize("k", KS)
def test_read_lengths_line_ends_and_alignment(gpu, scfq, k):
    """reads of k - 1, k, k + 1, 46, 47, 48 letters and of every length 0 .. 70, "\\n", "\\r\\n" and no final newline, the device pointer
    at offsets 0 .. 15: a sequence line ends on every byte of a chunk, and windows lie in the input's first and last chunks"""
    parts = [b"@\n" + letters(48, 1) + b"\n+\n\n"]                                            # windows in the first chunk
    for rep, L in enumerate([k - 1, k, k + 1, 46, 47, 48] + list(range(71))):
        eol = b"\r\n" if rep % 3 == 0 else b"\n"
        parts += [b"@h%d" % rep, eol, letters(L, rep), eol, b"+", eol, b"I" * L, eol]
    parts += [b"@last\n" + letters(50, 7)]                                                    # no final newline: windows in the last chunks
    data = b"".join(parts)
    a = np.frombuffer(data, dtype=np.uint8)
    want = {flags: kcount_of(data, k, flags != 0) for flags in MODES}
    assert want[0] == kcount_of_np(a, k) and want[0].short_lines == k + 1 and want[0].kmers > 100 and want[0].skipped == 0
    for tail in (data, data + b"\r", data + b"\n", data + b"\r\n"):
        b = np.frombuffer(tail, dtype=np.uint8)
        for offset in range(16) if tail is data else (0, 5):
            for flags in MODES:
                check_device(gpu, scfq, b, k, flags, ("lengths", len(tail) - len(data), offset), offset=offset,
                             want=want[flags] if tail is data else kcount_of(tail, k, flags != 0), full=offset == 0)


@pytest.mark.parametrize("k", KS)
def test_a_bad_letter_at_every_position(gpu, scfq, k):
    """an N or a lower-case letter at each position of a read of 2 k letters: the smear over up to 32 positions"""
    base = letters(2 * k, 3)
    reads = []
    for p in range(2 * k):
        r = bytearray(base)
        r[p] = ord("N") if p % 2 else ord("acgt"[p % 4])
        reads.append(bytes(r))
    data = fq(*reads)
    for flags in MODES:
        want = kcount_of(data, k, flags != 0)
        # read p has k + 1 windows; those that start in [max(0, p - k + 1), min(p, k)] hold position p
        assert want.skipped == sum(min(p, k) - max(0, p - k + 1) + 1 for p in range(2 * k)) == want.windows - want.kmers
        for offset in (0, 3, 11):
            check_device(gpu, scfq, np.frombuffer(data, dtype=np.uint8), k, flags, ("bad letter", offset), offset=offset, want=want, full=False)


@pytest.mark.parametrize("shift", [0, 7])
def test_partition_edges(gpu, scfq, shift):
    """records that straddle an 8 KiB step (every step is a block's boundary below 8 MiB), the chunk behind the input, and the
    run merge next to another word, placed as tests/_partition_cases.py places them for fq-kmers"""
    cases = list(k1_behind_the_input(STEP, shift, endings=("short", "long_cr"))) + list(k2_edges_inside(STEP, shift, deltas=range(-13, 3, 3)))
    cases += [c for m in (16, 17, 1025) for c in k3_merge(m)]
    assert len(cases) >= 30
    for label, a, facts in cases:
        for k, flags in ((13, 0), (21, CANONICAL), (32, 0)):
            check_device(gpu, scfq, a, k, flags, label, offset=shift, want=kcount_of_np(a, k, flags != 0), full=False)


def test_two_blocks_runs_of_steps(gpu, scfq):
    """more than 1024 steps: a block owns two consecutive steps, and records straddle the boundary between two blocks' runs"""
    data = _fq_fill(9 << 20, 5)
    a = np.frombuffer(data, dtype=np.uint8)
    assert a.size // STEP > 1024
    check_device(gpu, scfq, a, 13, CANONICAL, "9 MiB", offset=9, full=False)


# ---- keys -------------------------------------------------------------------------------------------------------------------
def test_the_all_ones_key(gpu, scfq):
    ones = 2 ** 64 - 1
    data = fq(b"T" * 40, b"A" * 40)
    s, t = scfq.kcount_host(data, k=32)
    with t:
        assert (s.windows, s.kmers, s.distinct, s.unique, s.max_count) == (18, 18, 2, 0, 9)
        assert t.dump().tolist() == [[0, 9], [ones, 9]] and t.query([ones, 0, 1, ones - 1]).tolist() == [9, 9, 0, 0]
        assert t.hist(2).tolist() == [0, 2] and t.hist(10).tolist() == [0] * 9 + [2] and t.hist(11).tolist() == [0] * 9 + [2, 0]
        assert t.dump(10).tolist() == [] and t.dump(9, 9).tolist() == [[0, 9], [ones, 9]]
        out = np.full((3, 2), SENTINEL, dtype=np.uint64)
        assert t.dump_into(out, 1) == 2 and (out == SENTINEL).all()                           # cap < total: nothing is written
    s, t = scfq.kcount_host(data, k=32, flags=CANONICAL)
    with t:
        assert (s.kmers, s.distinct, s.unique, s.max_count) == (18, 1, 0, 18)
        assert t.dump().tolist() == [[0, 18]] and t.query([ones, 0, 5]).tolist() == [18, 18, 0]
    s, t = scfq.kcount_host(fq(b"T" * 32, b"ACGT" * 8), k=32)                                 # the side counter alone is unique
    with t:
        assert (s.kmers, s.distinct, s.unique, s.max_count) == (2, 2, 2, 1) and t.hist(3).tolist() == [0, 2, 0]
        assert t.dump().tolist() == [[index_of(b"ACGT" * 8), 1], [ones, 1]]
    for flags in MODES:
        for k in (31, 32):
            a = np.frombuffer(fq(b"T" * 40, b"A" * 40, b"T" * 31 + b"G" + b"T" * 33), dtype=np.uint8)
            for offset in (0, 8):
                check_device(gpu, scfq, a, k, flags, "T and A", offset=offset, want=kcount_of(bytes(a), k, flags != 0))


@pytest.mark.parametrize("k", [13, 32])
def test_run_merge(gpu, scfq, k):
    """a 100 kB poly-G line, and a line that alternates two k-mers lane by lane (sixteen windows of one, sixteen of the other)"""
    L = 100_000
    poly_g = np.full(L, ord("G"), np.uint8)
    poly_g[4999::5000] = ord("N")
    unit = b"A" * (16 + k - 1) + b"C" * (16 + k - 1)
    alt = (b"A" * 16 + b"C" * 16) * 400
    for seq in (poly_g.tobytes(), alt, unit * 50):
        data = b"@g\n" + seq + b"\n+\n\n"
        a = np.frombuffer(data, dtype=np.uint8)
        for flags in MODES:
            want = kcount_of_np(a, k, flags != 0)
            for offset in (0, 13):                     # (13: the line's first letter on a lane's first byte)
                check_device(gpu, scfq, a, k, flags, ("merge", len(seq), offset), offset=offset, want=want, full=False)
    want = kcount_of_np(np.frombuffer(b"@g\n" + poly_g.tobytes() + b"\n+\n\n", dtype=np.uint8), k)
    assert want.distinct == 1 and want.max_count == 20 * (4999 - k + 1)


def test_one_count_above_2_to_32(gpu, scfq):
    """a single record whose sequence line is 2^32 + 4096 x A, made on the device: one key, its count above 2^32"""
    torch = gpu
    L, k = 2 ** 32 + 4096, 13
    head, tail = b"@a\n", b"\n+\n\n"
    buf = torch.full((len(head) + L + len(tail),), ord("A"), dtype=torch.uint8, device="cuda")
    buf[:len(head)] = torch.tensor(list(head), dtype=torch.uint8)
    buf[len(head) + L:] = torch.tensor(list(tail), dtype=torch.uint8)
    s, t = scfq.kcount_device(buf.data_ptr(), buf.numel(), k=k)
    with t:
        n = L - k + 1
        assert n > 2 ** 32
        assert (s.reads, s.lines, s.input_bytes, s.windows, s.kmers, s.skipped, s.short_lines, s.distinct, s.unique, s.max_count, s.passes) == \
            (1, 4, buf.numel(), n, n, 0, 0, 1, 0, n, 1)
        assert t.dump().tolist() == [[0, n]] and t.query([0, 1]).tolist() == [n, 0] and t.hist(4).tolist() == [0, 0, 0, 1]
    del buf


# ---- the table --------------------------------------------------------------------------------------------------------------
def distinct_reads(n, k=13):
    """n reads of k letters each, all different: exactly n distinct keys in plain mode"""
    return fq(*[word_of((i * 7919 + 5) % 4 ** k, k).encode() for i in range(n)])


def test_table_bits_10_at_its_capacity(gpu, scfq):
    for n in (1023, 1024):
        data = distinct_reads(n)
        want = kcount_of(data, 13)
        assert want.distinct == n == want.unique
        s, t = scfq.kcount_host(data, k=13, table_bits=10)
        with t:
            assert_summary(s, want, 13, 0, n)
            assert (s.slots, s.passes) == (1024, 1)
            assert_table(t, want, 13, 0, n)                                                   # (queries absent keys on the full table, too)
            absent = [v for v in range(0, 4 ** 13, 4 ** 13 // 300) if v not in want.table]
            assert len(absent) > 250 and not t.query(absent).any()
    t0 = time.perf_counter()
    with pytest.raises(scfq.ScfqError) as e:
        scfq.kcount_host(distinct_reads(1025), k=13, table_bits=10)
    assert e.value.rc == EFULL and e.value.handle is None and "1024 slots" in str(e.value)
    assert time.perf_counter() - t0 < 10, "a pass over a table that is too small ends by itself"
    s, none = scfq.kcount_host(distinct_reads(1025), k=13, table_bits=11, table=False)
    assert none is None and (s.distinct, s.slots, s.passes) == (1025, 2048, 1)


def child(env, k, flags, bits, *paths):
    e = dict(os.environ)
    for name in ("SCFQ_KCOUNT_START_BITS", "SCFQ_KCOUNT_MAX_PROBE", "SCFQ_KCOUNT_MERGE"):
        e.pop(name, None)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(HERE, "_kcount_child.py"), str(k), str(flags), str(bits)] + list(paths), env=e,
                       capture_output=True, text=True, stdin=subprocess.DEVNULL, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def same_but_diagnostics(a, b):
    sa, sb = dict(a["summary"]), dict(b["summary"])
    for name in ("slots", "passes"):
        sa.pop(name), sb.pop(name)
    return sa == sb and all(a[f] == b[f] for f in ("rc", "dump", "hist", "query"))


def test_growth(gpu, scfq, tmp_path):
    path = tmp_path / "five_thousand.fq"
    path.write_bytes(distinct_reads(5000, 21))
    want = kcount_of(path.read_bytes(), 21, True)
    assert 4900 <= want.distinct <= 5000
    plain = child({}, 21, CANONICAL, 0, str(path))
    assert plain["rc"] == 0 and plain["summary"]["passes"] == 1 and plain["dump"] == [list(r) for r in dump_of(want.table)]
    grown = child({"SCFQ_KCOUNT_START_BITS": "10"}, 21, CANONICAL, 0, str(path))
    assert grown["rc"] == 0 and grown["summary"]["passes"] >= 2 and grown["summary"]["slots"] > 1024
    assert same_but_diagnostics(plain, grown)
    # START_BITS does not touch a table_bits that is given
    fixed = child({"SCFQ_KCOUNT_START_BITS": "10"}, 21, CANONICAL, 14, str(path))
    assert fixed["summary"]["slots"] == 1 << 14 and fixed["summary"]["passes"] == 1 and same_but_diagnostics(plain, fixed)


def test_merge_of_lanes_switched_off(gpu, scfq, tmp_path):
    """SCFQ_KCOUNT_MERGE=0 leaves out the merge across lanes and nothing else: poly-G with an N now and then, a line that alternates two
    k-mers lane by lane and ordinary reads give what the merging run gives, which is the checker's"""
    poly_g = np.full(20_000, ord("G"), np.uint8)
    poly_g[4999::5000] = ord("N")
    path = tmp_path / "runs.fq"
    data = fq(poly_g.tobytes(), (b"A" * 16 + b"C" * 16) * 100, *[letters(60, 300 + i) for i in range(8)])
    path.write_bytes(data)
    for k, flags in ((13, 0), (32, CANONICAL)):
        want = kcount_of_np(np.frombuffer(data, dtype=np.uint8), k, flags != 0)
        merged = child({}, k, flags, 0, str(path))
        plain = child({"SCFQ_KCOUNT_MERGE": "0"}, k, flags, 0, str(path))
        assert merged["rc"] == 0 and merged["dump"] == [list(r) for r in dump_of(want.table)] and merged["summary"]["kmers"] == want.kmers
        assert plain["summary"] == merged["summary"] and same_but_diagnostics(merged, plain), (k, flags)


def mix64(x):
    m = 2 ** 64 - 1
    x ^= x >> 33
    x = x * 0xff51afd7ed558ccd & m
    x ^= x >> 33
    x = x * 0xc4ceb9fe1a85ec53 & m
    return x ^ x >> 33


def test_max_probe_1_grows_instead_of_miscounting(gpu, scfq, tmp_path):
    path = tmp_path / "collide.fq"
    data = fq(*[letters(40, 100 + i) for i in range(12)])
    path.write_bytes(data)
    want = kcount_of(data, 21)
    slots = 1024
    while slots < 2 * len(data):
        slots *= 2
    assert len({mix64(v) & (slots - 1) for v in want.table}) < want.distinct, "no two keys collide at the first size"
    got = child({"SCFQ_KCOUNT_MAX_PROBE": "1"}, 21, 0, 0, str(path))
    assert got["rc"] == 0 and got["summary"]["passes"] >= 2 and got["summary"]["slots"] > slots
    assert got["dump"] == [list(r) for r in dump_of(want.table)] and got["summary"]["kmers"] == want.kmers
    assert got["hist"] == hist_of(want.table, want.max_count + 2) and got["query"] == [c for _, c in dump_of(want.table)]
    full = child({"SCFQ_KCOUNT_MAX_PROBE": "1"}, 21, 0, 10, str(path))
    assert full["rc"] == EFULL and full["handle"] is None and "1024 slots" in full["text"] and full["seconds"] < 30


# ---- two inputs -------------------------------------------------------------------------------------------------------------
def test_two_inputs(gpu, scfq):
    p1, p2 = (os.path.join(GOLDEN, "pairs", n) for n in ("r1.fq", "r2.fq"))
    d1, d2 = open(p1, "rb").read(), open(p2, "rb").read()
    a1, a2 = np.frombuffer(d1, dtype=np.uint8), np.frombuffer(d2[:len(d2) * 2 // 3], dtype=np.uint8)
    for k, flags in ((21, 0), (21, CANONICAL), (32, CANONICAL)):
        want = kcount_of_np([np.frombuffer(d1, dtype=np.uint8), np.frombuffer(d2, dtype=np.uint8)], k, flags != 0)
        for s, t in (scfq.kcount_files(p1, p2, k=k, flags=flags), scfq.kcount_host(d1, d2, k=k, flags=flags)):
            with t:
                assert_summary(s, want, k, flags, "pairs")
                assert_table(t, want, k, flags, "pairs", bins=(2, want.max_count + 2))
        # lengths that differ, on the device at two alignments
        want = kcount_of_np([a1, a2], k, flags != 0)
        (t1, q1), (t2, q2) = to_dev(gpu, a1, 3), to_dev(gpu, a2, 12)
        s, t = scfq.kcount_device(q1, a1.size, q2, a2.size, k=k, flags=flags)
        with t:
            assert_summary(s, want, k, flags, "pairs, device")
            assert_table(t, want, k, flags, "pairs, device", bins=(2, want.max_count + 2))
    # an empty second input
    want = kcount_of(d1, 21)
    for s, t in (scfq.kcount_host(d1, b"", k=21), scfq.kcount_host(b"", d1, k=21), scfq.kcount_host(d1, None, k=21)):
        with t:
            assert_summary(s, want, 21, 0, "r2 empty")
            assert [tuple(r) for r in t.dump().tolist()] == dump_of(want.table)
    s, t = scfq.kcount_host(b"", k=21)
    with t:
        assert (s.reads, s.lines, s.windows, s.kmers, s.distinct, s.unique, s.max_count, s.slots, s.passes) == (0, 0, 0, 0, 0, 0, 0, 1024, 1)
        assert t.dump().tolist() == [] and t.hist(2).tolist() == [0, 0] and t.query([5]).tolist() == [0] and t.query([]).tolist() == []


def test_two_handles_alive_at_once(gpu, scfq):
    da, db = fq(letters(90, 1), letters(60, 2)), fq(letters(70, 3))
    wa, wb = kcount_of(da, 21), kcount_of(db, 21, True)
    for order in ((0, 1), (1, 0)):
        before = scfq.lib().scfq_device_bytes_now()
        sa, ta = scfq.kcount_host(da, k=21)
        sb, tb = scfq.kcount_host(db, k=21, flags=CANONICAL)
        assert_table(ta, wa, 21, 0, "a")
        assert_table(tb, wb, 21, CANONICAL, "b")
        first, second = ((ta, wa, 0), (tb, wb, CANONICAL)) if order == (0, 1) else ((tb, wb, CANONICAL), (ta, wa, 0))
        first[0].close()
        assert_table(second[0], second[1], 21, second[2], "the other one lives on")
        second[0].close()
        second[0].close()                                                                     # (twice is fine)
        assert scfq.lib().scfq_device_bytes_now() == before
    with pytest.raises(scfq.ScfqError) as e:
        s, t = scfq.kcount_host(da, k=21)
        with t:
            t.query([4 ** 21])
    assert e.value.rc == scfq.SCFQ_EARG and str(4 ** 21) in str(e.value)


# ---- dump -------------------------------------------------------------------------------------------------------------------
def test_dump_filters_and_capacity(gpu, scfq):
    data = open(os.path.join(KCOUNT, "reads.fq"), "rb").read()
    want = kcount_of(data, 21, True)
    s, t = scfq.kcount_host(data, k=21, flags=CANONICAL)
    with t:
        for lo, hi in ((1, 0), (5, 0), (1, 1), (2, 4), (15, 15), (want.max_count, 0), (want.max_count + 1, 0), (1, want.max_count), (2 ** 63, 0)):
            assert [tuple(r) for r in t.dump(lo, hi).tolist()] == dump_of(want.table, lo, hi), (lo, hi)
        rows = dump_of(want.table, 5)
        total = len(rows)
        out = np.full((total + 3, 2), SENTINEL, dtype=np.uint64)
        assert t.dump_into(out, total - 1, 5) == total and (out == SENTINEL).all()             # cap = total - 1: nothing is written
        assert t.dump_into(out, 0, 5) == total and t.dump_into(None, 0, 5) == total and (out == SENTINEL).all()
        assert t.dump_into(out, total + 3, 5) == total
        assert [tuple(r) for r in out[:total].tolist()] == rows and (out[total:] == SENTINEL).all()      # the last three untouched
        out[:] = SENTINEL
        assert t.dump_into(out, total, 5) == total and [tuple(r) for r in out[:total].tolist()] == rows
        assert_table(t, want, 21, CANONICAL, "fixture")
        assert t.hist(2 ** 20).tolist()[:40] == hist_of(want.table, 40)[:39] + [0]
        with pytest.raises(scfq.ScfqError):
            t.hist(1)


# ---- the command ------------------------------------------------------------------------------------------------------------
def sc(*args):
    r = subprocess.run([SC, "fq-kcount"] + list(args), capture_output=True, text=True, stdin=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_cli(gpu, scfq):
    """the fixture's four texts byte for byte, and the options around them"""
    reads = os.path.join(KCOUNT, "reads.fq")
    text = {n: open(os.path.join(KCOUNT, n)).read() for n in ("hist.txt", "dump_min5.txt", "top10.txt", "totals.txt")}
    opts = ("--k=21", "--canonical")
    assert sc(*opts, reads) == text["hist.txt"] and sc("--canonical", reads) == text["hist.txt"]                # 21 is the default
    assert sc(*opts, "--dump", "--min-count=5", reads) == text["dump_min5.txt"]
    assert sc(*opts, "--top=10", reads) == text["top10.txt"]
    assert sc(*opts, "--totals", reads) == text["totals.txt"]
    data = open(reads, "rb").read()
    want = kcount_of(data, 21, True)
    assert sc(*opts, "-t", "-b", "--high=12", reads) == HIST_HEADER + "\tbasename\n" + hist_text(want.table, 12, "\treads.fq")
    assert sc(*opts, "--table-bits=14", "--high=%d" % want.max_count, reads) == text["hist.txt"]
    assert sc(*opts, "-t", "--dump", "--min-count=20", "--max-count=21", reads) == DUMP_HEADER + "\n" + rows_text(dump_of(want.table, 20, 21), 21)
    assert sc(*opts, "-t", "--totals", reads) == TOTALS_HEADER + "\n" + text["totals.txt"]
    for n in (0, 5, 10 ** 6):
        assert sc(*opts, "--top=%d" % n, reads) == rows_text(top_of(want.table, n), 21), n
    # two files are counted together, plain mode at another k
    p1, p2 = (os.path.join(GOLDEN, "pairs", n) for n in ("r1.fq", "r2.fq"))
    both = kcount_of_np([np.frombuffer(open(p, "rb").read(), dtype=np.uint8) for p in (p1, p2)], 31)
    assert sc("--k=31", p1, p2) == hist_text(both.table) and sc("--k=31", "--totals", "-b", p1, p2) == totals_text(both, 31, "\tr1.fq")
    assert sc("--k=31", "--top=7", p1, p2) == rows_text(top_of(both.table, 7), 31)
    r = subprocess.run([SC, "fq-kcount", reads, "missing_second.fq"], capture_output=True, text=True, stdin=subprocess.DEVNULL)
    assert (r.returncode, r.stderr, r.stdout) == (2, "\x1b[31mError 2: Unable to open file: missing_second.fq\x1b[0m\n", "")
    r = subprocess.run([SC, "fq-kcount", "--table-bits=10", reads], capture_output=True, text=True, stdin=subprocess.DEVNULL)
    assert r.returncode == 1 and "1024 slots" in r.stderr and r.stdout == ""

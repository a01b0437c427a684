"""fq-cycles without a device: the ABI (symbols, struct layouts, C99 header), argument checks, the row formatter, the CLI's
header / help / open-error behaviour, and the checker itself against the CPU oracle and two literal tables."""
import ctypes
import glob
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG, ROOT
from _cycles_check import ROW_FIELDS, cli_text, row_text, split, table_of, table_of_np
from _readstats_check import per_read
from test_gpu_parity import random_fastq_like

SC = os.path.join(PKG, "sc")
HEADER = "cycle\tbases\tA\tC\tG\tT\tN\tother\tquals\tmean_qual"
NEW = ("scfq_cycles_buffer", "scfq_cycles_file", "scfq_format_cycle_row_tsv", "scfq_cycles_error_detail")
SUMMARY_HEAD = ("struct_size", "abi_version", "reads", "lines", "input_bytes", "max_seq_len", "max_qual_len", "cycles")
FASTQ = b"@a\nACGT\n+\nIIII\n"


def run(*args):
    return subprocess.run([SC] + list(args), capture_output=True, text=True, stdin=subprocess.DEVNULL)


def test_symbols_declared_exported_and_listed(scfq):
    header = open(os.path.join(ROOT, "include", "sc_fqcount.h")).read()
    debug = open(os.path.join(ROOT, "include", "sc_fqcount_debug.h")).read()
    L = scfq.lib()
    for name in NEW:
        assert name + "(" in header and name in scfq.EXPORTS and hasattr(L, name), name
    assert "scfq_debug_cycles_stages(" in debug and "scfq_debug_cycles_stages" in scfq.EXPORTS and hasattr(L, "scfq_debug_cycles_stages")
    assert len(scfq.cycles_stages()) == 4


def test_struct_layouts(scfq):
    assert ctypes.sizeof(scfq.CycleRow) == 64
    assert tuple(f[0] for f in scfq.CycleRow._fields_) == ROW_FIELDS == scfq.CYCLE_FIELDS
    for k, name in enumerate(ROW_FIELDS):
        assert getattr(scfq.CycleRow, name).offset == 8 * k, name
    S = scfq.CycleSummary
    for k, name in enumerate(SUMMARY_HEAD):
        assert getattr(S, name).offset == 8 * k, name
    assert S.tail.offset == 64 and S.total.offset == 128 and ctypes.sizeof(S) == 8 * (8 + 8 + 8)


def test_header_is_c99_and_sizes_agree(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "sc_fqcount.h"\n'
                   "typedef char row_is_64[sizeof(scfq_cycle_row) == 64 ? 1 : -1];\n"
                   "typedef char sum_size[sizeof(scfq_cycle_summary) == 8 * (8 + 8 + 8) ? 1 : -1];\n"
                   "typedef char at[offsetof(scfq_cycle_summary, cycles) == 56 && offsetof(scfq_cycle_summary, tail) == 64 && offsetof(scfq_cycle_summary, total) == 128 ? 1 : -1];\n"
                   "typedef char row_at[offsetof(scfq_cycle_row, n) == 40 && offsetof(scfq_cycle_row, qual_sum) == 56 ? 1 : -1];\n"
                   "int main(void){ scfq_cycle_row r; scfq_cycle_summary s; s.struct_size = sizeof s; r.bases = 0;\n"
                   "  return scfq_cycles_buffer(0, 0, 0, &r, 1, &s) + scfq_format_cycle_row_tsv(&r, 0, 0) + scfq_cycles_file(\"x\", 0, 0, 0, &s)\n"
                   "         + (scfq_cycles_error_detail() != 0) == 12345; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-fsyntax-only", str(src)])


def test_argument_checks(scfq):
    L = scfq.lib()
    s = scfq._new_cycle_summary()
    buf = ctypes.create_string_buffer(FASTQ)
    rows = (scfq.CycleRow * 4)()
    assert L.scfq_cycles_buffer(buf, 15, 0, rows, 4, None) == scfq.SCFQ_EARG                            # NULL summary
    bad = scfq.CycleSummary()                                                                          # struct_size not set
    assert L.scfq_cycles_buffer(buf, 15, 0, rows, 4, ctypes.byref(bad)) == scfq.SCFQ_EARG
    bad.struct_size = ctypes.sizeof(scfq.CycleSummary) - 8
    assert L.scfq_cycles_buffer(buf, 15, 0, rows, 4, ctypes.byref(bad)) == scfq.SCFQ_EARG
    assert L.scfq_cycles_buffer(None, 15, 0, rows, 4, ctypes.byref(s)) == scfq.SCFQ_EARG               # NULL pointer with n > 0
    assert L.scfq_cycles_buffer(buf, 15, 0, None, 4, ctypes.byref(s)) == scfq.SCFQ_EARG                # NULL rows with cap > 0
    assert L.scfq_cycles_error_detail() == b""
    assert L.scfq_cycles_buffer(buf, 15, 0, rows, (1 << 24) + 1, ctypes.byref(s)) == scfq.SCFQ_EARG    # cap above the limit
    assert b"16777216" in L.scfq_cycles_error_detail()
    assert L.scfq_cycles_file(None, None, rows, 4, ctypes.byref(s)) == scfq.SCFQ_EARG
    assert L.scfq_cycles_file(b"x.fq", None, rows, 4, ctypes.byref(bad)) == scfq.SCFQ_EARG
    assert L.scfq_cycles_file(b"x.fq", None, None, 4, ctypes.byref(s)) == scfq.SCFQ_EARG
    assert L.scfq_cycles_file(b"x.fq", None, rows, (1 << 24) + 1, ctypes.byref(s)) == scfq.SCFQ_EARG
    assert L.scfq_format_cycle_row_tsv(None, None, 0) == scfq.SCFQ_EARG
    with pytest.raises(scfq.ScfqError) as e:
        scfq.cycles_host(FASTQ, np.zeros(((1 << 24) + 1, 8), dtype=np.int64))
    assert e.value.rc == scfq.SCFQ_EARG and "16777216" in str(e.value)


def test_no_gpu_means_loud_failure(scfq):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    for cap in (0, 4):
        with pytest.raises(scfq.ScfqError) as e:
            scfq.cycles_host(FASTQ, cap)
        assert e.value.rc == scfq.SCFQ_EHIP
        with pytest.raises(scfq.ScfqError) as e:
            scfq.cycles_file(os.path.join(GOLDEN, "dup.fq"), cap)
        assert e.value.rc == scfq.SCFQ_EHIP
    with pytest.raises(scfq.ScfqError) as e:
        scfq.cycles_file(os.path.join(GOLDEN, "does_not_exist.fq"), 4)
    assert e.value.rc == scfq.SCFQ_EOPEN


def test_row_formatter(scfq):
    assert scfq.format_cycle_row_tsv(scfq.CycleRow()) == "0\t0\t0\t0\t0\t0\t0\t0\tnan"                 # 0/0 -> nan
    assert scfq.format_cycle_row_tsv((9, 1, 2, 3, 1, 1, 0, 0)) == "9\t1\t2\t3\t1\t1\t1\t0\tnan"        # other = 9 - 8
    row = "300\t75\t70\t80\t60\t5\t10\t300\t33.0"                                                      # ".0" on a bare integer
    r = scfq.CycleRow(300, 75, 70, 80, 60, 5, 300, 9900)
    assert scfq.format_cycle_row_tsv(r) == row
    assert scfq.format_cycle_row_tsv((300, 75, 70, 80, 60, 5, 300, 9901)) == row[:-4] + "%.16g" % (9901 / 300)
    assert scfq.format_cycle_row_tsv((2, 1, 0, 0, 1, 0, 2, 67)) == "2\t1\t0\t0\t1\t0\t0\t2\t33.5"
    for r8 in ((2, 0, 0, 0, 0, 2, 2, 66), (17_000_000, 0, 0, 0, 0, 17_000_000, 17_000_000, 4_335_000_000), (1, 0, 0, 0, 0, 0, 3, 700)):
        assert scfq.format_cycle_row_tsv(r8) == row_text(r8)
    L = scfq.lib()
    assert L.scfq_format_cycle_row_tsv(ctypes.byref(r), None, 0) == len(row)                           # sizing call
    small = ctypes.create_string_buffer(8)
    assert L.scfq_format_cycle_row_tsv(ctypes.byref(r), small, 8) == len(row) and small.value == row[:7].encode()
    exact = ctypes.create_string_buffer(len(row) + 1)
    assert L.scfq_format_cycle_row_tsv(ctypes.byref(r), exact, len(row) + 1) == len(row) and exact.value.decode() == row


def test_cli_without_a_device():
    r = run("fq-cycles", "--help")
    assert r.returncode == 0 and "fq-cycles [options] [fastq ...]" in r.stdout and "--max-cycles=N" in r.stdout
    assert run("fq-cycles").stdout == r.stdout
    top = run("--help").stdout
    assert "fq-cycles" in top and top.index("fq-readstats") < top.index("fq-cycles")
    r = run("fq-cycles", "-t", "-b")
    assert (r.returncode, r.stdout, r.stderr) == (0, HEADER + "\tbasename\n", "")
    assert run("fq-cycles", "-tba").stdout == HEADER + "\tbasename\tabsolute\n"
    assert run("fq-cycles", "--header", "--max-cycles=0").stdout == HEADER + "\n"
    r = run("fq-cycles", "does_not_exist.fq")
    c = run("fq-readstats", "does_not_exist.fq")
    assert (r.returncode, r.stderr, r.stdout) == (c.returncode, c.stderr, c.stdout) == (2, "\x1b[31mError 2: Unable to open file: does_not_exist.fq\x1b[0m\n", "")
    r, c = run("fq-cycles", "missing.fq.gz"), run("fq-readstats", "missing.fq.gz")
    assert (r.returncode, r.stderr) == (c.returncode, c.stderr) and r.returncode == 1
    r, c = run("fq-cycles", "-b"), run("fq-readstats", "-b")
    assert (r.returncode, r.stderr) == (c.returncode, c.stderr) == (3, "\x1b[31mError 3: No FASTQ specified\x1b[0m\n")
    assert run("fq-cycles", "--bogus").returncode == 1
    for bad in ("--max-cycles=", "--max-cycles=x", "--max-cycles=-1", "--max-cycles=1.5", "--max-cycles=16777217", "--max-cycles"):
        r = run("fq-cycles", "-t", bad)
        assert r.returncode == 1 and HEADER not in r.stdout and "Error" in r.stderr, bad


def golden_files():
    return sorted(glob.glob(os.path.join(GOLDEN, "*.fq")) + glob.glob(os.path.join(GOLDEN, "edge", "*.fq")))


def check_identity(oracle, data, ctx):
    """the checker's totals against the CPU oracle's counters and the per-read checker's column sums; plain against numpy"""
    table, lines, ms, mq = table_of(data)
    a = np.frombuffer(data, dtype=np.uint8)
    oc = oracle.count(a, "bytes")
    _, _, total = split(table, 0)
    assert lines == oc.lines, ctx
    assert (total[0], total[3] + total[2], total[5]) == (oc.bases, oc.gc_bases, oc.n_bases), ctx
    reads = per_read(data)
    assert (total[6], total[7]) == (sum(r[3] for r in reads), sum(r[4] for r in reads)), ctx
    assert (ms, mq) == (max([r[0] for r in reads] or [0]), max([r[3] for r in reads] or [0])), ctx
    t2, l2, ms2, mq2 = table_of_np(a)
    assert (l2, ms2, mq2) == (lines, ms, mq) and t2.shape == table.shape and np.array_equal(t2, table), ctx
    for cap in (0, 1, table.shape[0], table.shape[0] + 3):
        rows, tail, tot = split(table, cap)
        assert tot == total and [int(v) for v in rows.sum(axis=0)] == [x - y for x, y in zip(total, tail)], (ctx, cap)


def test_checker_against_the_oracle(scfq, oracle):
    files = golden_files()
    assert len(files) >= 30
    for path in files:
        check_identity(oracle, open(path, "rb").read(), path)


@pytest.mark.parametrize("kind", ["uniform", "ascii", "dense_nl", "sparse_nl", "crlf"])
def test_plain_and_numpy_checkers_agree(scfq, oracle, kind):
    assert hasattr(scfq, "cycles_device")
    rng = np.random.default_rng(43)
    for n in (0, 1, 2, 15, 16, 17, 255, 4096, 20_000):
        a = random_fastq_like(rng, n, kind)
        for cut in (n, n - 1, 2 * n // 3):
            if cut >= 0:
                check_identity(oracle, bytes(a[:cut]), (kind, n, cut))


def test_literal_tables(scfq):
    assert hasattr(scfq, "cycles_file")
    table, lines, ms, mq = table_of(open(os.path.join(GOLDEN, "edge", "n_rich.fq"), "rb").read())
    want = [(2, 0, 0, 0, 0, 2, 2, 66)] * 4 + [(1, 1, 0, 0, 0, 0, 1, 33), (1, 0, 1, 0, 0, 0, 1, 33), (1, 0, 0, 1, 0, 0, 1, 33), (1, 0, 0, 0, 1, 0, 1, 33)] + \
           [(1, 0, 0, 0, 0, 1, 1, 33)] * 2 + [(1, 0, 0, 1, 0, 0, 1, 33)] * 2 + [(1, 0, 1, 0, 0, 0, 1, 33)] * 2
    assert [tuple(r) for r in table.tolist()] == want and (lines, ms, mq) == (8, 14, 14)
    table, lines, ms, mq = table_of(open(os.path.join(GOLDEN, "edge", "many_short.fq"), "rb").read())
    assert table.shape == (8, 8) and (lines, ms, mq) == (1200, 8, 8)
    for p, letter in enumerate("ACGTNNGC"):
        col = 1 + "ACGTN".index(letter)
        assert table[p].tolist() == [300] + [300 if k == col else 0 for k in range(1, 6)] + [300, 10500 if p == 4 else 21900], p
    assert cli_text(table[:2], 1000, "\tx") == "1\t300\t300\t0\t0\t0\t0\t0\t300\t73.0\tx\n2\t300\t0\t300\t0\t0\t0\t0\t300\t73.0\tx\n"
    assert cli_text(table[:2], 1) == "1\t300\t300\t0\t0\t0\t0\t0\t300\t73.0\n>1\t300\t0\t300\t0\t0\t0\t0\t300\t73.0\n"

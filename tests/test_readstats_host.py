"""fq-readstats without a device: the ABI (symbols, struct layouts, C99 header), argument checks, the row formatter, the CLI's
header / help / open-error behaviour, and the checker itself against the CPU oracle."""
import ctypes
import glob
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG, ROOT
from _readstats_check import REC_FIELDS, lines_of, per_read, per_read_np, row_text, summary_of

SC = os.path.join(PKG, "sc")
HEADER = "reads\tbases\tmin_len\tmax_len\tmean_len\tn50\tl50\tn90\tl90\tmean_qual"
NEW = ("scfq_read_stats_buffer", "scfq_read_stats_file", "scfq_format_read_stats_tsv")


def run(*args):
    return subprocess.run([SC] + list(args), capture_output=True, text=True, stdin=subprocess.DEVNULL)


def test_symbols_declared_exported_and_listed(scfq):
    header = open(os.path.join(ROOT, "include", "sc_fqcount.h")).read()
    L = scfq.lib()
    for name in NEW:
        assert name + "(" in header and name in scfq.EXPORTS and hasattr(L, name), name


def test_struct_layouts(scfq):
    assert ctypes.sizeof(scfq.ReadRec) == 40
    assert [f[0] for f in scfq.ReadRec._fields_] == list(REC_FIELDS)
    S = scfq.ReadSummary
    names = ("struct_size", "abi_version", "reads", "lines", "input_bytes", "bases", "gc_bases", "n_bases", "qual_bytes", "qual_sum",
             "min_len", "max_len", "n50", "l50", "n90", "l90")
    for k, name in enumerate(names):
        assert getattr(S, name).offset == 8 * k, name
    assert S.len_hist.offset == 128 and S.gc_hist.offset == 128 + 8 * 65 and S.meanq_hist.offset == 128 + 8 * (65 + 102)
    assert S.no_qual.offset == 128 + 8 * (65 + 102 + 256) and ctypes.sizeof(S) == 8 * (16 + 65 + 102 + 256 + 1)


def test_header_is_c99_and_sizes_agree(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "sc_fqcount.h"\n'
                   "typedef char rec_is_40[sizeof(scfq_read_rec) == 40 ? 1 : -1];\n"
                   "typedef char sum_size[sizeof(scfq_read_summary) == 8 * (16 + 65 + 102 + 256 + 1) ? 1 : -1];\n"
                   "typedef char hist_at[offsetof(scfq_read_summary, len_hist) == 128 && offsetof(scfq_read_summary, no_qual) == 8 * (16 + 65 + 102 + 256) ? 1 : -1];\n"
                   "int main(void){ scfq_read_rec r; scfq_read_summary s; s.struct_size = sizeof s; r.seq_len = 0; (void)r; (void)s;\n"
                   "  return scfq_read_stats_buffer(0, 0, 0, 0, 0, &s) + scfq_format_read_stats_tsv(&s, 0, 0) + scfq_read_stats_file(\"x\", 0, &s) == 12345; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-fsyntax-only", str(src)])


def test_argument_checks(scfq):
    L = scfq.lib()
    s = scfq._new_read_summary()
    buf = ctypes.create_string_buffer(b"@a\nACGT\n+\nIIII\n")
    assert L.scfq_read_stats_buffer(buf, 15, 0, None, 0, None) == scfq.SCFQ_EARG                      # NULL summary
    bad = scfq.ReadSummary()                                                                           # struct_size not set
    assert L.scfq_read_stats_buffer(buf, 15, 0, None, 0, ctypes.byref(bad)) == scfq.SCFQ_EARG
    bad.struct_size = ctypes.sizeof(scfq.ReadSummary) - 8
    assert L.scfq_read_stats_buffer(buf, 15, 0, None, 0, ctypes.byref(bad)) == scfq.SCFQ_EARG
    assert L.scfq_read_stats_buffer(None, 15, 0, None, 0, ctypes.byref(s)) == scfq.SCFQ_EARG          # NULL pointer with n > 0
    assert L.scfq_read_stats_file(None, None, ctypes.byref(s)) == scfq.SCFQ_EARG
    assert L.scfq_read_stats_file(b"x.fq", None, ctypes.byref(bad)) == scfq.SCFQ_EARG
    assert L.scfq_format_read_stats_tsv(None, None, 0) == scfq.SCFQ_EARG


def test_no_gpu_means_loud_failure(scfq):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(scfq.ScfqError) as e:
        scfq.read_stats_host(b"@a\nACGT\n+\nIIII\n")
    assert e.value.rc == scfq.SCFQ_EHIP
    with pytest.raises(scfq.ScfqError) as e:
        scfq.read_stats_file(os.path.join(GOLDEN, "dup.fq"))
    assert e.value.rc == scfq.SCFQ_EHIP
    with pytest.raises(scfq.ScfqError) as e:
        scfq.read_stats_file(os.path.join(GOLDEN, "does_not_exist.fq"))
    assert e.value.rc == scfq.SCFQ_EOPEN


def test_row_formatter(scfq):
    s = scfq._new_read_summary()
    assert scfq.format_read_stats_tsv(s) == "0\t0\t0\t0\tnan\t0\t0\t0\t0\tnan"                        # 0/0 -> nan
    s.reads, s.bases, s.min_len, s.max_len, s.n50, s.l50, s.n90, s.l90 = 2, 300, 150, 150, 150, 1, 150, 2
    s.qual_bytes, s.qual_sum = 300, 300 * 70
    row = "2\t300\t150\t150\t150.0\t150\t1\t150\t2\t70.0"                                              # ".0" on a bare integer
    assert scfq.format_read_stats_tsv(s) == row
    s.bases, s.qual_sum = 301, 21001
    assert scfq.format_read_stats_tsv(s) == "2\t301\t150\t150\t150.5\t150\t1\t150\t2\t%s" % ("%.16g" % (21001 / 300))
    s.bases, s.qual_sum = 300, 21000
    L = scfq.lib()
    assert L.scfq_format_read_stats_tsv(ctypes.byref(s), None, 0) == len(row)                          # sizing call
    small = ctypes.create_string_buffer(8)
    assert L.scfq_format_read_stats_tsv(ctypes.byref(s), small, 8) == len(row) and small.value == row[:7].encode()
    exact = ctypes.create_string_buffer(len(row) + 1)
    assert L.scfq_format_read_stats_tsv(ctypes.byref(s), exact, len(row) + 1) == len(row) and exact.value.decode() == row


def test_cli_without_a_device():
    r = run("fq-readstats", "--help")
    assert r.returncode == 0 and "fq-readstats [options] [fastq ...]" in r.stdout and "--hist=len|gc|qual" in r.stdout
    assert "fq-readstats" in run("--help").stdout
    r = run("fq-readstats", "-t", "-b")
    assert (r.returncode, r.stdout, r.stderr) == (0, HEADER + "\tbasename\n", "")
    assert run("fq-readstats", "-tba").stdout == HEADER + "\tbasename\tabsolute\n"
    r = run("fq-readstats", "does_not_exist.fq")
    c = run("fq-count", "does_not_exist.fq")
    assert (r.returncode, r.stderr, r.stdout) == (c.returncode, c.stderr, c.stdout) == (2, "\x1b[31mError 2: Unable to open file: does_not_exist.fq\x1b[0m\n", "")
    r, c = run("fq-readstats", "missing.fq.gz"), run("fq-count", "missing.fq.gz")
    assert (r.returncode, r.stderr) == (c.returncode, c.stderr) and r.returncode == 1
    r, c = run("fq-readstats", "-b"), run("fq-count", "-b")
    assert (r.returncode, r.stderr) == (c.returncode, c.stderr) == (3, "\x1b[31mError 3: No FASTQ specified\x1b[0m\n")
    assert run("fq-readstats", "--bogus").returncode == 1


def golden_files():
    return sorted(glob.glob(os.path.join(GOLDEN, "*.fq")) + glob.glob(os.path.join(GOLDEN, "edge", "*.fq")))


def check_identity(oracle, data, ctx):
    """the checker's totals against the CPU oracle's counters"""
    rows = per_read(data)
    oc = oracle.count(np.frombuffer(data, dtype=np.uint8), "bytes")
    assert len(lines_of(data)) == oc.lines and len(rows) == oc.reads, ctx
    sums = [sum(r[k] for r in rows) for k in range(5)]
    hist = list(oc.qual_hist)
    assert sums == [oc.bases, oc.gc_bases, oc.n_bases, sum(hist), sum(b * c for b, c in enumerate(hist))], ctx
    arr, lines = per_read_np(np.frombuffer(data, dtype=np.uint8))
    assert lines == oc.lines and [tuple(int(v) for v in r) for r in arr] == rows, ctx


def test_checker_against_the_oracle(scfq, oracle):
    assert tuple(f[0] for f in scfq.ReadRec._fields_) == REC_FIELDS          # the rows the checker yields are the table's columns
    files = golden_files()
    assert len(files) >= 30
    for path in files:
        check_identity(oracle, open(path, "rb").read(), path)
    rng = np.random.default_rng(41)
    alphabets = (b"ACGTN@+I\r\n\n", b"\r\n\r\nGCN", b"ACGTNacgtn@+FI#:,\r\n\n\n", bytes(range(256)))
    for trial in range(1200):
        alpha = np.frombuffer(alphabets[trial % 4], dtype=np.uint8)
        data = bytes(rng.choice(alpha, int(rng.integers(0, 400))).astype(np.uint8))
        check_identity(oracle, data, (trial, data))


TABLE = {
    "edge/crlf_no_final.fq": (2, 11, 5, 6, 6, 1, 5, 2),
    "edge/n_rich.fq": (2, 18, 4, 14, 14, 1, 4, 2),
    "edge/blank_lines.fq": (3, 2, 0, 2, 2, 1, 2, 1),
    "edge/trunc5.fq": (2, 4, 0, 4, 4, 1, 4, 1),
    "novaseq.fq": (9, 9, 1, 1, 1, 5, 1, 9),
    "edge/many_short.fq": (300, 2400, 8, 8, 8, 150, 8, 270),
    "edge/long_line_50k.fq": (1, 50000, 50000, 50000, 50000, 1, 50000, 1),
    "edge/empty.fq": (0, 0, 0, 0, 0, 0, 0, 0),
}


def test_checker_literals(scfq):
    assert hasattr(scfq, "read_stats_file")
    for name, want in TABLE.items():
        s = summary_of(per_read(open(os.path.join(GOLDEN, name), "rb").read()))
        assert tuple(s[k] for k in ("reads", "bases", "min_len", "max_len", "n50", "l50", "n90", "l90")) == want, name
    assert row_text([(150, 60, 0, 150, 150 * 70)] * 2) == "2\t300\t150\t150\t150.0\t150\t1\t150\t2\t70.0"
    assert row_text([]) == "0\t0\t0\t0\tnan\t0\t0\t0\t0\tnan"

"""fq-kmers without a device: the ABI (symbols, struct layout, C99 header), argument checks, the row formatter, the CLI's
header / help / error behaviour, and the two checkers of _kmers_check.py against each other, the CPU oracle and literal tables."""
import ctypes
import glob
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG, ROOT
from _kmers_check import SUMMARY_FIELDS, cli_text, index_of, kmers_of, kmers_of_np, revcomp_index, totals_text, word_of
from test_gpu_parity import random_fastq_like

SC = os.path.join(PKG, "sc")
HEADER = "kmer\tcount"
TOTALS_HEADER = "k\twindows\tkmers\tskipped\tshort_lines\tdistinct\tmax_count"
NEW = ("scfq_kmers_buffer", "scfq_kmers_file", "scfq_format_kmer_tsv", "scfq_kmers_error_detail")
FASTQ = b"@h\nACGTN\n+\nIIIII\n"
KS = (1, 2, 7, 8, 12)


def run(*args):
    return subprocess.run([SC] + list(args), capture_output=True, text=True, stdin=subprocess.DEVNULL)


def test_symbols_declared_exported_and_listed(scfq):
    header = open(os.path.join(ROOT, "include", "sc_fqcount.h")).read()
    debug = open(os.path.join(ROOT, "include", "sc_fqcount_debug.h")).read()
    L = scfq.lib()
    for name in NEW:
        assert name + "(" in header and name in scfq.EXPORTS and hasattr(L, name), name
    assert "scfq_debug_kmers_stages(" in debug and "scfq_debug_kmers_stages" in scfq.EXPORTS and hasattr(L, "scfq_debug_kmers_stages")
    assert len(scfq.kmers_stages()) == 4
    assert "SCFQ_KMERS_CANONICAL" in header and scfq.SCFQ_KMERS_CANONICAL == 1
    for name in ("KmerSummary", "kmers_device", "kmers_host", "kmers_file", "format_kmer_tsv", "kmers_stages"):
        assert hasattr(scfq, name), name


def test_struct_layout(scfq):
    S = scfq.KmerSummary
    assert tuple(f[0] for f in S._fields_) == SUMMARY_FIELDS and len(SUMMARY_FIELDS) == 14
    for k, name in enumerate(SUMMARY_FIELDS):
        assert getattr(S, name).offset == 8 * k and getattr(S, name).size == 8, name
    assert ctypes.sizeof(S) == 8 * 14


def test_header_is_c99_and_sizes_agree(tmp_path):
    src = tmp_path / "t.c"
    offsets = " && ".join("offsetof(scfq_kmer_summary, %s) == %d" % (name, 8 * k) for k, name in enumerate(SUMMARY_FIELDS))
    src.write_text('#include <stddef.h>\n#include "sc_fqcount.h"\n#include "sc_fqcount_debug.h"\n'
                   "typedef char sum_size[sizeof(scfq_kmer_summary) == 8 * 14 ? 1 : -1];\n"
                   "typedef char at[" + offsets + " ? 1 : -1];\n"
                   "typedef char consts[SCFQ_KMERS_MAX_K == 12 && SCFQ_KMERS_CANONICAL == 1 ? 1 : -1];\n"
                   "int main(void){ scfq_kmer_summary s; uint64_t t[4]; double ms[4]; s.struct_size = sizeof s;\n"
                   "  return scfq_kmers_buffer(0, 0, 0, 1, SCFQ_KMERS_CANONICAL, t, 4, &s) + scfq_format_kmer_tsv(1, 3, 2, 0, 0)\n"
                   "         + scfq_kmers_file(\"x\", 0, 1, 0, 0, 0, &s) + scfq_debug_kmers_stages(ms, 4) + (scfq_kmers_error_detail() != 0) == 12345; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-fsyntax-only", str(src)])


def test_argument_checks(scfq):
    L = scfq.lib()
    s = scfq._new_kmer_summary()
    buf = ctypes.create_string_buffer(FASTQ)
    n = len(FASTQ)
    table = (ctypes.c_uint64 * 16)()
    ok = ctypes.byref(s)
    assert L.scfq_kmers_buffer(buf, n, 0, 2, 0, table, 16, None) == scfq.SCFQ_EARG                     # NULL summary
    bad = scfq.KmerSummary()                                                                          # struct_size not set
    assert L.scfq_kmers_buffer(buf, n, 0, 2, 0, table, 16, ctypes.byref(bad)) == scfq.SCFQ_EARG
    bad.struct_size = ctypes.sizeof(scfq.KmerSummary) - 8
    assert L.scfq_kmers_buffer(buf, n, 0, 2, 0, table, 16, ctypes.byref(bad)) == scfq.SCFQ_EARG
    assert L.scfq_kmers_buffer(None, n, 0, 2, 0, table, 16, ok) == scfq.SCFQ_EARG                      # NULL pointer with n > 0
    assert L.scfq_kmers_buffer(buf, n, 0, 2, 0, None, 16, ok) == scfq.SCFQ_EARG                        # NULL table with cap > 0
    assert L.scfq_kmers_error_detail() == b""
    for k in (0, 13, 1 << 31):
        assert L.scfq_kmers_buffer(buf, n, 0, k, 0, None, 0, ok) == scfq.SCFQ_EARG                     # k outside 1 .. 12
        assert (b"k = %d" % k) in L.scfq_kmers_error_detail() and b"12" in L.scfq_kmers_error_detail()
        assert L.scfq_kmers_file(b"x.fq", None, k, 0, None, 0, ok) == scfq.SCFQ_EARG
        assert (b"k = %d" % k) in L.scfq_kmers_error_detail()
    assert L.scfq_kmers_buffer(buf, n, 0, 2, 2, table, 16, ok) == scfq.SCFQ_EARG                       # unknown flag bits
    assert b"flag" in L.scfq_kmers_error_detail() and b"0x2" in L.scfq_kmers_error_detail()
    assert L.scfq_kmers_buffer(buf, n, 0, 2, 0x80000001, table, 16, ok) == scfq.SCFQ_EARG
    assert b"0x80000000" in L.scfq_kmers_error_detail()
    assert L.scfq_kmers_buffer(buf, n, 0, 2, 0, table, 15, ok) == scfq.SCFQ_EARG                       # 0 < cap < 4^k
    assert b"cap 15" in L.scfq_kmers_error_detail() and b"16" in L.scfq_kmers_error_detail()
    big = np.zeros(4 ** 7, dtype=np.uint64)
    assert L.scfq_kmers_buffer(buf, n, 0, 7, 0, ctypes.c_void_p(big.ctypes.data), 4 ** 7 - 1, ok) == scfq.SCFQ_EARG
    assert b"cap 16383" in L.scfq_kmers_error_detail() and b"16384" in L.scfq_kmers_error_detail()
    assert L.scfq_kmers_file(None, None, 2, 0, table, 16, ok) == scfq.SCFQ_EARG
    assert L.scfq_kmers_file(b"x.fq", None, 2, 0, table, 16, ctypes.byref(bad)) == scfq.SCFQ_EARG
    assert L.scfq_kmers_file(b"x.fq", None, 2, 0, None, 16, ok) == scfq.SCFQ_EARG
    assert L.scfq_kmers_file(b"x.fq", None, 2, 4, table, 16, ok) == scfq.SCFQ_EARG
    assert L.scfq_kmers_file(b"x.fq", None, 2, 0, table, 1, ok) == scfq.SCFQ_EARG
    with pytest.raises(scfq.ScfqError) as e:
        scfq.kmers_host(FASTQ, 13)
    assert e.value.rc == scfq.SCFQ_EARG and "k = 13" in str(e.value)
    with pytest.raises(scfq.ScfqError) as e:
        scfq.kmers_host(FASTQ, 7, table=np.zeros(4 ** 7 - 1, dtype=np.uint64))
    assert e.value.rc == scfq.SCFQ_EARG and "16383" in str(e.value)


def test_no_gpu_means_loud_failure(scfq):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    for table in (None, True):
        for flags in (0, scfq.SCFQ_KMERS_CANONICAL):
            with pytest.raises(scfq.ScfqError) as e:
                scfq.kmers_host(FASTQ, 3, flags, table)
            assert e.value.rc == scfq.SCFQ_EHIP
            with pytest.raises(scfq.ScfqError) as e:
                scfq.kmers_file(os.path.join(GOLDEN, "dup.fq"), 3, flags, table)
            assert e.value.rc == scfq.SCFQ_EHIP
    with pytest.raises(scfq.ScfqError) as e:
        scfq.kmers_file(os.path.join(GOLDEN, "does_not_exist.fq"), 3, 0, True)
    assert e.value.rc == scfq.SCFQ_EOPEN


def test_row_formatter(scfq):
    assert scfq.format_kmer_tsv(4, index_of(b"ACGT"), 12) == "ACGT\t12"
    assert scfq.format_kmer_tsv(1, 3, 5) == "T\t5"
    assert scfq.format_kmer_tsv(1, 0, 0) == "A\t0"
    assert scfq.format_kmer_tsv(12, 4 ** 12 - 1, 18446744073709551615) == "T" * 12 + "\t18446744073709551615"
    assert scfq.format_kmer_tsv(12, 0, 7) == "A" * 12 + "\t7"
    for k, v in ((3, 27), (7, 12345), (12, 1234567)):
        assert scfq.format_kmer_tsv(k, v, v) == "%s\t%d" % (word_of(v, k), v) and index_of(word_of(v, k).encode()) == v
    L = scfq.lib()
    row = "ACGT\t12"
    assert L.scfq_format_kmer_tsv(4, 27, 12, None, 0) == len(row)                                      # sizing call
    small = ctypes.create_string_buffer(6)
    assert L.scfq_format_kmer_tsv(4, 27, 12, small, 6) == len(row) and small.value == row[:5].encode()
    exact = ctypes.create_string_buffer(len(row) + 1)
    assert L.scfq_format_kmer_tsv(4, 27, 12, exact, len(row) + 1) == len(row) and exact.value.decode() == row
    for k, v in ((0, 0), (13, 0), (1, 4), (12, 4 ** 12)):
        assert L.scfq_format_kmer_tsv(k, v, 1, None, 0) == scfq.SCFQ_EARG


def test_cli_without_a_device():
    r = run("fq-kmers", "--help")
    assert r.returncode == 0 and "fq-kmers [options] [fastq ...]" in r.stdout
    for opt in ("--k=N", "--canonical", "--top=N", "--totals", "-t, --header", "-b, --basename", "-a, --absolute"):
        assert opt in r.stdout, opt
    assert run("fq-kmers").stdout == r.stdout
    top = run("--help").stdout
    assert "fq-kmers" in top and top.index("fq-cycles") < top.index("fq-kmers")
    r = run("fq-kmers", "-t", "-b")
    assert (r.returncode, r.stdout, r.stderr) == (0, HEADER + "\tbasename\n", "")
    assert run("fq-kmers", "-tba").stdout == HEADER + "\tbasename\tabsolute\n"
    assert run("fq-kmers", "--header", "--k=12", "--canonical", "--top=0").stdout == HEADER + "\n"
    assert run("fq-kmers", "--header", "--totals").stdout == TOTALS_HEADER + "\n"
    assert run("fq-kmers", "-tba", "--totals").stdout == TOTALS_HEADER + "\tbasename\tabsolute\n"
    r = run("fq-kmers", "does_not_exist.fq")
    c = run("fq-cycles", "does_not_exist.fq")
    assert (r.returncode, r.stderr, r.stdout) == (c.returncode, c.stderr, c.stdout) == (2, "\x1b[31mError 2: Unable to open file: does_not_exist.fq\x1b[0m\n", "")
    r, c = run("fq-kmers", "missing.fq.gz"), run("fq-cycles", "missing.fq.gz")
    assert (r.returncode, r.stderr) == (c.returncode, c.stderr) and r.returncode == 1
    r, c = run("fq-kmers", "-b"), run("fq-cycles", "-b")
    assert (r.returncode, r.stderr) == (c.returncode, c.stderr) == (3, "\x1b[31mError 3: No FASTQ specified\x1b[0m\n")
    r, c = run("fq-kmers", "--bogus"), run("fq-cycles", "--bogus")
    assert (r.returncode, r.stderr) == (c.returncode, c.stderr) and r.returncode == 1
    r, c = run("fq-kmers", "-x"), run("fq-cycles", "-x")
    assert (r.returncode, r.stderr) == (c.returncode, c.stderr) and r.returncode == 1
    for bad in ("--k=0", "--k=13", "--k=x", "--k=", "--top=-1", "--k=-1", "--k=1.5", "--top=", "--top=x", "--k", "--top"):
        for totals in ((), ("--totals",)):
            r = run("fq-kmers", "-t", bad, *totals)
            assert r.returncode == 1 and HEADER not in r.stdout and TOTALS_HEADER not in r.stdout and "Error" in r.stderr, bad


def golden_files():
    return sorted(glob.glob(os.path.join(GOLDEN, "*.fq")) + glob.glob(os.path.join(GOLDEN, "edge", "*.fq")))


def check_agree(data, ctx, ks=KS):
    """the plain checker against the numpy one; the identities every result has to keep"""
    a = np.frombuffer(data, dtype=np.uint8)
    for k in ks:
        for canonical in (False, True):
            p = kmers_of(data, k, canonical)
            q = kmers_of_np(a, k, canonical)
            assert p == q, (ctx, k, canonical, p[1:], q[1:])
            table, windows, kmers, skipped, short, lines = p
            assert windows == kmers + skipped and sum(table.values()) == kmers, (ctx, k, canonical)
            assert all(0 <= v < 4 ** k and c > 0 for v, c in table.items()), (ctx, k, canonical)
            if canonical:
                assert all(v <= revcomp_index(v, k) for v in table), (ctx, k)
                plain = kmers_of(data, k)
                folded = {}
                for v, c in plain[0].items():
                    m = min(v, revcomp_index(v, k))
                    folded[m] = folded.get(m, 0) + c
                assert folded == table and plain[1:] == p[1:], (ctx, k)
            d = kmers_of_np(a, k, canonical, dense=True)
            assert d[1:] == p[1:] and d[0].dtype == np.uint64 and d[0].shape == (4 ** k,), (ctx, k, canonical)
            if k <= 8:
                assert {int(v): int(d[0][v]) for v in np.flatnonzero(d[0])} == table, (ctx, k, canonical)


def test_checkers_agree_on_the_fixtures(scfq):
    assert hasattr(scfq, "kmers_file")
    files = golden_files()
    assert len(files) >= 30
    for path in files:
        data = open(path, "rb").read()
        check_agree(data, path, ks=KS if len(data) < 200_000 else (1, 7, 12))


@pytest.mark.parametrize("kind", ["uniform", "ascii", "dense_nl", "sparse_nl", "crlf"])
def test_checkers_agree_on_random_buffers(scfq, kind):
    assert hasattr(scfq, "kmers_device")
    rng = np.random.default_rng(47)
    for n in (0, 1, 2, 15, 16, 17, 255, 4096, 20_000):
        a = random_fastq_like(rng, n, kind)
        for cut in (n, n - 1, 2 * n // 3):
            if cut >= 0:
                check_agree(bytes(a[:cut]), (kind, n, cut))


def test_checker_against_the_oracle_at_k_1(scfq, oracle):
    assert hasattr(scfq, "kmers_host")
    for path in golden_files():
        data = open(path, "rb").read()
        oc = oracle.count(np.frombuffer(data, dtype=np.uint8), "bytes")
        table, windows, kmers, skipped, short, lines = kmers_of(data, 1)
        assert lines == oc.lines and windows == oc.bases, path
        assert table.get(1, 0) + table.get(2, 0) == oc.gc_bases and skipped >= oc.n_bases, path


def test_literal_tables(scfq):
    assert hasattr(scfq, "format_kmer_tsv")
    ix = index_of
    data = b"@h\nACGTN\n+\nIIIII\n"
    assert kmers_of(data, 2) == ({ix(b"AC"): 1, ix(b"CG"): 1, ix(b"GT"): 1}, 4, 3, 1, 0, 4)
    assert kmers_of(data, 2, True) == ({ix(b"AC"): 2, ix(b"CG"): 1}, 4, 3, 1, 0, 4)
    assert cli_text(kmers_of(data, 2)[0], 2) == "AC\t1\nCG\t1\nGT\t1\n"
    assert cli_text(kmers_of(data, 2, True)[0], 2, "\tx", top=1) == "AC\t2\tx\n"
    many = open(os.path.join(GOLDEN, "edge", "many_short.fq"), "rb").read()
    assert kmers_of(many, 2) == ({ix(b"AC"): 300, ix(b"CG"): 300, ix(b"GC"): 300, ix(b"GT"): 300}, 2100, 1200, 900, 0, 1200)
    assert kmers_of(many, 8) == ({}, 300, 0, 300, 0, 1200)
    assert kmers_of(many, 9) == ({}, 0, 0, 0, 300, 1200)
    assert cli_text(kmers_of(many, 2)[0], 2) == "AC\t300\nCG\t300\nGC\t300\nGT\t300\n"
    assert cli_text(kmers_of(many, 2)[0], 2, top=3) == "AC\t300\nCG\t300\nGC\t300\n"
    assert totals_text(kmers_of(many, 2), 2, "\tmany_short.fq") == "2\t2100\t1200\t900\t0\t4\t300\tmany_short.fq\n"
    assert totals_text(kmers_of(many, 9), 9) == "9\t0\t0\t0\t300\t0\t0\n"
    # the final '\r' of an input without a final '\n' is text; the '\r' before a real '\n' is not
    assert kmers_of(b"@h\nACGT\r", 4)[:4] == ({ix(b"ACGT"): 1}, 2, 1, 1) and kmers_of(b"@h\nACGT\r", 5)[:4] == ({}, 1, 0, 1)
    assert kmers_of(b"@h\nACGT\r\n", 4)[:5] == ({ix(b"ACGT"): 1}, 1, 1, 0, 0) and kmers_of(b"@h\nACGT\r\n", 5)[:5] == ({}, 0, 0, 0, 1)
    assert kmers_of(b"@h\nACGT", 4)[:4] == ({ix(b"ACGT"): 1}, 1, 1, 0)
    # a palindrome is counted once per occurrence
    assert kmers_of(b"@h\nACGT\n", 4, True)[:3] == ({ix(b"ACGT"): 1}, 1, 1) and revcomp_index(ix(b"ACGT"), 4) == ix(b"ACGT")
    assert kmers_of(b"@h\nTTTT\n", 3, True)[0] == {0: 2}

"""fq-kcount without a device: the ABI (symbols, struct layout, C99 header), every argument check (all come before the first HIP
call), the row formatter, the grammar of `sc fq-kcount`, and the checker of _kcount_check.py against literal, hand-worked cases,
against its numpy form and against the committed fixture."""
import ctypes
import glob
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG, ROOT
from _kcount_check import (CANONICAL, DUMP_HEADER, EARG, EFULL, EHIP, HIST_HEADER, SUMMARY_FIELDS, TOTALS_HEADER, canonical_key, dump_of, hist_of,
                           hist_text, kcount_of, kcount_of_np, rows_text, top_of, totals_text)
from _kmers_check import index_of, revcomp_index, word_of

SC = os.path.join(PKG, "sc")
KCOUNT = os.path.join(GOLDEN, "kcount")
NEW = ("scfq_kcount_buffers", "scfq_kcount_files", "scfq_kcount_hist", "scfq_kcount_dump", "scfq_kcount_query", "scfq_kcount_free",
       "scfq_format_kcount_tsv", "scfq_kcount_error_detail")
FASTQ = b"@h\nACGTACGTACGTACGTN\n+\nIIIIIIIIIIIIIIIII\n"


def run(*args):
    return subprocess.run([SC] + list(args), capture_output=True, text=True, stdin=subprocess.DEVNULL)


def fq(*seqs):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(seqs))


# ---- the checker, by hand -----------------------------------------------------------------------------------------------------
def test_checker_literal_cases():
    ix = index_of
    # 15 letters at k = 13: three windows
    w = kcount_of(fq(b"ACGTACGTACGTACG"), 13)
    assert w.table == {ix(b"ACGTACGTACGTA"): 1, ix(b"CGTACGTACGTAC"): 1, ix(b"GTACGTACGTACG"): 1}
    assert (w.windows, w.kmers, w.skipped, w.short_lines, w.lines, w.reads, w.input_bytes) == (3, 3, 0, 0, 4, 1, 38)
    assert (w.distinct, w.unique, w.max_count) == (3, 3, 1)
    # canonical: CGTACGTACGTAC is the reverse complement of GTACGTACGTACG
    assert revcomp_index(ix(b"GTACGTACGTACG"), 13) == ix(b"CGTACGTACGTAC")
    w = kcount_of(fq(b"ACGTACGTACGTACG"), 13, True)
    assert w.table == {ix(b"ACGTACGTACGTA"): 1, ix(b"CGTACGTACGTAC"): 2} and (w.distinct, w.unique, w.max_count) == (2, 1, 2)
    # a palindrome at k = 14 is counted once per occurrence
    pal = b"ACGTACG" + b"CGTACGT"
    assert revcomp_index(ix(pal), 14) == ix(pal)
    w = kcount_of(fq(pal, pal), 14, True)
    assert w.table == {ix(pal): 2} and (w.windows, w.kmers, w.unique) == (2, 2, 0)
    assert kcount_of(fq(pal, pal), 14).table == {ix(pal): 2}
    # 32 T: the all-ones key in plain mode, key 0 in canonical mode
    t40 = fq(b"T" * 40)
    assert kcount_of(t40, 32).table == {2 ** 64 - 1: 9} and ix(b"T" * 32) == 2 ** 64 - 1
    assert kcount_of(t40, 32, True).table == {0: 9}
    assert kcount_of(fq(b"T" * 40, b"A" * 40), 32).table == {2 ** 64 - 1: 9, 0: 9}
    assert kcount_of(fq(b"T" * 40, b"A" * 40), 32, True).table == {0: 18}
    # two inputs are summed, short lines and skipped windows included
    a, b = fq(b"ACGTACGTACGTACG", b"ACGT"), fq(b"ACGTACGTACGTANG")
    w = kcount_of([a, b], 13)
    assert w.table == {ix(b"ACGTACGTACGTA"): 2, ix(b"CGTACGTACGTAC"): 1, ix(b"GTACGTACGTACG"): 1}
    assert (w.windows, w.kmers, w.skipped, w.short_lines, w.lines, w.reads, w.input_bytes) == (6, 4, 2, 1, 12, 3, len(a) + len(b))
    assert (w.distinct, w.unique, w.max_count) == (3, 2, 2)
    assert kcount_of([a, b""], 13) == kcount_of(a, 13) != kcount_of([a, b], 13)


def test_checker_readers():
    table = {5: 1, 9: 3, 2: 3, 7: 10, 1: 2}
    assert hist_of(table, 2) == [0, 5]
    assert hist_of(table, 4) == [0, 1, 1, 3]
    assert hist_of(table, 11) == [0, 1, 1, 2, 0, 0, 0, 0, 0, 0, 1] and hist_of(table, 12) == [0, 1, 1, 2, 0, 0, 0, 0, 0, 0, 1, 0]
    assert dump_of(table) == [(1, 2), (2, 3), (5, 1), (7, 10), (9, 3)]
    assert dump_of(table, 3) == [(2, 3), (7, 10), (9, 3)] and dump_of(table, 2, 3) == [(1, 2), (2, 3), (9, 3)] and dump_of(table, 11) == []
    assert top_of(table, 2) == [(7, 10), (2, 3)] and top_of(table, 3) == [(7, 10), (2, 3), (9, 3)] and top_of(table, 0) == []
    assert len(top_of(table, 99)) == 5
    assert hist_text(table) == "1\t1\n2\t1\n3\t2\n4\t0\n5\t0\n6\t0\n7\t0\n8\t0\n9\t0\n10\t1\n"
    assert hist_text(table, high=3) == "1\t1\n2\t1\n3\t2\n4\t1\n" and hist_text(table, high=2, suffix="\tx") == "1\t1\tx\n2\t1\tx\n3\t3\tx\n"
    assert hist_text({}, high=5) == ""
    assert rows_text([(0, 4), (1, 2)], 13, "\tf") == "AAAAAAAAAAAAA\t4\tf\nAAAAAAAAAAAAC\t2\tf\n"
    assert canonical_key(index_of(b"T" * 13), 13) == 0 and canonical_key(0, 32) == 0 and canonical_key(2 ** 64 - 1, 32) == 0


def golden_files():
    return sorted(glob.glob(os.path.join(GOLDEN, "*.fq")) + glob.glob(os.path.join(GOLDEN, "edge", "*.fq")))


def test_checker_forms_agree():
    files = [p for p in golden_files() if os.path.getsize(p) < 60_000]
    assert len(files) >= 20
    for path in files:
        data = open(path, "rb").read()
        a = np.frombuffer(data, dtype=np.uint8)
        for k in (13, 21, 32):
            for canonical in (False, True):
                assert kcount_of(data, k, canonical) == kcount_of_np(a, k, canonical), (path, k, canonical)
    data = fq(b"T" * 40, b"A" * 40, b"ACGTNACGT" * 9, b"acgt" * 20)
    a = np.frombuffer(data, dtype=np.uint8)
    for k in (13, 31, 32):
        for canonical in (False, True):
            assert kcount_of([data, data[:91]], k, canonical) == kcount_of_np([a, a[:91]], k, canonical), (k, canonical)


def test_fixture_is_what_its_generator_writes():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_kcount", os.path.join(KCOUNT, "make_kcount.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    data = m.make_reads()
    assert data == open(os.path.join(KCOUNT, "reads.fq"), "rb").read()
    for name, text in m.expected(data).items():
        assert text == open(os.path.join(KCOUNT, name)).read(), name
    want = kcount_of(data, m.K, True)
    h = hist_of(want.table, 40)
    assert h[1] > 10 * h[4] and max(range(5, 40), key=lambda c: h[c]) in range(10, 21)      # an error peak and a coverage peak
    top = top_of(want.table, 11)
    assert top[9][1] == top[10][1] and top[9][0] < top[10][0]                                # the tie across the cut
    assert os.path.getsize(os.path.join(KCOUNT, "reads.fq")) < 1 << 20


# ---- the ABI ----------------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_listed(scfq):
    header = open(os.path.join(ROOT, "include", "sc_fqcount.h")).read()
    debug = open(os.path.join(ROOT, "include", "sc_fqcount_debug.h")).read()
    L = scfq.lib()
    for name in NEW:
        assert name + "(" in header and name in scfq.EXPORTS and hasattr(L, name), name
    assert "scfq_debug_kcount_stages(" in debug and "scfq_debug_kcount_stages" in scfq.EXPORTS and hasattr(L, "scfq_debug_kcount_stages")
    assert len(scfq.kcount_stages()) == 4
    assert (scfq.SCFQ_KCOUNT_MIN_K, scfq.SCFQ_KCOUNT_MAX_K, scfq.SCFQ_KCOUNT_CANONICAL, scfq.SCFQ_EFULL) == (13, 32, 1, EFULL)
    assert scfq.SCFQ_EARG == EARG and scfq.SCFQ_EHIP == EHIP
    assert scfq.strerror(EFULL) != scfq.strerror(-99) and "full" in scfq.strerror(EFULL)
    for name in ("KcountSummary", "KcountOpts", "KmerCount", "KcountTable", "kcount_device", "kcount_host", "kcount_files", "format_kcount_tsv",
                 "kcount_stages"):
        assert hasattr(scfq, name), name
    for name in ("hist", "dump", "query", "close"):
        assert hasattr(scfq.KcountTable, name), name
    assert "SCFQ_KMERS_MAX_K     12" in header                                               # fq-kmers keeps its limit


def test_struct_layout(scfq):
    S = scfq.KcountSummary
    assert tuple(f[0] for f in S._fields_) == SUMMARY_FIELDS == scfq.KCOUNT_SUMMARY_FIELDS and len(SUMMARY_FIELDS) == 16
    for i, name in enumerate(SUMMARY_FIELDS):
        assert getattr(S, name).offset == 8 * i and getattr(S, name).size == 8, name
    assert ctypes.sizeof(S) == 128 and ctypes.sizeof(scfq.KcountOpts) == 24 and ctypes.sizeof(scfq.KmerCount) == 16
    O = scfq.KcountOpts
    assert [(getattr(O, n).offset, getattr(O, n).size) for n in ("struct_size", "k", "flags", "table_bits", "reserved")] == \
        [(0, 8), (8, 4), (12, 4), (16, 4), (20, 4)]


def test_header_is_c99_and_sizes_agree(tmp_path):
    src = tmp_path / "t.c"
    offsets = " && ".join("offsetof(scfq_kcount_summary, %s) == %d" % (name, 8 * i) for i, name in enumerate(SUMMARY_FIELDS))
    src.write_text('#include <stddef.h>\n#include "sc_fqcount.h"\n#include "sc_fqcount_debug.h"\n'
                   "typedef char sum_size[sizeof(scfq_kcount_summary) == 128 && sizeof(scfq_kcount_opts) == 24 && sizeof(scfq_kmer_count) == 16 ? 1 : -1];\n"
                   "typedef char at[" + offsets + " ? 1 : -1];\n"
                   "typedef char consts[SCFQ_KCOUNT_MIN_K == 13 && SCFQ_KCOUNT_MAX_K == 32 && SCFQ_KCOUNT_CANONICAL == 1 && SCFQ_EFULL == -10\n"
                   "                    && SCFQ_KMERS_MAX_K == 12 ? 1 : -1];\n"
                   "int main(void){ scfq_kcount_summary s; scfq_kcount_opts o; scfq_kcount* t = 0; scfq_kmer_count r; uint64_t h[4], n; double ms[4];\n"
                   "  s.struct_size = sizeof s; o.struct_size = sizeof o; o.k = 21; o.flags = 0; o.table_bits = 0; o.reserved = 0;\n"
                   "  return scfq_kcount_buffers(0, 0, 0, 0, 0, &o, &t, &s) + scfq_kcount_files(\"x\", 0, 0, &o, &t, &s) + scfq_kcount_hist(t, h, 4)\n"
                   "         + scfq_kcount_dump(t, 1, 0, &r, 1, &n) + scfq_kcount_query(t, h, 1, h) + scfq_format_kcount_tsv(13, 3, 2, 0, 0)\n"
                   "         + scfq_debug_kcount_stages(ms, 4) + (scfq_kcount_error_detail() != 0) + (scfq_kcount_free(t), 0) == 12345; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-fsyntax-only", str(src)])


def test_argument_checks(scfq):
    """every SCFQ_EARG of the contract; none of them needs a device"""
    L = scfq.lib()
    buf = ctypes.create_string_buffer(FASTQ)
    n = len(FASTQ)
    detail = L.scfq_kcount_error_detail

    def call(opts, s=None, want_table=True, r1=buf, n1=n, r2=None, n2=0):
        h = ctypes.c_void_p(0x1234)
        s = scfq._new_kcount_summary() if s is None else s
        rc = L.scfq_kcount_buffers(r1, n1, r2, n2, 0, ctypes.byref(opts) if opts is not None else None, ctypes.byref(h) if want_table else None,
                                   ctypes.byref(s) if s is not False else None)
        if want_table:
            assert h.value is None, "*out is NULL after a failure"
        return rc

    for k in (0, 1, 12, 33, 64, 1 << 31):
        assert call(scfq.kcount_opts(k)) == EARG and (b"k = %d" % k) in detail() and b"13" in detail() and b"32" in detail()
        s = scfq._new_kcount_summary()
        assert L.scfq_kcount_files(b"x.fq", None, None, ctypes.byref(scfq.kcount_opts(k)), None, ctypes.byref(s)) == EARG
        assert (b"k = %d" % k) in detail()
    for flags, text in ((2, b"0x2"), (0x80000001, b"0x80000000"), (0xfffffffe, b"0xfffffffe")):
        assert call(scfq.kcount_opts(21, flags)) == EARG and b"flag" in detail() and text in detail()
    for bits in (1, 9, 33, 64, 1 << 31):
        assert call(scfq.kcount_opts(21, 0, bits)) == EARG and (b"table_bits = %d" % bits) in detail()
    assert call(scfq.kcount_opts(21, 0, 0, reserved=1)) == EARG and b"reserved" in detail()
    bad = scfq.kcount_opts(21)
    bad.struct_size -= 8
    assert call(bad) == EARG and b"opts->struct_size" in detail()
    bad.struct_size = 0
    assert call(bad) == EARG and call(None) == EARG and b"opts" in detail()
    for size in (0, 120, 136):
        s = scfq.KcountSummary()
        s.struct_size = size
        assert call(scfq.kcount_opts(21), s) == EARG and b"sum->struct_size" in detail()
    assert call(scfq.kcount_opts(21), False, want_table=False) == EARG and detail() != b""     # neither a table nor a summary
    assert call(scfq.kcount_opts(21), r1=None) == EARG and b"NULL input" in detail()            # NULL pointer with n > 0
    assert call(scfq.kcount_opts(21), r2=None, n2=5) == EARG and b"NULL input" in detail()
    s = scfq._new_kcount_summary()
    assert L.scfq_kcount_files(None, None, None, ctypes.byref(scfq.kcount_opts(21)), None, ctypes.byref(s)) == EARG and b"path1" in detail()
    # the readers of a table
    h = (ctypes.c_uint64 * 4)()
    total = ctypes.c_uint64()
    row = scfq.KmerCount()
    assert L.scfq_kcount_hist(None, h, 4) == EARG and L.scfq_kcount_dump(None, 1, 0, ctypes.byref(row), 1, ctypes.byref(total)) == EARG
    assert L.scfq_kcount_query(None, h, 1, h) == EARG
    fake = ctypes.c_void_p(0x1000)          # (never dereferenced: the checks come first)
    for bins in (0, 1, (1 << 20) + 1, 1 << 40):
        assert L.scfq_kcount_hist(fake, h, bins) == EARG and (b"bins = %d" % bins) in detail()
    assert L.scfq_kcount_hist(fake, None, 4) == EARG
    assert L.scfq_kcount_dump(fake, 1, 0, None, 1, ctypes.byref(total)) == EARG and L.scfq_kcount_dump(fake, 1, 0, ctypes.byref(row), 1, None) == EARG
    assert L.scfq_kcount_query(fake, None, 1, h) == EARG and L.scfq_kcount_query(fake, h, 1, None) == EARG
    L.scfq_kcount_free(None)
    with pytest.raises(scfq.ScfqError) as e:
        scfq.kcount_host(FASTQ, k=12)
    assert e.value.rc == EARG and "k = 12" in str(e.value)
    with pytest.raises(scfq.ScfqError) as e:
        scfq.kcount_host(FASTQ, k=21, table_bits=9)
    assert e.value.rc == EARG and "table_bits = 9" in str(e.value)


def test_no_gpu_means_loud_failure(scfq):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    for flags in (0, CANONICAL):
        for table in (False, True):
            with pytest.raises(scfq.ScfqError) as e:
                scfq.kcount_host(FASTQ, FASTQ, k=13, flags=flags, table=table)
            assert e.value.rc == EHIP and e.value.handle is None
            with pytest.raises(scfq.ScfqError) as e:
                scfq.kcount_files(os.path.join(KCOUNT, "reads.fq"), k=21, flags=flags, table=table)
            assert e.value.rc == EHIP
    with pytest.raises(scfq.ScfqError) as e:
        scfq.kcount_files(os.path.join(GOLDEN, "does_not_exist.fq"))
    assert e.value.rc == scfq.SCFQ_EOPEN


def test_row_formatter(scfq):
    f = scfq.format_kcount_tsv
    assert f(13, index_of(b"ACGTACGTACGTA"), 12) == "ACGTACGTACGTA\t12"
    assert f(13, 0, 0) == "A" * 13 + "\t0" and f(13, 4 ** 13 - 1, 5) == "T" * 13 + "\t5"
    assert f(32, 2 ** 64 - 1, 2 ** 64 - 1) == "T" * 32 + "\t18446744073709551615"
    assert f(32, 0, 7) == "A" * 32 + "\t7" and f(32, 1 << 63, 1) == "G" + "A" * 31 + "\t1"
    for k, v in ((13, 12345678), (21, 0x123456789AB), (31, 0x2AAAAAAAAAAAAAAA), (32, 0xFEDCBA9876543210)):
        assert f(k, v, v) == "%s\t%d" % (word_of(v, k), v) and index_of(word_of(v, k).encode()) == v
    L = scfq.lib()
    row = "ACGTACGTACGTA\t12"
    key = index_of(b"ACGTACGTACGTA")
    assert L.scfq_format_kcount_tsv(13, key, 12, None, 0) == len(row)                          # sizing call
    small = ctypes.create_string_buffer(b"#" * 8, 8)
    assert L.scfq_format_kcount_tsv(13, key, 12, small, 6) == len(row) and small.raw == row[:5].encode() + b"\0##"
    exact = ctypes.create_string_buffer(len(row) + 1)
    assert L.scfq_format_kcount_tsv(13, key, 12, exact, len(row) + 1) == len(row) and exact.value.decode() == row
    for k, v in ((0, 0), (12, 0), (33, 0), (13, 4 ** 13), (31, 4 ** 31), (31, 2 ** 64 - 1)):
        assert L.scfq_format_kcount_tsv(k, v, 1, None, 0) == EARG, (k, v)
    # fq-kmers' formatter keeps its range
    assert L.scfq_format_kmer_tsv(13, 0, 1, None, 0) == EARG and scfq.format_kmer_tsv(12, 0, 7) == "A" * 12 + "\t7"


# ---- the command ------------------------------------------------------------------------------------------------------------
def test_cli_without_a_device():
    r = run("fq-kcount", "--help")
    assert r.returncode == 0 and r.stderr == "" and "fq-kcount [options] IN.fq [IN2.fq]" in r.stdout
    for opt in ("--k=N", "--canonical", "--table-bits=N", "--high=N", "--totals", "--dump", "--min-count=C", "--max-count=C", "--top=N",
                "-t, --header", "-b, --basename", "-a, --absolute"):
        assert opt in r.stdout, opt
    assert run("fq-kcount").stdout == r.stdout and run("fq-kcount", "-h").stdout == r.stdout
    assert "fq-kcount" not in run("--help").stdout                                           # listed in its own help only
    assert run("fq-kcount", "-t").stdout == HIST_HEADER + "\n"
    assert run("fq-kcount", "-t", "-b", "--k=13", "--canonical", "--high=1").stdout == HIST_HEADER + "\tbasename\n"
    assert run("fq-kcount", "-tba", "--totals", "--k=32").stdout == TOTALS_HEADER + "\tbasename\tabsolute\n"
    assert run("fq-kcount", "--header", "--dump", "--min-count=5", "--max-count=5").stdout == DUMP_HEADER + "\n"
    assert run("fq-kcount", "--header", "--top=0", "--table-bits=10").stdout == DUMP_HEADER + "\n"
    r = run("fq-kcount", "does_not_exist.fq")
    assert (r.returncode, r.stderr, r.stdout) == (2, "\x1b[31mError 2: Unable to open file: does_not_exist.fq\x1b[0m\n", "")
    r = run("fq-kcount", "-b")
    assert (r.returncode, r.stderr) == (3, "\x1b[31mError 3: No FASTQ specified\x1b[0m\n")
    usage = ["--k=12", "--k=33", "--k=0", "--k=x", "--k=", "--k", "--high=0", "--high=1048575", "--high=x", "--table-bits=9", "--table-bits=33",
             "--top=-1", "--top=", "--top", "--top=18446744073709551615", "--top=1000000000000000000", "--min-count=0", "--bogus", "--dump=1"]
    pairs = [("--top=3", "--dump"), ("--top=3", "--totals"), ("--dump", "--totals"), ("--min-count=2",), ("--max-count=2", "--top=1"),
             ("--dump", "--min-count=3", "--max-count=2"), ("a.fq", "b.fq", "c.fq")]
    for bad in [(u,) for u in usage] + pairs:
        r = run("fq-kcount", "-t", *bad)
        assert r.returncode == 1 and "Error" in r.stderr and "Usage:" in r.stdout, bad
        for header in (HIST_HEADER, DUMP_HEADER, TOTALS_HEADER):
            assert "\n" + header + "\n" not in "\n" + r.stdout, bad
    # fq-kmers still refuses what is this command's range
    assert run("fq-kmers", "--k=13", "x.fq").returncode == 1 and run("fq-kmers", "--k=12", "-t").returncode == 0

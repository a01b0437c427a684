"""fa-gc without a device: the checker of _fa_gc_check.py against the reference's pins, the three host helpers against the
checker, position parsing and order (the Python mirror and the CLI's stderr), and the ABI (symbols, struct layout, C99 header,
argument checks, SCFQ_EHIP without a device)."""
import ctypes
import gzip
import io
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG, ROOT
from _fa_gc_check import PINS, FaModel, c_round, cli_text, gc_interval, order, parse_positions, parse_window, value_text, warning_line

SC = os.path.join(PKG, "sc")
FASTA = os.path.join(GOLDEN, "fasta", "test.fasta")
NEW = ("scfq_fa_index_buffer", "scfq_fa_index_file", "scfq_fa_contig_at", "scfq_fa_contig_find", "scfq_fa_count_intervals",
       "scfq_fa_index_free", "scfq_fa_error_detail", "scfq_fa_parse_window", "scfq_fa_gc_interval", "scfq_format_fa_gc_value")
SUMMARY_FIELDS = ("struct_size", "abi_version", "input_bytes", "tiles", "contigs", "bases", "gc_bases", "acgt_bases", "orphan_bases")
SMALL = b">a\nACGT\n"


def run(*args):
    return subprocess.run([SC] + list(args), capture_output=True, text=True, stdin=subprocess.DEVNULL)


def red(code, msg):
    return "\x1b[31mError %d: %s\x1b[0m\n" % (code, msg)


@pytest.fixture(scope="module")
def fixture_model():
    return FaModel(open(FASTA, "rb").read())


# ---- the checker itself ----------------------------------------------------------------------------------------------

def test_checker_on_the_fixture_and_the_pins(scfq, fixture_model):
    assert hasattr(scfq, "fa_gc")
    m = fixture_model
    assert os.path.getsize(FASTA) == 3021
    assert [(c[0], c[3]) for c in m.contigs] == [(b"chr1", 1000), (b"chr2", 1000), (b"chr3", 1000)]
    assert m.bases == 3000 and m.orphan_bases == 0
    for pos, wtext, cell, counts in PINS:
        (chrom, p), = parse_positions(pos)[0]
        w = parse_window(wtext)
        c = m.find(chrom)
        b, e = gc_interval(p, w, m.contigs[c][3])
        assert m.count(c, b, e)[:2] == counts == m.count_slow(c, b, e)[:2], pos
        assert value_text(*counts, w) == cell, pos
        out, err = cli_text(m, [(chrom, p)], [w])
        assert out == "chrom\tpos\tgc_%d\n%s\t%d\t%s\n" % (2 * w, chrom, p, cell) and err == ""


def test_checker_on_handmade_inputs(scfq):
    assert hasattr(scfq, "fa_index_host")
    m = FaModel(b"NNgc\n>one two\nAC GT\r\n\nac>gt\n>\n>two\tx\nRYN")
    assert m.orphan_bases == 4 and m.bases == 4 + 9 + 0 + 3
    assert [(c[0], c[3]) for c in m.contigs] == [(b"one", 9), (b"", 0), (b"two", 3)]
    assert m.count(0, 0, 9) == (4, 8, 9) == m.count_slow(0, 0, 9) and m.count(2, 0, 3) == (0, 0, 3)
    assert (m.gc_bases, m.acgt_bases) == (2 + 4, 2 + 8)
    assert FaModel(b"").contigs == [] and FaModel(b"").bases == 0 and FaModel(b">").contigs == [(b"", 0, 0, 0)]
    q = [(0, 0, 9), (0, 2, 5), (2, 1, 1)]
    assert m.count_many(q).tolist() == [list(m.count(*x)) for x in q]


# ---- the host helpers ------------------------------------------------------------------------------------------------

def test_symbols_declared_exported_and_listed(scfq):
    header = open(os.path.join(ROOT, "include", "sc_fqcount.h")).read()
    debug = open(os.path.join(ROOT, "include", "sc_fqcount_debug.h")).read()
    L = scfq.lib()
    for name in NEW:
        assert name + "(" in header and name in scfq.EXPORTS and hasattr(L, name), name
    assert "scfq_debug_fa_stages(" in debug and "scfq_debug_fa_stages" in scfq.EXPORTS and len(scfq.fa_stages()) == 4
    for name in ("fa_index_device", "fa_index_host", "fa_index_file", "fa_count_intervals", "fa_parse_window", "fa_gc_interval",
                 "format_fa_gc_value", "fa_gc", "FaSummary"):
        assert hasattr(scfq, name), name
    assert "312500000" in header and "255" in header          # the 5e5 note and the name limit


@pytest.mark.parametrize("text", ["1", "50", "3,200", "1e3", "5e5", "1,000,000", "2.5e2", "1e0"])
def test_parse_window(scfq, text):
    assert scfq.fa_parse_window(text) == parse_window(text)
    assert {"1": 1, "50": 50, "3,200": 3200, "1e3": 1000, "5e5": 312500000}.get(text, parse_window(text)) == scfq.fa_parse_window(text)


@pytest.mark.parametrize("text", ["0", "abc", "-3", "", "1e-2", "e", "1e", "e3", "1.5", "0e5"])
def test_parse_window_errors(scfq, text):
    with pytest.raises(ValueError):
        parse_window(text)
    w = ctypes.c_uint64(77)
    assert scfq.lib().scfq_fa_parse_window(text.encode(), ctypes.byref(w)) == scfq.SCFQ_EARG and w.value == 77
    detail = scfq.lib().scfq_fa_error_detail().decode()
    assert detail == "Window lengths must be >= 1" if text in ("0", "-3", "1e-2", "0e5") else "invalid window" in detail
    with pytest.raises(scfq.ScfqError) as e:
        scfq.fa_parse_window(text)
    assert e.value.rc == scfq.SCFQ_EARG
    assert scfq.lib().scfq_fa_parse_window(None, ctypes.byref(w)) == scfq.SCFQ_EARG
    assert scfq.lib().scfq_fa_parse_window(b"5", None) == scfq.SCFQ_EARG


def test_gc_interval(scfq):
    for length in (0, 1, 2, 1000):
        for pos in (-5, 0, 1, 2, length - 1, length, length + 1, length + 100):
            for w in (1, 2, 7, 999, 1000, 1001, 100000, 2 ** 63, 2 ** 64 - 1):
                assert scfq.fa_gc_interval(pos, w, length) == gc_interval(pos, w, length), (pos, w, length)
    assert scfq.fa_gc_interval(1, 1, 1000) == (0, 2) and scfq.fa_gc_interval(1000, 5, 1000) == (994, 1000)
    assert scfq.fa_gc_interval(0, 5, 1000) is None and scfq.fa_gc_interval(1001, 5, 1000) is None
    assert scfq.fa_gc_interval(10, 100000, 1000) == (0, 1000)
    L = scfq.lib()
    b, e, bad = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int()
    assert L.scfq_fa_gc_interval(1, 1, 10, None, ctypes.byref(e), ctypes.byref(bad)) == scfq.SCFQ_EARG
    assert L.scfq_fa_gc_interval(1, 1, 10, ctypes.byref(b), None, ctypes.byref(bad)) == scfq.SCFQ_EARG
    assert L.scfq_fa_gc_interval(1, 1, 10, ctypes.byref(b), ctypes.byref(e), None) == scfq.SCFQ_EARG


def test_value_text(scfq):
    f = scfq.format_fa_gc_value
    assert f(1, 2, 1) == "0.5" and f(5, 5, 1) == "1.0" and f(0, 7, 1) == "0.0" and f(0, 0, 50) == "nan" == value_text(0, 0, 50)
    assert f(495, 1000, 100000) == "0.495" and f(513, 1000, 100000) == "0.513"
    assert f(1, 20000, 100) == "5e-05" == value_text(1, 20000, 100)                       # below 1e-4: exponent form
    assert f(1, 10000, 10) == "0.0001" == value_text(1, 10000, 10)
    assert f(1, 3, 1) == "0.333" and f(2, 3, 1) == "0.667" and f(1, 3, 100000) == "0.33333333"
    # ties at the rounding digit (window 1: three digits): C round() on the product as the double holds it
    for gc, acgt in ((1, 2000), (3, 2000), (5, 2000), (1, 16), (3, 16), (5, 16), (7, 16), (9, 16), (1, 32), (125, 1000), (2675, 10000)):
        assert f(gc, acgt, 1) == value_text(gc, acgt, 1), (gc, acgt)
    assert value_text(1, 16, 1) == "0.063" and value_text(3, 16, 1) == "0.188" and c_round(2.5) == 3.0 and c_round(0.5) == 1.0
    rng = np.random.default_rng(5)
    for _ in range(3000):
        acgt = int(rng.integers(1, 3000))
        gc = int(rng.integers(0, acgt + 1))
        w = int(rng.choice([1, 9, 10, 50, 999, 3200, 100000, 312500000]))
        assert f(gc, acgt, w) == value_text(gc, acgt, w), (gc, acgt, w)
    L = scfq.lib()
    assert L.scfq_format_fa_gc_value(1, 2, 1, None, 0) == 3
    small = ctypes.create_string_buffer(3)
    assert L.scfq_format_fa_gc_value(495, 1000, 100000, small, 3) == 5 and small.value == b"0."
    assert L.scfq_format_fa_gc_value(1, 2, 1, None, 8) == scfq.SCFQ_EARG


# ---- positions -------------------------------------------------------------------------------------------------------

POS_TEXT = ("chrom\tpos\n"                  # line 1: a header, skipped silently
            "chr1\t5\n"
            "# a comment\n"
            "#chrX\tnot\n"
            "chr2:7\n"
            "bad line\n"                    # line 6: a warning
            " \t:chr3 : \t 9 extra fields\n"
            "\n"                            # line 8: a warning (no fields)
            "chr1 12\tx\r\n"
            "lonely\n"                      # line 10: a warning
            "chr2\t-4\n"
            "X::3")
POS_WANT = [("chr1", 5), ("chr2", 7), ("chr3", 9), ("chr1", 12), ("chr2", -4), ("X", 3)]


def pos_warnings(path):
    return ['Invalid line: 6 in "%s" > bad line' % path, 'Invalid line: 8 in "%s" > ' % path, 'Invalid line: 10 in "%s" > lonely' % path]


@pytest.mark.parametrize("gz", [False, True])
def test_position_files(scfq, tmp_path, gz):
    path = str(tmp_path / ("pos.tsv.gz" if gz else "pos.tsv"))
    with (gzip.open if gz else open)(path, "wb") as f:
        f.write(POS_TEXT.encode())
    assert parse_positions(path) == (POS_WANT, pos_warnings(path))
    err = io.StringIO()
    assert scfq.fa_positions(path, err) == POS_WANT
    assert err.getvalue() == "".join(warning_line(w) for w in pos_warnings(path))
    # the CLI reads the positions before it opens the FASTA: its warnings are there whatever becomes of the index
    r = run("fa-gc", "--pos", path, str(tmp_path / "missing.fa"), "5")
    assert r.stderr == err.getvalue() + red(2, "Unable to open file: " + str(tmp_path / "missing.fa")) and r.returncode == 2 and r.stdout == ""


def test_position_strings(scfq):
    for text, want in (("chr1:5", ("chr1", 5)), ("X:100", ("X", 100)), (":7", ("", 7)), ("a:-2", ("a", -2))):
        assert scfq.fa_positions(text) == [want] == parse_positions(text)[0]
    r = run("fa-gc", "--pos", "chr1:x", FASTA, "5")
    assert (r.returncode, r.stdout, r.stderr) == (1, "", red(1, "Invalid position: chr1:x"))
    r = run("fa-gc", "--pos", "calls.bcf", FASTA, "5")
    assert r.returncode == 1 and r.stdout == "" and "BCF" in r.stderr and "calls.bcf" in r.stderr
    r = run("fa-gc", "--pos", "no_such_positions.bed", FASTA, "5")
    assert (r.returncode, r.stdout, r.stderr) == (2, "", red(2, "Unable to open file: no_such_positions.bed"))


def test_order(scfq):
    mixed = [("chr2", 9), ("II", 1), ("chr10", 5), ("X", 7), ("1", 3), ("chrM", 2), ("I", 8), ("chr2", 4), ("x", 1), ("II", 1),
             ("chr1", 3), ("I", 2), ("CHR10", 1), ("chrY", 6), ("1", 1), ("chrM", 2), ("chr2", 9)]
    want = [("1", 1), ("1", 3), ("chr1", 3), ("chr2", 4), ("chr2", 9), ("chr2", 9), ("CHR10", 1), ("chr10", 5),
            ("x", 1), ("X", 7), ("chrY", 6), ("chrM", 2), ("chrM", 2),
            ("I", 8), ("I", 2), ("II", 1), ("II", 1)]
    assert order(mixed) == want
    assert sorted(mixed, key=lambda p: scfq.fa_sort_key(*p)) == want
    rng = np.random.default_rng(11)
    names = ["chr1", "1", "chr01", "2", "chr10", "chr9", "X", "chrx", "Y", "chrM", "m", "I", "II", "chrUn_1", "MT", "chr", "scaffold_7"]
    for _ in range(50):
        pts = [(names[int(rng.integers(len(names)))], int(rng.integers(1, 6))) for _ in range(40)]
        assert sorted(pts, key=lambda p: scfq.fa_sort_key(*p)) == order(pts)


# ---- CLI and ABI -----------------------------------------------------------------------------------------------------

def test_cli_usage_without_a_device():
    r = run("fa-gc", "--help")
    assert r.returncode == 0 and "fa-gc [options] fasta [windows ...]" in r.stdout and "--pos" in r.stdout
    assert run("fa-gc").stdout == r.stdout
    top = run("--help").stdout
    assert "fa-gc" in top and top.index("fq-kmers") < top.index("fa-gc")
    r = run("fa-gc", FASTA, "100")
    assert (r.returncode, r.stdout, r.stderr) == (1, "", red(1, "Must provide --pos: (chr:100 / bed / vcf )"))
    for pos in (("--pos", "chr1:10"), ("--pos=chr1:10",), ("-p", "chr1:10")):
        r = run("fa-gc", *pos, FASTA)
        assert (r.returncode, r.stdout, r.stderr) == (1, "", red(1, "Must provide a list of windows: (e.g. 100 200 500)")), pos
        r = run("fa-gc", *pos, FASTA, "100", "0")
        assert (r.returncode, r.stdout, r.stderr) == (1, "", red(1, "Window lengths must be >= 1")), pos
    r = run("fa-gc", "--pos", "chr1:10", FASTA, "abc")
    assert r.returncode == 1 and r.stdout == "" and "abc" in r.stderr
    r = run("fa-gc", "--pos", "chr1:10", "does_not_exist.fa", "100")
    assert (r.returncode, r.stdout, r.stderr) == (2, "", red(2, "Unable to open file: does_not_exist.fa"))
    r = run("fa-gc", "--bogus", FASTA, "100")
    assert r.returncode == 1 and "Unknown option" in r.stderr


def test_struct_layout(scfq):
    S = scfq.FaSummary
    assert tuple(f[0] for f in S._fields_) == SUMMARY_FIELDS
    for k, name in enumerate(SUMMARY_FIELDS):
        assert getattr(S, name).offset == 8 * k and getattr(S, name).size == 8, name
    assert ctypes.sizeof(S) == 72 and ctypes.sizeof(scfq.FaInterval) == 24 and ctypes.sizeof(scfq.FaCounts) == 24
    assert ctypes.sizeof(scfq.FaContig) == 32 and scfq.FaContig.length.offset == 24


def test_header_is_c99_and_sizes_agree(tmp_path):
    src = tmp_path / "t.c"
    offsets = " && ".join("offsetof(scfq_fa_summary, %s) == %d" % (name, 8 * k) for k, name in enumerate(SUMMARY_FIELDS))
    src.write_text('#include <stddef.h>\n#include "sc_fqcount.h"\n#include "sc_fqcount_debug.h"\n'
                   "typedef char sizes[sizeof(scfq_fa_summary) == 72 && sizeof(scfq_fa_interval) == 24 && sizeof(scfq_fa_counts) == 24"
                   " && sizeof(scfq_fa_contig) == 32 ? 1 : -1];\n"
                   "typedef char at[" + offsets + " ? 1 : -1];\n"
                   "int main(void){ scfq_fa_summary s; scfq_fa_index* ix = 0; scfq_fa_contig c; scfq_fa_interval q = {0, 0, 1};\n"
                   "  scfq_fa_counts out; uint64_t i, b, e; int bad; double ms[4]; char buf[32]; s.struct_size = sizeof s;\n"
                   "  scfq_fa_index_free(ix);\n"
                   "  return scfq_fa_index_buffer(\"\", 0, 0, &ix, &s) + scfq_fa_index_file(\"x\", 0, &ix, &s) + scfq_fa_contig_at(ix, 0, &c)\n"
                   "         + scfq_fa_contig_find(ix, \"a\", &i) + scfq_fa_count_intervals(ix, &q, 1, &out) + scfq_fa_parse_window(\"5\", &i)\n"
                   "         + scfq_fa_gc_interval(1, 1, 1, &b, &e, &bad) + scfq_format_fa_gc_value(1, 2, 3, buf, 32)\n"
                   "         + scfq_debug_fa_stages(ms, 4) + (scfq_fa_error_detail() != 0) == 12345; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-fsyntax-only", str(src)])


def test_argument_checks(scfq):
    L = scfq.lib()
    buf = ctypes.create_string_buffer(SMALL)
    h = ctypes.c_void_p(1234)
    s = scfq.FaSummary()
    s.struct_size = ctypes.sizeof(scfq.FaSummary)
    assert L.scfq_fa_index_buffer(buf, len(SMALL), 0, None, ctypes.byref(s)) == scfq.SCFQ_EARG                 # NULL out
    bad = scfq.FaSummary()                                                                                    # struct_size not set
    assert L.scfq_fa_index_buffer(buf, len(SMALL), 0, ctypes.byref(h), ctypes.byref(bad)) == scfq.SCFQ_EARG and h.value == 1234
    bad.struct_size = ctypes.sizeof(scfq.FaSummary) + 8
    assert L.scfq_fa_index_buffer(buf, len(SMALL), 0, ctypes.byref(h), ctypes.byref(bad)) == scfq.SCFQ_EARG
    assert L.scfq_fa_index_file(b"x.fa", None, ctypes.byref(h), ctypes.byref(bad)) == scfq.SCFQ_EARG
    assert L.scfq_fa_index_buffer(None, 5, 0, ctypes.byref(h), ctypes.byref(s)) == scfq.SCFQ_EARG             # NULL pointer with n > 0
    assert L.scfq_fa_index_file(None, None, ctypes.byref(h), ctypes.byref(s)) == scfq.SCFQ_EARG
    assert L.scfq_fa_index_file(b"x.fa", None, None, ctypes.byref(s)) == scfq.SCFQ_EARG
    c, i = scfq.FaContig(), ctypes.c_uint64()
    q, out = scfq.FaInterval(0, 0, 1), scfq.FaCounts()
    assert L.scfq_fa_contig_at(None, 0, ctypes.byref(c)) == scfq.SCFQ_EARG
    assert L.scfq_fa_contig_find(None, b"a", ctypes.byref(i)) == scfq.SCFQ_EARG
    assert L.scfq_fa_count_intervals(None, ctypes.byref(q), 1, ctypes.byref(out)) == scfq.SCFQ_EARG
    assert L.scfq_fa_count_intervals(None, None, 0, None) == scfq.SCFQ_EARG
    L.scfq_fa_index_free(None)
    assert L.scfq_fa_index_file(os.path.join(GOLDEN, "fasta", "does_not_exist.fa").encode(), None, ctypes.byref(h), ctypes.byref(s)) \
        == scfq.SCFQ_EOPEN and h.value is None


def test_no_gpu_means_loud_failure(scfq):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    for call in (lambda: scfq.fa_index_host(SMALL), lambda: scfq.fa_index_host(b""), lambda: scfq.fa_index_file(FASTA),
                 lambda: scfq.fa_gc(FASTA, "chr1:10", ["100"])):
        with pytest.raises(scfq.ScfqError) as e:
            call()
        assert e.value.rc == scfq.SCFQ_EHIP
    r = run("fa-gc", "--pos", "chr1:10", FASTA, "100")
    assert r.returncode == 1 and r.stdout == "" and r.stderr.startswith("\x1b[31mError 1: ")

"""fq-normalize without a device: the fixture against its generator, the laws of the checker (_normalize_check.py) and hand-worked
cases, the ABI (symbols, struct layout, C99 header), every argument check (all come before the first HIP call), the formatters and
the grammar of `sc fq-normalize`."""
import ctypes
import gzip
import importlib.util
import os
import subprocess

import pytest

from conftest import GOLDEN, PKG, ROOT
from _kcount_check import kcount_of
from _kmers_check import index_of
from _normalize_check import (EARG, EHIP, FIELDS, GOLDEN as GOLDEN_RATIO, HIGH, HIST_HEADER, KEPT, LOW, MAX_DEPTH, NO_KMERS, ROW_FIELDS, ROW_HEADER,
                              STATS_WORDS, classify, counts_of, hist_rows, mix64, normalize_of, record_of, report_row)

SC = os.path.join(PKG, "sc")
NORM = os.path.join(GOLDEN, "normalize")
NEW = ("scfq_norm_buffers", "scfq_norm_files", "scfq_format_norm_row_tsv", "scfq_format_norm_hist_tsv", "scfq_norm_error_detail")
FASTQ = b"@h\nACGTACGTACGTACGTACGTACGTN\n+\nIIIIIIIIIIIIIIIIIIIIIIIII\n"


def run(*args):
    return subprocess.run([SC] + list(args), capture_output=True, text=True, stdin=subprocess.DEVNULL)


def fq(*seqs):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(seqs))


def load_generator():
    spec = importlib.util.spec_from_file_location("make_normalize", os.path.join(NORM, "make_normalize.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ---- the fixture ------------------------------------------------------------------------------------------------------------
def test_fixture_is_what_its_generator_writes():
    m = load_generator()
    files, w = m.make_files()
    assert sorted(files) == sorted(n for n in os.listdir(NORM) if not n.endswith(".py") and n != "__pycache__")
    for name, data in files.items():
        have = open(os.path.join(NORM, name), "rb").read()
        if name.endswith(".gz"):       # (the compressed bytes are zlib's business)
            have, data = gzip.decompress(have), gzip.decompress(data)
        assert have == data, name
        assert len(have) < 1 << 20
    assert (m.K, m.TARGET, m.MIN_DEPTH) == (21, 20, 3)
    assert {NO_KMERS, LOW, HIGH, KEPT} <= set(w["classes"])
    assert w["units_in"] == 184 and w["dropped_no_kmers"] == 1 and w["dropped_low"] > 0 and w["dropped_high"] > 0
    # the interleaved form and the gzip form hold the same pairs
    assert files["out1.fq"].count(b"\n") == files["out2.fq"].count(b"\n") == 4 * w["units_out"]


# ---- the checker ------------------------------------------------------------------------------------------------------------
def test_checker_literal_cases():
    # MurmurHash3's finalizer: fixed points and a value worked out by hand from its three steps
    assert mix64(0) == 0
    x = 1
    x ^= x >> 33
    x = x * 0xFF51AFD7ED558CCD % 2 ** 64
    x ^= x >> 33
    x = x * 0xC4CEB9FE1A85EC53 % 2 ** 64
    x ^= x >> 33
    assert mix64(1) == x == 0xB456BCFC34C2CB2C
    # the lower median
    assert record_of([]) == (0, 0, 0, 0)
    assert record_of([5]) == (1, 5, 5, 0)
    assert record_of([1, 9]) == (2, 1, 1, 1)
    assert record_of([9, 1, 5]) == (3, 5, 1, 1)
    assert record_of([9, 1, 5, 7]) == (4, 5, 1, 1)
    assert record_of([0, 0, 3, 1], weak_below=0) == (4, 0, 0, 0) and record_of([0, 0, 3, 1], weak_below=3) == (4, 0, 0, 3)
    # counts in window order, skipped windows left out, saturation
    ix = index_of
    table = {ix(b"ACGTACGTACGTA"): 7, ix(b"CGTACGTACGTAC"): 2 ** 40}
    assert counts_of(b"ACGTACGTACGTACG", table, 13, False) == [7, MAX_DEPTH, 0]
    assert counts_of(b"ACGTACGTACGTACG", table, 13, True) == [7, MAX_DEPTH, MAX_DEPTH]      # GTACGTACGTACG is the reverse complement
    assert counts_of(b"ACGTACGTACGTNCG", table, 13, False) == [] and counts_of(b"ACGTACGTACGT", table, 13, False) == []
    assert counts_of(b"NACGTACGTACGTAc", table, 13, False) == [7]
    assert counts_of(b"T" * 33, {2 ** 64 - 1: 5}, 32, False) == [5, 5] and counts_of(b"T" * 33, {0: 4}, 32, True) == [4, 4]
    # the rule
    assert classify([(0, 0)], 0) == (NO_KMERS, 0) and classify([(0, 0), (0, 0)], 5, 20, 3) == (NO_KMERS, 0)
    assert classify([(5, 9), (0, 0)], 0) == (KEPT, 9) and classify([(0, 0), (5, 9)], 0) == (KEPT, 9)
    assert classify([(5, 9), (5, 4)], 0) == (KEPT, 4) and classify([(5, 9), (5, 4)], 0, min_depth=5) == (LOW, 4)
    assert classify([(5, 4)], 0, min_depth=4) == (KEPT, 4)
    assert classify([(5, 20)], 0, target=20) == (KEPT, 20) and classify([(5, 0)], 0, target=20) == (KEPT, 0)
    r = [mix64(u * GOLDEN_RATIO % 2 ** 64) >> 32 for u in range(64)]
    assert [classify([(5, 21)], u, target=20)[0] for u in range(64)] == [HIGH if x * 21 >> 32 >= 20 else KEPT for x in r]
    assert any(classify([(5, 10 ** 6)], u, target=1)[0] == HIGH for u in range(4))
    # low comes before high
    assert classify([(5, 2)], 0, target=1, min_depth=3) == (LOW, 2)


def test_checker_on_a_small_input():
    a = b"ACGTTGCATGCCGATAGCTAGG"            # 22 bases: ten windows at k = 13
    data = fq(a, a, a[:14], b"ACGT", a[::-1])
    table = kcount_of(data, 13, False).table
    w = normalize_of(table, 13, False, data, bins=4)
    assert w["recs"][:4] == [(10, 2, 2, 0), (10, 2, 2, 0), (2, 3, 3, 0), (0, 0, 0, 0)] and w["recs"][4] == (10, 1, 1, 10)
    assert w["classes"] == [KEPT, KEPT, KEPT, NO_KMERS, KEPT] and w["hist"] == [[0, 0], [1, 1], [2, 2], [1, 1]]
    assert (w["units_in"], w["units_out"], w["dropped_no_kmers"], w["short_reads"], w["windows"], w["kmers"], w["weak_kmers"]) == (5, 4, 1, 1, 32, 32, 10)
    assert w["out1"] == fq(a, a, a[:14]) + b"@r4\n%s\n+\n%s\n" % (a[::-1], b"I" * 22) and w["out2"] == b""
    keep = normalize_of(table, 13, False, data, keep_no_kmers=True, bins=4)
    assert keep["units_out"] == 5 and keep["dropped_no_kmers"] == 0 and keep["hist"] == w["hist"] and keep["out1"] == data
    # pairs: the lower mate decides, interleaved sends both to out1
    two = normalize_of(table, 13, False, fq(a, a[:14]), fq(a[::-1], b"ACGT"), min_depth=2)
    assert two["classes"] == [LOW, KEPT] and two["out1"] == b"@r1\n%s\n+\n%s\n" % (a[:14], b"I" * 14) and two["out2"] == b"@r1\nACGT\n+\nIIII\n"
    inter = normalize_of(table, 13, False, fq(a, a[::-1], a[:14], b"ACGT"), interleaved=True, min_depth=2)
    assert inter["classes"] == [LOW, KEPT] and inter["out1"] == b"@r2\n%s\n+\n%s\n@r3\nACGT\n+\nIIII\n" % (a[:14], b"I" * 14)
    assert report_row(w).split("\t") == [str(w[f]) for f in ROW_FIELDS] and hist_rows([[1, 0], [5, 2]]) == ["0\t1\t0", "1\t5\t2"]


def test_checker_laws():
    m = load_generator()
    files, _ = m.make_files()
    r1, r2 = files["r1.fq"], files["r2.fq"]
    table = kcount_of([r1, r2], 21, True).table
    # target = 0 and min_depth = 0 keep everything but no_kmers
    w = normalize_of(table, 21, True, r1, r2)
    assert all(c in (KEPT, NO_KMERS) for c in w["classes"]) and w["units_out"] == w["units_in"] - w["dropped_no_kmers"]
    assert w["dropped_low"] == w["dropped_high"] == 0 and w["dropped_no_kmers"] == 1
    # raising the target never drops a unit that was kept, at a fixed seed
    for seed in (0, 12345):
        before = None
        for target in (1, 2, 5, 10, 15, 20, 25, 30, 40, 80):
            kept = {u for u, c in enumerate(normalize_of(table, 21, True, r1, r2, target=target, seed=seed)["classes"]) if c == KEPT}
            assert before is None or before <= kept, (seed, target)
            before = kept
    # the kept share at D = 40, target = 20: 0.5 +- six binomial standard deviations of 0.0016
    kept = sum(classify([(1, 40)], u, target=20)[0] == KEPT for u in range(100000))
    assert abs(kept / 100000 - 0.5) <= 0.01, kept


# ---- the ABI ----------------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_listed(scfq):
    header = open(os.path.join(ROOT, "include", "sc_fqcount.h")).read()
    debug = open(os.path.join(ROOT, "include", "sc_fqcount_debug.h")).read()
    L = scfq.lib()
    for name in NEW:
        assert name + "(" in header and name in scfq.EXPORTS and hasattr(L, name), name
    assert "scfq_debug_norm_stages(" in debug and "scfq_debug_norm_stages" in scfq.EXPORTS and len(scfq.norm_stages()) == 4
    assert (scfq.SCFQ_NORM_MAX_DEPTH, scfq.SCFQ_NORM_INTERLEAVED, scfq.SCFQ_NORM_KEEP_NO_KMERS, scfq.NORM_MAX_BINS) == (MAX_DEPTH, 1, 2, 1 << 20)
    for name in ("NormOpts", "NormRec", "NormStats", "norm_opts", "norm_device", "norm_host", "norm_file", "format_norm_row_tsv", "format_norm_hist_tsv"):
        assert hasattr(scfq, name), name
    for text in ("32 bytes per input byte", "SCFQ_NORM_LDS_WINDOWS", "sorted[(kmers - 1) / 2]", "0x9E3779B97F4A7C15"):
        assert text in header, text


def test_struct_layout(scfq):
    S = scfq.NormStats
    names = tuple(f[0] for f in S._fields_)
    assert names == scfq.NORM_STATS_FIELDS and len(names) == STATS_WORDS and set(FIELDS) < set(names)
    for i, name in enumerate(names):
        assert getattr(S, name).offset == 8 * i and getattr(S, name).size == 8, name
    assert ctypes.sizeof(S) == 8 * STATS_WORDS and ctypes.sizeof(scfq.NormOpts) == 48 and ctypes.sizeof(scfq.NormRec) == 16
    O = scfq.NormOpts
    want = [("struct_size", 0, 8), ("flags", 8, 4), ("k", 12, 4), ("table_flags", 16, 4), ("table_bits", 20, 4), ("target", 24, 4), ("min_depth", 28, 4),
            ("weak_below", 32, 4), ("reserved", 36, 4), ("seed", 40, 8)]
    assert [(n, getattr(O, n).offset, getattr(O, n).size) for n, _, _ in want] == want


def test_header_is_c99_and_sizes_agree(tmp_path, scfq):
    src = tmp_path / "t.c"
    offsets = " && ".join("offsetof(scfq_norm_stats, %s) == %d" % (name, 8 * i) for i, name in enumerate(scfq.NORM_STATS_FIELDS))
    src.write_text('#include <stddef.h>\n#include "sc_fqcount.h"\n#include "sc_fqcount_debug.h"\n'
                   "typedef char sizes[sizeof(scfq_norm_stats) == 296 && sizeof(scfq_norm_opts) == 48 && sizeof(scfq_norm_rec) == 16 ? 1 : -1];\n"
                   "typedef char at[" + offsets + " ? 1 : -1];\n"
                   "typedef char consts[SCFQ_NORM_MAX_DEPTH == 4294967294u && SCFQ_NORM_INTERLEAVED == 1 && SCFQ_NORM_KEEP_NO_KMERS == 2\n"
                   "                    && SCFQ_NORM_MAX_BINS == 1048576 && offsetof(scfq_norm_opts, seed) == 40 ? 1 : -1];\n"
                   "int main(void){ scfq_norm_stats s; scfq_norm_opts o; scfq_norm_rec r; scfq_kcount* t = 0; uint64_t h[4]; double ms[4]; char b[8];\n"
                   "  s.struct_size = sizeof s; o.struct_size = sizeof o;\n"
                   "  return scfq_norm_buffers(t, 0, 0, 0, 0, 0, &o, &r, 1, 0, 0, 0, 0, 0, h, 2, &s)\n"
                   "         + scfq_norm_files(t, \"x\", 0, 0, &o, -1, -1, &r, 1, h, 2, &s) + scfq_format_norm_row_tsv(&s, 0, b, 8)\n"
                   "         + scfq_format_norm_hist_tsv(1, 2, 3, b, 8) + scfq_debug_norm_stages(ms, 4) + (scfq_norm_error_detail() != 0) == 12345; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-fsyntax-only", str(src)])


def test_argument_checks(scfq):
    """every SCFQ_EARG of the contract, each with its text; none of them needs a device (without one, a call that got past the checks
    returns SCFQ_EHIP, and a fake table handle would be dereferenced)"""
    L = scfq.lib()
    buf = ctypes.create_string_buffer(FASTQ)
    n = len(FASTQ)
    detail = L.scfq_norm_error_detail
    fake = ctypes.c_void_p(0)        # (no table: the two-pass form, whose own options are checked as well)

    def stats(size=None):
        s = scfq.NormStats()
        s.struct_size = ctypes.sizeof(scfq.NormStats) if size is None else size
        return s

    def buffers(opts, s=None, r1=buf, n1=n, r2=None, n2=0, out2=None, cap2=0, hist=None, bins=0):
        s = stats() if s is None else s
        return L.scfq_norm_buffers(fake, r1, n1, r2, n2, 0, ctypes.byref(opts) if opts is not None else None, None, 0, None, 0, out2, cap2, 0, hist, bins,
                                   ctypes.byref(s) if s is not False else None)

    def files(opts, s=None, p1=b"x.fq", p2=None, fd2=-1, hist=None, bins=0):
        s = stats() if s is None else s
        return L.scfq_norm_files(fake, p1, p2, None, ctypes.byref(opts) if opts is not None else None, -1, fd2, None, 0, hist, bins, ctypes.byref(s))

    ok = dict(k=21, canonical=True)
    h = (ctypes.c_uint64 * 8)()
    out = ctypes.create_string_buffer(16)
    for call in (buffers, files):
        for flags, text in ((4, b"0x4"), (0x80000001, b"0x80000000"), (0xfffffffc, b"0xfffffffc")):
            assert call(scfq.norm_opts(flags=flags, **ok)) == EARG and b"flag" in detail() and text in detail()
        assert call(scfq.norm_opts(reserved=1, **ok)) == EARG and b"reserved" in detail()
        bad = scfq.norm_opts(**ok)
        bad.struct_size -= 8
        assert call(bad) == EARG and b"opts->struct_size" in detail()
        for size in (0, 288, 304):
            assert call(scfq.norm_opts(**ok), stats(size)) == EARG and b"stats->struct_size" in detail()
        for bins in (0, 1, (1 << 20) + 1, 1 << 40):
            assert call(scfq.norm_opts(**ok), hist=h, bins=bins) == EARG and (b"bins = %d" % bins) in detail()
        assert call(scfq.norm_opts(**ok), hist=None, bins=4) == EARG and b"bins = 4" in detail()
        # the two-pass form: k, table_flags and table_bits are fq-kcount's
        for k in (0, 12, 33):
            assert call(scfq.norm_opts(k=k)) == EARG and (b"k = %d" % k) in detail() and b"counted first" in detail()
        assert call(None) == EARG and b"k = 0" in detail()                          # the defaults need a table
        assert call(scfq.norm_opts(k=21, table_flags=2)) == EARG and b"0x2" in detail()
        assert call(scfq.norm_opts(k=21, table_bits=9)) == EARG and b"table_bits = 9" in detail()
    assert buffers(scfq.norm_opts(**ok), False) == EARG and b"stats" in detail()
    # the input forms
    assert buffers(scfq.norm_opts(**ok), r1=None, n1=0, r2=buf, n2=n) == EARG and b"second input without a first" in detail()
    assert buffers(scfq.norm_opts(interleaved=True, **ok), r2=buf, n2=n) == EARG and b"interleaved" in detail()
    assert buffers(scfq.norm_opts(interleaved=True, **ok), out2=out, cap2=16) == EARG and b"out2" in detail()
    assert buffers(scfq.norm_opts(**ok), out2=out, cap2=16) == EARG and b"out2" in detail()
    assert buffers(scfq.norm_opts(**ok), r1=None) == EARG and b"NULL" in detail()
    assert files(scfq.norm_opts(**ok), p1=None) == EARG and b"path1" in detail()
    assert files(scfq.norm_opts(**ok), p1=None, p2=b"y.fq") == EARG and b"second input without a first" in detail()
    assert files(scfq.norm_opts(interleaved=True, **ok), p2=b"y.fq") == EARG and b"interleaved" in detail()
    assert files(scfq.norm_opts(**ok), fd2=5) == EARG and b"out2" in detail()
    with pytest.raises(scfq.ScfqError) as e:
        scfq.norm_host(None, FASTQ, opts=scfq.norm_opts(k=12))
    assert e.value.rc == EARG and "k = 12" in str(e.value)


def test_no_gpu_means_loud_failure(scfq):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(scfq.ScfqError) as e:
        scfq.norm_host(None, FASTQ, opts=scfq.norm_opts(k=13, canonical=True, target=5))
    assert e.value.rc == EHIP
    with pytest.raises(scfq.ScfqError) as e:
        scfq.norm_file(None, os.path.join(NORM, "r1.fq"), os.path.join(NORM, "r2.fq"), opts=scfq.norm_opts(k=21))
    assert e.value.rc == EHIP
    with pytest.raises(scfq.ScfqError) as e:
        scfq.norm_file(None, os.path.join(NORM, "does_not_exist.fq"), opts=scfq.norm_opts(k=21))
    assert e.value.rc == scfq.SCFQ_EOPEN


def test_formatters(scfq):
    assert scfq.format_norm_row_tsv(None, header=True) == ROW_HEADER
    s = scfq.NormStats()
    s.struct_size = ctypes.sizeof(s)
    for i, name in enumerate(ROW_FIELDS):
        setattr(s, name, 1000 + i)
    s.seed = 2 ** 64 - 1
    assert scfq.format_norm_row_tsv(s) == "\t".join(str(1000 + i) for i in range(len(ROW_FIELDS)))
    s.units_in = 2 ** 64 - 1
    assert scfq.format_norm_row_tsv(s).startswith("18446744073709551615\t1001\t")
    assert scfq.format_norm_hist_tsv(0, 5, 3) == "0\t5\t3" == hist_rows([[5, 3]])[0]
    assert scfq.format_norm_hist_tsv(1001, 2 ** 64 - 1, 0) == "1001\t18446744073709551615\t0"
    L = scfq.lib()
    assert L.scfq_format_norm_hist_tsv(12, 34, 56, None, 0) == 8
    small = ctypes.create_string_buffer(b"#" * 8, 8)
    assert L.scfq_format_norm_hist_tsv(12, 34, 56, small, 5) == 8 and small.raw == b"12\t3\0###"
    s.struct_size = 8
    assert L.scfq_format_norm_row_tsv(ctypes.byref(s), 0, None, 0) == EARG and L.scfq_format_norm_row_tsv(None, 0, None, 0) == EARG


# ---- the command ------------------------------------------------------------------------------------------------------------
def test_cli_without_a_device():
    r = run("fq-normalize", "--help")
    assert r.returncode == 0 and r.stderr == "" and "fq-normalize [options] IN.fq > out.fq" in r.stdout
    assert "fq-normalize [options] --out1=PATH --out2=PATH R1.fq R2.fq" in r.stdout and "fq-normalize [options] --interleaved [--out=PATH] IN.fq" in r.stdout
    for opt in ("--k=N", "--plain", "--target=N", "--min-depth=N", "--weak-below=N", "--seed=N", "--keep-no-kmers", "--table-bits=N", "--stats",
                "--hist[=BINS]", "--per-read=PATH", "--out=PATH", "--out1=PATH", "--out2=PATH", "--interleaved", "-t, --header", "-b, --basename",
                "-a, --absolute"):
        assert opt in r.stdout, opt
    assert run("fq-normalize").stdout == r.stdout and run("fq-normalize", "-h").stdout == r.stdout
    assert "fq-normalize" not in run("--help").stdout                                        # listed in its own help only
    r = run("fq-normalize", "does_not_exist.fq")
    assert (r.returncode, r.stderr, r.stdout) == (2, "\x1b[31mError 2: Unable to open file: does_not_exist.fq\x1b[0m\n", "")
    r = run("fq-normalize", "-b")
    assert (r.returncode, r.stderr) == (3, "\x1b[31mError 3: No FASTQ specified\x1b[0m\n")
    r1, r2 = os.path.join(NORM, "r1.fq"), os.path.join(NORM, "r2.fq")
    usage = ["--k=12", "--k=33", "--k=x", "--k=", "--k", "--target=-1", "--target=4294967295", "--target=", "--min-depth=x", "--weak-below=4294967295",
             "--seed=-1", "--seed=18446744073709551616", "--table-bits=9", "--table-bits=33", "--hist=1", "--hist=1048577", "--hist=", "--hist=x",
             "--bogus", "--plain=1", "--stats=1", "--out=", "--per-read="]
    forms = [(r1, r2, "--out=x.fq"), (r1, r2, "--out1=x.fq"), (r1, r2, "--out2=x.fq"), (r1, "--out1=x.fq", "--out2=y.fq"), (r1, r2, "--interleaved"),
             (r1, r2, r1)]
    for bad in [(u, r1) for u in usage] + forms:
        r = run("fq-normalize", *bad)
        assert r.returncode == 1 and "Error" in r.stderr and "Usage:" in r.stdout, bad
    assert not os.path.exists("x.fq") and not os.path.exists("y.fq")

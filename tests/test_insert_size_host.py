"""fq-insert-size without a device: the ABI (symbols, struct layout, C99 header), argument checks, the row formatter, the CLI's header /
help / error behaviour, the two checkers of _insert_size_check.py against each other, and literal cases of the contract."""
import ctypes
import glob
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG, ROOT
from _insert_size_check import (DEFAULTS, FIELDS, HIST_BINS, fastq, insert_of, insert_of_np, interleave, nimf, pair_of, planted, random_dna,
                                revcomp, same, summary_text, cli_text)
from test_gpu_parity import random_fastq_like

SC = os.path.join(PKG, "sc")
PAIRS = os.path.join(GOLDEN, "pairs")
HEADER = "pairs\toverlapped\tpercent_overlapped\tmin\tmedian\tmean\tstd_dev\tmode\tmax\tread_through\tmismatch_rate"
DIST_HEADER = "insert_size\tcount"
NEW = ("scfq_insert_size_buffers", "scfq_insert_size_files", "scfq_format_insert_size_tsv", "scfq_insert_size_error_detail")
SUMMARY = ("struct_size", "abi_version") + FIELDS
FASTQ = b"@h\nACGTN\n+\nIIIII\n"
PARAM_SETS = (DEFAULTS, (1, 65535, 100), (3, 1, 50), (8, 0, 0))


def run(*args):
    return subprocess.run([SC] + list(args), capture_output=True, text=True, stdin=subprocess.DEVNULL)


def test_symbols_declared_exported_and_listed(scfq):
    header = open(os.path.join(ROOT, "include", "sc_fqcount.h")).read()
    debug = open(os.path.join(ROOT, "include", "sc_fqcount_debug.h")).read()
    L = scfq.lib()
    for name in NEW:
        assert name + "(" in header and name in scfq.EXPORTS and hasattr(L, name), name
    assert "scfq_debug_insert_size_stages(" in debug and "scfq_debug_insert_size_stages" in scfq.EXPORTS and hasattr(L, "scfq_debug_insert_size_stages")
    assert len(scfq.insert_size_stages()) == 4
    assert (scfq.INSERT_MAX_LEN, scfq.INSERT_HIST_BINS, scfq.SCFQ_INSERT_INTERLEAVED) == (512, 1024, 1)
    for name in ("SCFQ_INSERT_MAX_LEN", "SCFQ_INSERT_HIST_BINS", "SCFQ_INSERT_INTERLEAVED"):
        assert name in header, name
    for name in ("OverlapRec", "InsertSummary", "InsertOpts", "insert_size_device", "insert_size_host", "insert_size_file", "format_insert_size_tsv",
                 "insert_size_stages"):
        assert hasattr(scfq, name), name


def test_struct_layout(scfq):
    R, O, S = scfq.OverlapRec, scfq.InsertOpts, scfq.InsertSummary
    assert ctypes.sizeof(R) == 8 and (R.offset.offset, R.overlap.offset, R.mismatches.offset) == (0, 4, 6)
    assert ctypes.sizeof(O) == 24 and (O.struct_size.offset, O.flags.offset, O.min_overlap.offset, O.max_mismatches.offset, O.max_mismatch_pct.offset) == (0, 8, 12, 16, 20)
    assert tuple(f[0] for f in S._fields_) == SUMMARY and len(SUMMARY) == 25
    for k, name in enumerate(SUMMARY):
        assert getattr(S, name).offset == 8 * k and getattr(S, name).size == 8, name
    assert ctypes.sizeof(S) == 8 * 25


def test_header_is_c99_and_sizes_agree(tmp_path):
    src = tmp_path / "t.c"
    offsets = " && ".join("offsetof(scfq_insert_summary, %s) == %d" % (name, 8 * k) for k, name in enumerate(SUMMARY))
    offsets += " && offsetof(scfq_overlap_rec, offset) == 0 && offsetof(scfq_overlap_rec, overlap) == 4 && offsetof(scfq_overlap_rec, mismatches) == 6"
    offsets += " && offsetof(scfq_insert_opts, flags) == 8 && offsetof(scfq_insert_opts, max_mismatch_pct) == 20"
    src.write_text('#include <stddef.h>\n#include "sc_fqcount.h"\n#include "sc_fqcount_debug.h"\n'
                   "typedef char sum_size[sizeof(scfq_insert_summary) == 8 * 25 ? 1 : -1];\n"
                   "typedef char rec_size[sizeof(scfq_overlap_rec) == 8 ? 1 : -1];\n"
                   "typedef char opt_size[sizeof(scfq_insert_opts) == 24 ? 1 : -1];\n"
                   "typedef char at[" + offsets + " ? 1 : -1];\n"
                   "typedef char consts[SCFQ_INSERT_MAX_LEN == 512 && SCFQ_INSERT_HIST_BINS == 1024 && SCFQ_INSERT_INTERLEAVED == 1 ? 1 : -1];\n"
                   "int main(void){ scfq_insert_summary s; scfq_insert_opts o; scfq_overlap_rec r[2]; double ms[4]; uint64_t h[SCFQ_INSERT_HIST_BINS];\n"
                   "  s.struct_size = sizeof s; o.struct_size = sizeof o; o.flags = 0; o.min_overlap = 30; o.max_mismatches = 5; o.max_mismatch_pct = 20;\n"
                   "  return scfq_insert_size_buffers(0, 0, 0, 0, 0, &o, r, 2, h, &s) + scfq_format_insert_size_tsv(&s, 0, 0)\n"
                   "         + scfq_insert_size_files(\"x\", \"y\", 0, &o, 0, 0, h, &s) + scfq_debug_insert_size_stages(ms, 4)\n"
                   "         + (scfq_insert_size_error_detail() != 0) == 12345; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-fsyntax-only", str(src)])


def test_argument_checks(scfq):
    L = scfq.lib()
    s = scfq._new_insert_summary()
    buf = ctypes.create_string_buffer(FASTQ)
    n = len(FASTQ)
    recs = (scfq.OverlapRec * 4)()
    hist = (ctypes.c_uint64 * HIST_BINS)()
    ok = ctypes.byref(s)
    detail = L.scfq_insert_size_error_detail
    B, F = L.scfq_insert_size_buffers, L.scfq_insert_size_files
    # without text
    assert B(buf, n, buf, n, 0, None, None, 0, hist, None) == scfq.SCFQ_EARG                          # NULL summary
    bad = scfq.InsertSummary()                                                                       # struct_size not set
    assert B(buf, n, buf, n, 0, None, None, 0, hist, ctypes.byref(bad)) == scfq.SCFQ_EARG
    bad.struct_size = ctypes.sizeof(scfq.InsertSummary) - 8
    assert B(buf, n, buf, n, 0, None, None, 0, hist, ctypes.byref(bad)) == scfq.SCFQ_EARG
    assert B(None, n, buf, n, 0, None, None, 0, hist, ok) == scfq.SCFQ_EARG                           # NULL pointer with n > 0
    assert B(buf, n, None, n, 0, None, None, 0, hist, ok) == scfq.SCFQ_EARG
    assert B(buf, n, buf, n, 0, None, None, 4, hist, ok) == scfq.SCFQ_EARG                            # NULL table with rec_cap > 0
    small = scfq.insert_opts()
    small.struct_size -= 4
    assert B(buf, n, buf, n, 0, ctypes.byref(small), None, 0, hist, ok) == scfq.SCFQ_EARG             # wrong size of the options
    assert F(None, b"y.fq", None, None, None, 0, hist, ok) == scfq.SCFQ_EARG
    assert F(b"x.fq", b"y.fq", None, None, None, 0, hist, ctypes.byref(bad)) == scfq.SCFQ_EARG
    assert F(b"x.fq", b"y.fq", None, None, None, 4, hist, ok) == scfq.SCFQ_EARG
    assert F(b"x.fq", b"y.fq", None, ctypes.byref(small), None, 0, hist, ok) == scfq.SCFQ_EARG
    assert detail() == b""

    def both(opts, *texts):
        for call in (lambda: B(buf, n, buf, n, 0, ctypes.byref(opts), None, 0, hist, ok),
                     lambda: F(b"x.fq", b"y.fq", None, ctypes.byref(opts), None, 0, hist, ok)):
            assert call() == scfq.SCFQ_EARG, texts
            for t in texts:
                assert t in detail(), (t, detail())

    both(scfq.insert_opts(min_overlap=0), b"min_overlap 0", b"1 .. 512")
    both(scfq.insert_opts(min_overlap=513), b"min_overlap 513", b"1 .. 512")
    both(scfq.insert_opts(max_mismatches=65536), b"max_mismatches 65536", b"0 .. 65535")
    both(scfq.insert_opts(max_mismatch_pct=101), b"max_mismatch_pct 101", b"0 .. 100")
    o = scfq.insert_opts()
    o.flags = 6
    both(o, b"unknown flag bits 0x6")
    both(scfq.insert_opts(interleaved=True), b"interleaved", b"no second")                              # the flag with two inputs
    assert B(buf, n, None, 5, 0, ctypes.byref(scfq.insert_opts(interleaved=True)), None, 0, hist, ok) == scfq.SCFQ_EARG
    with pytest.raises(scfq.ScfqError) as e:
        scfq.insert_size_host(FASTQ, FASTQ, (0, 5, 20))
    assert e.value.rc == scfq.SCFQ_EARG and "min_overlap 0" in str(e.value)
    # the edges of the ranges are allowed: what fails then is the missing device or nothing
    for params in ((1, 0, 0), (512, 65535, 100), None):
        for second in (FASTQ, None):
            try:
                scfq.insert_size_host(FASTQ, second, params)
            except scfq.ScfqError as err:
                assert err.rc == scfq.SCFQ_EHIP, err


def test_no_gpu_means_loud_failure(scfq):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r1, r2, il = (os.path.join(PAIRS, f) for f in ("r1.fq", "r2.fq", "interleaved.fq"))
    for params in (None, (1, 0, 0)):
        for call in (lambda: scfq.insert_size_host(FASTQ, FASTQ, params), lambda: scfq.insert_size_host(FASTQ, None, params),
                     lambda: scfq.insert_size_host(b"", b"", params), lambda: scfq.insert_size_file(r1, r2, params),
                     lambda: scfq.insert_size_file(r1, r2 + ".gz", params), lambda: scfq.insert_size_file(il, None, params)):
            with pytest.raises(scfq.ScfqError) as e:
                call()
            assert e.value.rc == scfq.SCFQ_EHIP
    for a, b in ((os.path.join(PAIRS, "does_not_exist.fq"), r2), (os.path.join(PAIRS, "does_not_exist.fq"), None)):
        with pytest.raises(scfq.ScfqError) as e:
            scfq.insert_size_file(a, b)
        assert e.value.rc == scfq.SCFQ_EOPEN
    r = run("fq-insert-size", r1, r2)
    assert r.returncode == 1 and r.stdout == "" and "HIP" in r.stderr


def summary(scfq, **fields):
    s = scfq._new_insert_summary()
    for k, v in fields.items():
        setattr(s, k, v)
    return s


def test_row_formatter(scfq):
    w = dict(pairs=8, overlapped=4, min_insert=100, median_insert=150, mode_insert=100, max_insert=300, read_through=1, insert_sum=700,
             insert_sq_sum=100 * 100 * 2 + 200 * 200 + 300 * 300, mismatches=3, overlap_bases=400)
    text = "8\t4\t50.0\t100\t150\t175.0\t%s\t100\t300\t1\t0.0075" % "82.915619758885"
    assert scfq.format_insert_size_tsv(summary(scfq, **w)) == text == summary_text(w)
    zero = dict(w, pairs=0, overlapped=0, insert_sum=0, insert_sq_sum=0, mismatches=0, overlap_bases=0, min_insert=0, median_insert=0, mode_insert=0,
                max_insert=0, read_through=0)
    assert scfq.format_insert_size_tsv(summary(scfq, **zero)) == "0\t0\tnan\t0\t0\tnan\tnan\t0\t0\t0\tnan" == summary_text(zero)      # 0 / 0
    none = dict(zero, pairs=5)
    assert scfq.format_insert_size_tsv(summary(scfq, **none)) == "5\t0\t0.0\t0\t0\tnan\tnan\t0\t0\t0\tnan" == summary_text(none)
    one = dict(w, pairs=1, overlapped=1, insert_sum=150, insert_sq_sum=22500, mismatches=0, overlap_bases=150)
    assert scfq.format_insert_size_tsv(summary(scfq, **one)).split("\t")[5:7] == ["150.0", "0.0"]
    # the variance's numerator is far above 2^53: 2e9 pairs, half of them at 100 and half at 1000
    half = 10 ** 9
    big = dict(w, pairs=2 * half, overlapped=2 * half, insert_sum=half * 1100, insert_sq_sum=half * (100 ** 2 + 1000 ** 2))
    num = big["overlapped"] * big["insert_sq_sum"] - big["insert_sum"] ** 2
    assert num == 81 * 10 ** 22 and num > 2 ** 53
    got = scfq.format_insert_size_tsv(summary(scfq, **big))
    assert got == summary_text(big) and got.split("\t")[5:7] == ["550.0", "450.0"]
    # ... and is no square: one more pair, at 7
    odd = dict(big, pairs=2 * half + 1, overlapped=2 * half + 1, insert_sum=big["insert_sum"] + 7, insert_sq_sum=big["insert_sq_sum"] + 49)
    num = odd["overlapped"] * odd["insert_sq_sum"] - odd["insert_sum"] ** 2
    assert num > 2 ** 64 and float(num) != num                     # (the conversion to a double rounds)
    got = scfq.format_insert_size_tsv(summary(scfq, **odd))
    assert got == summary_text(odd) and got.split("\t")[6].startswith("450.0000000")
    # the largest sums a run can reach: 2^31 pairs at 1023
    p = 2 ** 31 - 1
    top = dict(w, pairs=p, overlapped=p - 1, insert_sum=(p - 2) * 1023 + 1, insert_sq_sum=(p - 2) * 1023 ** 2 + 1, min_insert=1, max_insert=1023)
    assert scfq.format_insert_size_tsv(summary(scfq, **top)) == summary_text(top)
    L = scfq.lib()
    s = summary(scfq, **w)
    assert L.scfq_format_insert_size_tsv(ctypes.byref(s), None, 0) == len(text)                        # sizing call
    small = ctypes.create_string_buffer(5)
    assert L.scfq_format_insert_size_tsv(ctypes.byref(s), small, 5) == len(text) and small.value == text[:4].encode()
    exact = ctypes.create_string_buffer(len(text) + 1)
    assert L.scfq_format_insert_size_tsv(ctypes.byref(s), exact, len(text) + 1) == len(text) and exact.value.decode() == text
    assert L.scfq_format_insert_size_tsv(None, exact, len(text) + 1) == scfq.SCFQ_EARG


def test_cli_without_a_device():
    r = run("fq-insert-size", "--help")
    assert r.returncode == 0 and "fq-insert-size [options] R1.fq R2.fq" in r.stdout
    for opt in ("--interleaved", "--min-overlap=N", "--max-mismatches=N", "--max-mismatch-pct=N", "--dist", "-t, --header", "-b, --basename",
                "-a, --absolute", "-h, --help"):
        assert opt in r.stdout, opt
    assert run("fq-insert-size").stdout == r.stdout and run("fq-insert-size", "-h").stdout == r.stdout
    top = run("--help").stdout
    assert "Insert sizes from the overlap" in top and top.index("fq-adapters") < top.index("fq-insert-size") < top.index("FASTA")
    assert top[top.index("fq-adapters"):top.index("fq-insert-size")].count("\n") == 1                   # directly behind it
    r = run("fq-insert-size", "-t", "-b")
    assert (r.returncode, r.stdout, r.stderr) == (0, HEADER + "\tbasename\n", "")
    assert run("fq-insert-size", "-tba").stdout == HEADER + "\tbasename\tabsolute\n"
    assert run("fq-insert-size", "--header", "--min-overlap=1", "--max-mismatches=65535", "--max-mismatch-pct=100", "--interleaved").stdout == HEADER + "\n"
    assert run("fq-insert-size", "-t", "--dist").stdout == DIST_HEADER + "\n"
    assert run("fq-insert-size", "-ta", "--dist", "--interleaved").stdout == DIST_HEADER + "\tabsolute\n"
    r = run("fq-insert-size", "does_not_exist.fq", "nor_this.fq")
    c = run("fq-cycles", "does_not_exist.fq")
    assert (r.returncode, r.stderr, r.stdout) == (c.returncode, c.stderr, c.stdout) == (2, "\x1b[31mError 2: Unable to open file: does_not_exist.fq\x1b[0m\n", "")
    r = run("fq-insert-size", "--interleaved", "does_not_exist.fq")
    assert (r.returncode, r.stderr, r.stdout) == (c.returncode, c.stderr, c.stdout)
    r, c = run("fq-insert-size", "--interleaved", "missing.fq.gz"), run("fq-cycles", "missing.fq.gz")
    assert (r.returncode, r.stderr) == (c.returncode, c.stderr) and r.returncode == 1
    r, c = run("fq-insert-size", "-b"), run("fq-cycles", "-b")
    assert (r.returncode, r.stderr) == (c.returncode, c.stderr) == (3, "\x1b[31mError 3: No FASTQ specified\x1b[0m\n")
    r, c = run("fq-insert-size", "--bogus"), run("fq-cycles", "--bogus")
    assert (r.returncode, r.stderr) == (c.returncode, c.stderr) and r.returncode == 1
    r, c = run("fq-insert-size", "-x"), run("fq-cycles", "-x")
    assert (r.returncode, r.stderr) == (c.returncode, c.stderr) and r.returncode == 1
    # an odd number of files without --interleaved
    for files in (["a.fq"], ["a.fq", "b.fq", "c.fq"]):
        r = run("fq-insert-size", "-t", *files)
        assert r.returncode == 1 and HEADER not in r.stdout and "Error" in r.stderr and "two at a time" in r.stderr, files
    for bad in (["--min-overlap=0"], ["--min-overlap=513"], ["--min-overlap="], ["--min-overlap=x"], ["--min-overlap"], ["--min-overlap=-1"],
                ["--max-mismatches=65536"], ["--max-mismatches=x"], ["--max-mismatches="], ["--max-mismatch-pct=101"], ["--max-mismatch-pct=2.5"],
                ["--max-mismatch-pct"], ["--min-overlap=1000000000000"]):
        for dist in ((), ("--dist",)):
            r = run("fq-insert-size", "-t", *bad, *dist)
            assert r.returncode == 1 and HEADER not in r.stdout and DIST_HEADER not in r.stdout and "Error" in r.stderr, bad
    r, c = run("fq-insert-size", "--min-overlap=x"), run("fq-cycles", "--max-cycles=x")
    assert r.returncode == c.returncode == 1 and r.stderr == c.stderr.replace("--max-cycles", "--min-overlap")


def golden_files():
    return sorted(glob.glob(os.path.join(GOLDEN, "*.fq")) + glob.glob(os.path.join(GOLDEN, "edge", "*.fq")) + glob.glob(os.path.join(PAIRS, "*.fq")))


def check_agree(data1, data2, ctx, param_sets=PARAM_SETS):
    """the plain checker against the numpy one; the identities every result has to keep"""
    a1 = np.frombuffer(data1, dtype=np.uint8)
    a2 = None if data2 is None else np.frombuffer(data2, dtype=np.uint8)
    for params in param_sets:
        p = insert_of(data1, data2, params)
        q = insert_of_np(a1, a2, params)
        assert same(p, q), (ctx, params, {k: (p[k], q[k]) for k in FIELDS if p[k] != q[k]}, np.flatnonzero((p["recs"] != q["recs"]).any(axis=1))[:8])
        assert p["pairs"] == p["overlapped"] + p["not_overlapped"] + p["too_long"] == p["recs"].shape[0], ctx
        assert int(p["hist"].sum()) == p["overlapped"] and int(p["hist"][0]) == 0, ctx
        assert p["unpaired"] == (p["reads1"] & 1 if data2 is None else abs(p["reads1"] - p["reads2"])), ctx
        if p["overlapped"]:
            assert 1 <= p["min_insert"] <= p["median_insert"] <= p["max_insert"] <= 1023 and p["hist"][p["mode_insert"]] == p["hist"].max(), ctx


def test_checkers_agree_on_the_fixtures(scfq):
    assert hasattr(scfq, "insert_size_file")
    files = golden_files()
    assert len(files) >= 33
    for path in files:
        data = open(path, "rb").read()
        check_agree(data, None, path)
    r1, r2 = (open(os.path.join(PAIRS, f), "rb").read() for f in ("r1.fq", "r2.fq"))
    check_agree(r1, r2, "pairs")
    # the interleaved fixture holds the same pairs
    two, one = insert_of(r1, r2), insert_of(open(os.path.join(PAIRS, "interleaved.fq"), "rb").read())
    assert np.array_equal(two["recs"], one["recs"]) and np.array_equal(two["hist"], one["hist"]) and two["pairs"] == one["pairs"] == 88
    assert (two["overlapped"], two["not_overlapped"], two["too_long"], two["read_through"]) == (66, 22, 0, 22)
    for name in ("r1.fq", "r2.fq", "interleaved.fq", "r2.fq.gz"):
        assert os.path.getsize(os.path.join(PAIRS, name)) < 64 * 1024, name
    import gzip
    assert gzip.open(os.path.join(PAIRS, "r2.fq.gz")).read() == r2


@pytest.mark.parametrize("kind", ["uniform", "ascii", "dense_nl", "sparse_nl", "crlf"])
def test_checkers_agree_on_random_buffers(scfq, kind):
    assert hasattr(scfq, "insert_size_device")
    rng = np.random.default_rng(59)
    for n in (0, 1, 2, 15, 16, 17, 255, 4096, 12_000):
        a = random_fastq_like(rng, n, kind)
        b = random_fastq_like(rng, n // 2 + 3, kind)
        for cut in (n, n - 1, 2 * n // 3):
            if cut >= 0:
                check_agree(bytes(a[:cut]), None, (kind, n, cut, "interleaved"), PARAM_SETS[:3])
                check_agree(bytes(a[:cut]), bytes(b), (kind, n, cut, "two"), PARAM_SETS[1:3])


def test_literal_cases(scfq):
    assert hasattr(scfq, "format_insert_size_tsv")
    rng = np.random.default_rng(61)
    # planted inserts with 150 bp mates: the overlap is 30 or more from insert 30 to insert 270
    want = {1: None, 29: None, 30: (-120, 30, 0), 31: (-119, 31, 0), 149: (-1, 149, 0), 150: (0, 150, 0), 151: (1, 149, 0), 269: (119, 31, 0),
            270: (120, 30, 0), 271: None}
    mates = {ins: planted(rng, 150, 150, ins) for ins in want}
    for ins, rec in want.items():
        assert pair_of(*mates[ins]) == rec, ins
    res = insert_of(fastq([m[0] for m in mates.values()]), fastq([m[1] for m in mates.values()]))
    assert res["recs"].tolist() == [list(r or (0, 0, 0)) for r in want.values()]
    assert {int(s): int(res["hist"][s]) for s in np.flatnonzero(res["hist"])} == {s: 1 for s in want if want[s]}
    assert (res["pairs"], res["overlapped"], res["not_overlapped"], res["read_through"], res["min_insert"], res["max_insert"]) == (10, 7, 3, 3, 30, 270)
    assert (res["median_insert"], res["mode_insert"], res["insert_sum"], res["overlap_bases"]) == (150, 30, 30 + 31 + 149 + 150 + 151 + 269 + 270, 570)
    assert same(res, insert_of_np(np.frombuffer(fastq([m[0] for m in mates.values()]), np.uint8), np.frombuffer(fastq([m[1] for m in mates.values()]), np.uint8)))
    both = fastq(interleave(*zip(*mates.values())))
    assert same(insert_of(both), dict(res, reads1=20, lines1=80, reads2=0, lines2=0, input_bytes1=len(both), input_bytes2=0))
    # a tie: every offset 0, 4, .. 20 has the whole of C agreeing; the largest wins
    assert pair_of(b"ACGT" * 15, revcomp(b"ACGT" * 10)) == (20, 40, 0)
    # ... and poly-A against poly-T: every offset agrees everywhere, the largest overlap is the shorter read, at the largest d
    assert pair_of(b"A" * 100, b"T" * 60) == (40, 60, 0) and pair_of(b"A" * 60, b"T" * 100) == (0, 60, 0)
    assert pair_of(b"A" * 40, b"A" * 40) is None
    # an N inside the overlap is a mismatch, in either mate or in both at one place; so are lower case and high bytes
    a, b = planted(rng, 150, 150, 150)
    assert pair_of(a, b) == (0, 150, 0)
    hit = lambda s, i, ch: s[:i] + ch + s[i + 1:]
    assert pair_of(hit(a, 10, b"N"), b) == (0, 150, 1) and pair_of(a, hit(b, 149 - 10, b"N")) == (0, 150, 1)
    assert pair_of(hit(a, 10, b"N"), hit(b, 149 - 10, b"N")) == (0, 150, 1)
    assert pair_of(hit(a, 10, a[10:11].lower()), b) == (0, 150, 1) and pair_of(hit(a, 10, b"\xc1"), hit(b, 3, b"\xff")) == (0, 150, 2)
    assert pair_of(b"N" * 150, b"N" * 150) is None and pair_of(a.lower(), b.lower()) is None
    # the 20 % rule binds before the count does: overlap 10 with 3 mismatches (3 <= 5, but 300 > 200)
    a, b = planted(rng, 50, 50, 90)
    c = revcomp(b)
    flip = lambda s, i: hit(s, i, b"C" if s[i:i + 1] != b"C" else b"G")
    for k, rec in ((0, (40, 10, 0)), (1, (40, 10, 1)), (2, (40, 10, 2)), (3, None)):
        cc = c
        for i in (0, 5, 9)[:k]:
            cc = flip(cc, i)
        assert pair_of(a, revcomp(cc), (10, 5, 20)) == rec, k
    assert pair_of(a, revcomp(flip(flip(flip(c, 0), 5), 9)), (10, 5, 30)) == (40, 10, 3)
    # max_mismatches binds where the percentage does not
    a, b = planted(rng, 150, 150, 150)
    six = a
    for i in (0, 20, 63, 64, 100, 149):
        six = flip(six, i)
    assert pair_of(six, b) is None and pair_of(six, b, (30, 6, 20)) == (0, 150, 6)
    # empty and missing lines, a lone record, CR LF
    assert insert_of(b"", b"")["pairs"] == 0 and insert_of(b"")["pairs"] == 0
    res = insert_of(fastq([a]), b"")
    assert (res["pairs"], res["unpaired"], res["reads1"], res["reads2"]) == (0, 1, 1, 0)
    res = insert_of(fastq([a, b, a]))
    assert (res["pairs"], res["unpaired"], res["overlapped"]) == (1, 1, 1)
    res = insert_of(fastq([a], b"\r\n"), fastq([b], b"\r\n"))
    assert res["recs"].tolist() == [[0, 150, 0]]
    res = insert_of(fastq([a]), b"@r0\n")                      # mate 2 has no sequence line
    assert (res["pairs"], res["not_overlapped"]) == (1, 1)
    # too long: 513, and never looked at
    res = insert_of(fastq([a + a + a + a[:63], a]), fastq([b, b * 4]))
    assert res["recs"].tolist() == [[0, 0, 0xFFFF]] * 2 and (res["too_long"], res["overlapped"], res["not_overlapped"]) == (2, 0, 0)
    # the text the CLI prints
    res = insert_of(fastq([m[0] for m in mates.values()]), fastq([m[1] for m in mates.values()]))
    assert cli_text(res, dist=True, suffix="\tx") == "".join("%d\t1\tx\n" % s for s in (30, 31, 149, 150, 151, 269, 270))
    ins = (30, 31, 149, 150, 151, 269, 270)
    sd = float(7 * sum(s * s for s in ins) - sum(ins) ** 2) ** 0.5 / 7
    assert abs(sd - np.std(ins)) < 1e-9
    assert cli_text(res) == "10\t7\t70.0\t30\t150\t150.0\t%s\t30\t270\t3\t0.0\n" % nimf(sd)


def test_unrelated_pairs_do_not_overlap(scfq):
    """a condition the GPU tests rest on when they count planted pairs literally: at the defaults nothing is accepted in 300 pairs of
    unrelated random 150 bp reads (about 3e-11 per offset)"""
    assert hasattr(scfq, "insert_size_host")
    rng = np.random.default_rng(67)
    m1, m2 = [random_dna(rng, 150) for _ in range(300)], [random_dna(rng, 150) for _ in range(300)]
    res = insert_of(fastq(m1), fastq(m2))
    assert (res["pairs"], res["overlapped"], res["not_overlapped"]) == (300, 0, 300) and not res["recs"].any() and not res["hist"].any()

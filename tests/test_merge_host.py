"""fq-merge without a device: the ABI (symbols, struct layout, C99 header), argument checks, the stats formatter, the CLI's help / error
behaviour, literal cases of the contract whose merged records are written out by hand, the two checkers of _merge_check.py against
each other and against _insert_size_check, and the golden outputs of the pairs fixture."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG, ROOT
from _insert_size_check import insert_of, paired_block, revcomp
from _readstats_check import line_spans_np
from _merge_check import FIELDS, STATS_HEADER, consensus, merge_of, merge_of_np, same, stat, stats_text, with_random_qualities
from test_gpu_parity import random_fastq_like

SC = os.path.join(PKG, "sc")
PAIRS = os.path.join(GOLDEN, "pairs")
NEW = ("scfq_merge_buffers", "scfq_merge_files", "scfq_format_merge_stats_tsv", "scfq_merge_error_detail")
STATS = ("struct_size", "abi_version") + FIELDS
FASTQ = b"@h\nACGTN\n+\nIIIII\n"


def run(*args):
    return subprocess.run([SC] + list(args), capture_output=True, text=True, stdin=subprocess.DEVNULL)


def test_symbols_declared_exported_and_listed(scfq):
    header = open(os.path.join(ROOT, "include", "sc_fqcount.h")).read()
    debug = open(os.path.join(ROOT, "include", "sc_fqcount_debug.h")).read()
    L = scfq.lib()
    for name in NEW:
        assert name + "(" in header and name in scfq.EXPORTS and hasattr(L, name), name
    assert "scfq_debug_merge_stages(" in debug and "scfq_debug_merge_stages" in scfq.EXPORTS and hasattr(L, "scfq_debug_merge_stages")
    assert len(scfq.merge_stages()) == 4
    assert scfq.SCFQ_MERGE_INTERLEAVED == 1 and "SCFQ_MERGE_INTERLEAVED" in header
    for name in ("MergeOpts", "MergeStats", "merge_device", "merge_host", "merge_file", "format_merge_stats_tsv", "merge_stages"):
        assert hasattr(scfq, name), name


def test_struct_layout(scfq):
    O, S = scfq.MergeOpts, scfq.MergeStats
    assert ctypes.sizeof(O) == 32
    assert [(n, getattr(O, n).offset) for n, _ in O._fields_] == [("struct_size", 0), ("flags", 8), ("min_overlap", 12), ("max_mismatches", 16),
                                                                  ("max_mismatch_pct", 20), ("phred_offset", 24), ("reserved", 28)]
    assert tuple(f[0] for f in S._fields_) == STATS and len(STATS) == 26
    for k, name in enumerate(STATS):
        assert getattr(S, name).offset == 8 * k and getattr(S, name).size == 8, name
    assert ctypes.sizeof(S) == 8 * 26


def test_header_is_c99_and_sizes_agree(tmp_path):
    src = tmp_path / "t.c"
    offsets = " && ".join("offsetof(scfq_merge_stats, %s) == %d" % (name, 8 * k) for k, name in enumerate(STATS))
    offsets += " && offsetof(scfq_merge_opts, flags) == 8 && offsetof(scfq_merge_opts, phred_offset) == 24 && offsetof(scfq_merge_opts, reserved) == 28"
    src.write_text('#include <stddef.h>\n#include "sc_fqcount.h"\n#include "sc_fqcount_debug.h"\n'
                   "typedef char stats_size[sizeof(scfq_merge_stats) == 8 * 26 ? 1 : -1];\n"
                   "typedef char opt_size[sizeof(scfq_merge_opts) == 32 ? 1 : -1];\n"
                   "typedef char at[" + offsets + " ? 1 : -1];\n"
                   "typedef char consts[SCFQ_MERGE_INTERLEAVED == 1 ? 1 : -1];\n"
                   "int main(void){ scfq_merge_stats s; scfq_merge_opts o; double ms[4]; char out[8];\n"
                   "  s.struct_size = sizeof s; o.struct_size = sizeof o; o.flags = 0; o.min_overlap = 30; o.max_mismatches = 5; o.max_mismatch_pct = 20;\n"
                   "  o.phred_offset = 33; o.reserved = 0;\n"
                   "  return scfq_merge_buffers(0, 0, 0, 0, 0, &o, out, 8, 0, 0, 0, 0, 0, &s) + scfq_format_merge_stats_tsv(&s, 0, 0)\n"
                   "         + scfq_merge_files(\"x\", \"y\", 0, &o, 1, -1, -1, &s) + scfq_debug_merge_stages(ms, 4)\n"
                   "         + (scfq_merge_error_detail() != 0) == 12345; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-fsyntax-only", str(src)])


def test_argument_checks(scfq):
    L = scfq.lib()
    s = scfq._new_merge_stats()
    buf = ctypes.create_string_buffer(FASTQ)
    n = len(FASTQ)
    out = ctypes.create_string_buffer(64)
    ok = ctypes.byref(s)
    detail = L.scfq_merge_error_detail
    B, F = L.scfq_merge_buffers, L.scfq_merge_files
    none = (None, 0, None, 0, None, 0, 0)
    # without text
    assert B(buf, n, buf, n, 0, None, *none, None) == scfq.SCFQ_EARG                                    # NULL stats
    bad = scfq.MergeStats()                                                                           # struct_size not set
    assert B(buf, n, buf, n, 0, None, *none, ctypes.byref(bad)) == scfq.SCFQ_EARG
    bad.struct_size = ctypes.sizeof(scfq.MergeStats) - 8
    assert B(buf, n, buf, n, 0, None, *none, ctypes.byref(bad)) == scfq.SCFQ_EARG
    assert B(None, n, buf, n, 0, None, *none, ok) == scfq.SCFQ_EARG                                     # NULL pointer with n > 0
    assert B(buf, n, None, n, 0, None, *none, ok) == scfq.SCFQ_EARG
    for k in range(3):                                                                                # NULL output with a capacity
        caps = [None, 0, None, 0, None, 0, 0]
        caps[2 * k + 1] = 8
        assert B(buf, n, buf, n, 0, None, *caps, ok) == scfq.SCFQ_EARG, k
    small = scfq.merge_opts()
    small.struct_size -= 4
    assert B(buf, n, buf, n, 0, ctypes.byref(small), *none, ok) == scfq.SCFQ_EARG                       # wrong size of the options
    assert F(None, b"y.fq", None, None, -1, -1, -1, ok) == scfq.SCFQ_EARG
    assert F(b"x.fq", b"y.fq", None, None, -1, -1, -1, ctypes.byref(bad)) == scfq.SCFQ_EARG
    assert F(b"x.fq", b"y.fq", None, ctypes.byref(small), -1, -1, -1, ok) == scfq.SCFQ_EARG
    assert detail() == b""

    def both(opts, *texts):
        for call in (lambda: B(buf, n, buf, n, 0, ctypes.byref(opts), *none, ok),
                     lambda: F(b"x.fq", b"y.fq", None, ctypes.byref(opts), -1, -1, -1, ok)):
            assert call() == scfq.SCFQ_EARG, texts
            for t in texts:
                assert t in detail(), (t, detail())

    both(scfq.merge_opts(min_overlap=0), b"min_overlap 0", b"1 .. 512")
    both(scfq.merge_opts(min_overlap=513), b"min_overlap 513", b"1 .. 512")
    both(scfq.merge_opts(max_mismatches=65536), b"max_mismatches 65536", b"0 .. 65535")
    both(scfq.merge_opts(max_mismatch_pct=101), b"max_mismatch_pct 101", b"0 .. 100")
    for q0 in (0, 32, 34, 63, 65, 126):
        both(scfq.merge_opts(phred_offset=q0), b"phred_offset %d" % q0, b"33 or 64")
    o = scfq.merge_opts()
    o.reserved = 7
    both(o, b"reserved", b"7")
    o = scfq.merge_opts()
    o.flags = 6
    both(o, b"unknown flag bits 0x6")
    both(scfq.merge_opts(interleaved=True), b"interleaved", b"no second")                               # the flag with two inputs
    il = scfq.merge_opts(interleaved=True)
    assert B(buf, n, None, 5, 0, ctypes.byref(il), *none, ok) == scfq.SCFQ_EARG
    # a second unmerged output with interleaved input
    assert B(buf, n, None, 0, 0, ctypes.byref(il), None, 0, None, 0, out, 64, 0, ok) == scfq.SCFQ_EARG and b"unmerged2" in detail()
    assert F(b"x.fq", None, None, ctypes.byref(il), -1, -1, 5, ok) == scfq.SCFQ_EARG and b"unmerged2" in detail()
    assert F(b"x.fq", None, None, None, -1, -1, 5, ok) == scfq.SCFQ_EARG and b"unmerged2" in detail()
    with pytest.raises(scfq.ScfqError) as e:
        scfq.merge_host(FASTQ, FASTQ, (0, 5, 20))
    assert e.value.rc == scfq.SCFQ_EARG and "min_overlap 0" in str(e.value) and isinstance(e.value.stats, scfq.MergeStats)
    with pytest.raises(scfq.ScfqError) as e:
        scfq.merge_host(FASTQ, FASTQ, phred_offset=50)
    assert e.value.rc == scfq.SCFQ_EARG and "phred_offset 50" in str(e.value)
    # the edges of the ranges are allowed: what fails then is the missing device or nothing
    for params in ((1, 0, 0), (512, 65535, 100), None):
        for second in (FASTQ, None):
            for q0 in (33, 64):
                try:
                    scfq.merge_host(FASTQ, second, params, q0)
                except scfq.ScfqError as err:
                    assert err.rc == scfq.SCFQ_EHIP, err


def test_no_gpu_means_loud_failure(scfq, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r1, r2, il = (os.path.join(PAIRS, f) for f in ("r1.fq", "r2.fq", "interleaved.fq"))
    for call in (lambda: scfq.merge_host(FASTQ, FASTQ), lambda: scfq.merge_host(FASTQ, None), lambda: scfq.merge_host(b"", b""),
                 lambda: scfq.merge_host(FASTQ, FASTQ, caps=(100, 100, 100)), lambda: scfq.merge_file(r1, r2),
                 lambda: scfq.merge_file(r1, r2 + ".gz", (1, 0, 0), 64), lambda: scfq.merge_file(il, None)):
        with pytest.raises(scfq.ScfqError) as e:
            call()
        assert e.value.rc == scfq.SCFQ_EHIP
    for a, b in ((os.path.join(PAIRS, "does_not_exist.fq"), r2), (os.path.join(PAIRS, "does_not_exist.fq"), None)):
        with pytest.raises(scfq.ScfqError) as e:
            scfq.merge_file(a, b)
        assert e.value.rc == scfq.SCFQ_EOPEN
    un = tmp_path / "un1.fq"
    r = run("fq-merge", "--unmerged1=" + str(un), r1, r2)
    assert r.returncode == 1 and r.stdout == "" and "HIP" in r.stderr
    assert not un.exists()                                   # a call that fails leaves no output file behind


def test_stats_formatter(scfq):
    w = dict(pairs=8, merged_pairs=6, not_overlapped=1, too_long=1, unpaired=2, merged_bases=1200, overlap_bases=600, mismatches=7, took_mate1=3,
             took_mate2=2, neither_valid=1, merged_bytes=2500, unmerged1_bytes=640, unmerged2_bytes=650)
    s = scfq._new_merge_stats()
    for k in w:
        setattr(s, "merged" if k == "merged_pairs" else k, w[k])
    text = "8\t6\t75.0\t1\t1\t2\t1200\t600\t7\t3\t2\t1\t2500\t640\t650"
    assert scfq.format_merge_stats_tsv(s) == text == stats_text(w)
    assert len(STATS_HEADER.split("\t")) == len(text.split("\t")) == 15
    zero = scfq._new_merge_stats()
    assert scfq.format_merge_stats_tsv(zero) == "0\t0\tnan" + "\t0" * 12
    third = scfq._new_merge_stats()
    third.pairs, third.merged = 3, 1
    assert scfq.format_merge_stats_tsv(third).split("\t")[2] == "33.33333333333334"
    L = scfq.lib()
    assert L.scfq_format_merge_stats_tsv(ctypes.byref(s), None, 0) == len(text)                          # sizing call
    small = ctypes.create_string_buffer(5)
    assert L.scfq_format_merge_stats_tsv(ctypes.byref(s), small, 5) == len(text) and small.value == text[:4].encode()
    exact = ctypes.create_string_buffer(len(text) + 1)
    assert L.scfq_format_merge_stats_tsv(ctypes.byref(s), exact, len(text) + 1) == len(text) and exact.value.decode() == text
    assert L.scfq_format_merge_stats_tsv(None, exact, len(text) + 1) == scfq.SCFQ_EARG


def test_cli_without_a_device(tmp_path):
    r = run("fq-merge", "--help")
    assert r.returncode == 0 and "fq-merge [options] R1.fq R2.fq" in r.stdout and "fq-merge [options] --interleaved IN.fq" in r.stdout
    for opt in ("--interleaved", "--unmerged1=PATH", "--unmerged2=PATH", "--unmerged=PATH", "--min-overlap=N", "--max-mismatches=N",
                "--max-mismatch-pct=N", "--phred-offset=N", "--stats", "-h, --help"):
        assert opt in r.stdout, opt
    assert run("fq-merge").stdout == r.stdout and run("fq-merge", "-h").stdout == r.stdout
    top = run("--help").stdout
    assert "Merge overlapping read pairs" in top and top.index("fq-insert-size") < top.index("fq-merge") < top.index("FASTA")
    assert top[top.index("fq-insert-size"):top.index("fq-merge")].count("\n") == 1                      # directly behind it
    r = run("fq-merge", "does_not_exist.fq", "nor_this.fq")
    c = run("fq-cycles", "does_not_exist.fq")
    assert (r.returncode, r.stderr, r.stdout) == (c.returncode, c.stderr, c.stdout) == (2, "\x1b[31mError 2: Unable to open file: does_not_exist.fq\x1b[0m\n", "")
    r1 = os.path.join(PAIRS, "r1.fq")
    un = tmp_path / "never_made.fq"
    r = run("fq-merge", "--unmerged1=" + str(un), r1, "nor_this.fq")
    assert (r.returncode, r.stdout) == (2, "") and "Unable to open file: nor_this.fq" in r.stderr and not un.exists()
    r = run("fq-merge", "--interleaved", "does_not_exist.fq")
    assert (r.returncode, r.stderr, r.stdout) == (c.returncode, c.stderr, c.stdout)
    r, c = run("fq-merge", "--interleaved", "missing.fq.gz"), run("fq-cycles", "missing.fq.gz")
    assert (r.returncode, r.stderr) == (c.returncode, c.stderr) and r.returncode == 1
    r = run("fq-merge", "--stats")
    assert (r.returncode, r.stderr) == (3, "\x1b[31mError 3: No FASTQ specified\x1b[0m\n")
    r, c = run("fq-merge", "--bogus"), run("fq-cycles", "--bogus")
    assert (r.returncode, r.stderr) == (c.returncode, c.stderr) and r.returncode == 1
    assert run("fq-merge", "-x").returncode == 1
    # the number of files, and which --unmerged goes with which input form
    for args in (["a.fq"], ["a.fq", "b.fq", "c.fq"], ["--interleaved", "a.fq", "b.fq"], ["--interleaved", "--unmerged1=u.fq", "a.fq"],
                 ["--interleaved", "--unmerged2=u.fq", "a.fq"], ["--unmerged=u.fq", "a.fq", "b.fq"]):
        r = run("fq-merge", *args)
        assert r.returncode == 1 and "Error" in r.stderr and "@" not in r.stdout, args
    for bad in (["--min-overlap=0"], ["--min-overlap=513"], ["--min-overlap="], ["--min-overlap=x"], ["--min-overlap"], ["--min-overlap=-1"],
                ["--max-mismatches=65536"], ["--max-mismatches=x"], ["--max-mismatch-pct=101"], ["--max-mismatch-pct=2.5"], ["--phred-offset=34"],
                ["--phred-offset=0"], ["--phred-offset=x"], ["--phred-offset="], ["--phred-offset=65"], ["--unmerged1="], ["--unmerged2="],
                ["--unmerged="]):
        r = run("fq-merge", *bad, r1, r1)
        assert r.returncode == 1 and "Error" in r.stderr and "@" not in r.stdout, bad
    r, c = run("fq-merge", "--min-overlap=x"), run("fq-cycles", "--max-cycles=x")
    assert r.returncode == c.returncode == 1 and r.stderr == c.stderr.replace("--max-cycles", "--min-overlap")


# ---- literal cases: the merged record is written out by hand, C = revcomp(B) and QC = QB reversed are given in the comments ------------
LITERAL = [
    # both valid and equal everywhere, d* = 0: the larger quality byte.  C = ACGTTGCAAG, QC = 55555IIIII
    ("equal", b"ACGTTGCAAG", b"I5I5I5I5I5", b"CTTGCAACGT", b"IIIII55555", (4, 1, 100), 33,
     b"@equal\nACGTTGCAAG\n+\nI5I5IIIIII\n", (0, 0, 0)),
    # both valid and different at 1 (mate 1 has the larger byte: 'I' against '5', 33 + 20 = '5'), at 7 (a tie goes to mate 1, 33 + 2 = '#')
    # and at 9 (mate 2 has the larger byte: '+' against 'I', 33 + 30 = '?').  C = AGGTTGCTAC, QC = I5IIIIIIII
    ("different", b"ACGTTGCAAG", b"IIIIIIIII+", b"GTAGCAACCT", b"IIIIIIII5I", (4, 3, 100), 33,
     b"@different\nACGTTGCAAC\n+\nI5IIIII#I?\n", (2, 1, 0)),
    # exactly one valid at 3 (mate 2's T, its 'G') and at 5 (mate 1's G, its 'F'), neither at 8 (A[8] = N, the smaller byte 'B').
    # C = ACGTTNCANG, QC = JIHGFEDCBA
    ("n", b"ACGNTGCANG", b"ABCDEFGHIJ", b"CNTGNAACGT", b"ABCDEFGHIJ", (4, 3, 100), 33,
     b"@n\nACGTTGCANG\n+\nJIHGFFGHBJ\n", (0, 0, 1)),
    # d* = -4: both mates read through the insert ACGTTG into adapter; what lies outside [0, 6) is dropped.  C = GGGGACGTTG, QC = !!!!5J5555
    ("through", b"ACGTTGTTTT", b"IIIIIIIIII", b"CAACGTCCCC", b"5555J5!!!!", (4, 0, 0), 33,
     b"@through\nACGTTG\n+\nIJIIII\n", (0, 0, 0)),
    # d* = 6 and s = 14 > La = 10: mate 1 alone, the overlap of 4, mate 2 alone.  C = CAAGTCCA, QC = abcdefgh
    ("longer", b"ACGTTGCAAG", b"ABCDEFGHIJ", b"TGGACTTG", b"hgfedcba", (4, 0, 0), 33,
     b"@longer\nACGTTGCAAGTCCA\n+\nABCDEFabcdefgh\n", (0, 0, 0)),
    # mate 2 contained in mate 1: d* = 3, s = 9 < La = 12, C ends the fragment.  C = TTGCAA, QC = JJJJJJ
    ("contained", b"ACGTTGCAAGTC", b"IIIIIIIIIIII", b"TTGCAA", b"JJJJJJ", (4, 0, 0), 33,
     b"@contained\nACGTTGCAA\n+\nIIIJJJJJJ\n", (0, 0, 0)),
    # quality lines shorter than their sequence lines: the missing bytes count as '!'.  QA covers A[0..1]; QB covers B[0..4], which are
    # the positions 9 .. 5
    ("short", b"ACGTTGCAAG", b"II", b"CTTGCAACGT", b"55555", (4, 1, 100), 33,
     b"@short\nACGTTGCAAG\n+\nII!!!55555\n", (0, 0, 0)),
    # Q0 = 64: different at 1 ('h' against 'T': 64 + 20 = 'T') and at 5 ('~' against '!': 64 + 93 is cut to 126 = '~'), mate 1 both times.
    # C = AGGTTCCAAG, QC = hThhh!hhhh
    ("q64", b"ACGTTGCAAG", b"hhhhh~hhhh", b"CTTGGAACCT", b"hhhh!hhhTh", (4, 2, 100), 64,
     b"@q64\nACGTTGCAAG\n+\nhThhh~hhhh\n", (2, 0, 0)),
    # ... the same pair at Q0 = 33: 33 + 20 = '5', and 33 + 93 = 126 = '~'
    ("q33", b"ACGTTGCAAG", b"hhhhh~hhhh", b"CTTGGAACCT", b"hhhh!hhhTh", (4, 2, 100), 33,
     b"@q33\nACGTTGCAAG\n+\nh5hhh~hhhh\n", (2, 0, 0)),
    # a missing quality byte at Q0 = 64 is '@': QA is empty, so every overlap byte is the larger of '@' and QC's
    ("q64short", b"ACGTTGCAAG", b"", b"CTTGCAACGT", b"AAAAA?????", (4, 0, 0), 64,
     b"@q64short\nACGTTGCAAG\n+\n@@@@@AAAAA\n", (0, 0, 0)),
]


def record(name, seq, qual, eol=b"\n"):
    return b"@" + name.encode() + eol + seq + eol + b"+" + eol + qual + eol


@pytest.mark.parametrize("case", LITERAL, ids=[c[0] for c in LITERAL])
def test_literal_cases(scfq, case):
    assert hasattr(scfq, "merge_host")
    name, a, qa, b, qb, params, q0, merged, counts = case
    for eol in (b"\n", b"\r\n"):
        got = merge_of(record(name, a, qa, eol), record(name, b, qb, eol), params, q0)
        assert got["merged"] == merged and (got["took_mate1"], got["took_mate2"], got["neither_valid"]) == counts, (name, got["merged"])
        assert (got["merged_pairs"], got["unmerged1"], got["unmerged2"], got["merged_bytes"]) == (1, b"", b"", len(merged))
        assert got["merged_bases"] == (len(merged) - len(name) - 6) // 2
        assert same(got, merge_of_np(np.frombuffer(record(name, a, qa, eol), np.uint8), np.frombuffer(record(name, b, qb, eol), np.uint8), params, q0)), name
        # interleaved: the same record
        il = merge_of(record(name, a, qa, eol) + record(name, b, qb, eol), None, params, q0)
        assert il["merged"] == merged and il["unmerged1"] == b""


def test_literal_unmerged_and_mixed(scfq):
    assert hasattr(scfq, "merge_file")
    a, b = b"ACGTTGCAAG", b"GGGGGGGGGG"                               # nothing agrees
    r1, r2 = record("u", a, b"IIIIIIIIII", b"\r\n"), b"@u/2\n" + b + b"\n+\n55555"      # CR LF in; a quality line cut short, no final newline
    got = merge_of(r1, r2, (4, 0, 0))
    assert (got["merged"], got["unmerged1"], got["unmerged2"]) == (b"", b"@u\nACGTTGCAAG\n+\nIIIIIIIIII\n", b"@u/2\nGGGGGGGGGG\n+\n55555\n")
    assert (got["merged_pairs"], got["not_overlapped"], got["too_long"], got["unpaired"]) == (0, 1, 0, 0)
    il = merge_of(r1 + r2, None, (4, 0, 0))
    assert (il["merged"], il["unmerged1"], il["unmerged2"]) == (b"", got["unmerged1"] + got["unmerged2"], b"")
    # a merged pair between two unmerged ones, a too-long pair, and a record without a mate: the outputs keep pair order
    name, ma, mqa, mb, mqb, params, q0, merged, _ = LITERAL[0]
    long_a = b"ACGT" * 129                                            # 516 bases
    r1 = record("x", a, b"I" * 10) + record(name, ma, mqa) + record("l", long_a, b"I" * 516) + record("y", a, b"5" * 10) + record("alone", a, b"I" * 10)
    r2 = record("x", b, b"I" * 10) + record(name, mb, mqb) + record("l", revcomp(long_a), b"I" * 516) + record("y", b, b"5" * 10)
    got = merge_of(r1, r2, params, q0)
    assert got["merged"] == merged
    assert got["unmerged1"] == record("x", a, b"I" * 10) + record("l", long_a, b"I" * 516) + record("y", a, b"5" * 10)
    assert got["unmerged2"] == record("x", b, b"I" * 10) + record("l", revcomp(long_a), b"I" * 516) + record("y", b, b"5" * 10)
    assert (got["pairs"], got["merged_pairs"], got["not_overlapped"], got["too_long"], got["unpaired"]) == (4, 1, 2, 1, 1)
    assert same(got, merge_of_np(np.frombuffer(r1, np.uint8), np.frombuffer(r2, np.uint8), params, q0))
    # empty inputs
    for d1, d2 in ((b"", b""), (b"", None), (r1, b"")):
        got = merge_of(d1, d2)
        assert (got["merged"], got["unmerged1"], got["unmerged2"], got["pairs"]) == (b"", b"", b"", 0)
    assert consensus(b"A", b"I", b"T", b"J", 0) == (b"A", b"J", 0, 0, 0)


def check_agree(data1, data2, ctx, param_sets=((30, 5, 20), (1, 65535, 100), (3, 1, 50)), q0s=(33, 64)):
    """the plain checker against the numpy one and against fq-insert-size's; the identities every result has to keep"""
    a1 = np.frombuffer(data1, dtype=np.uint8)
    a2 = None if data2 is None else np.frombuffer(data2, dtype=np.uint8)
    for params in param_sets:
        ins = insert_of(data1, data2, params)
        for q0 in q0s:
            p = merge_of(data1, data2, params, q0)
            q = merge_of_np(a1, a2, params, q0)
            assert same(p, q), (ctx, params, q0, [k for k in p if p[k] != q[k]])
            assert (p["overlap_bases"], p["mismatches"], p["merged_pairs"], p["not_overlapped"], p["too_long"], p["pairs"], p["unpaired"]) == \
                   (ins["overlap_bases"], ins["mismatches"], ins["overlapped"], ins["not_overlapped"], ins["too_long"], ins["pairs"], ins["unpaired"]), ctx
            assert p["merged_bases"] == ins["insert_sum"], ctx
            assert p["took_mate1"] + p["took_mate2"] + p["neither_valid"] <= p["mismatches"], ctx
            assert p["merged"].count(b"\n") == 4 * p["merged_pairs"], ctx
            assert all(stat(p, k) >= 0 for k in FIELDS)


def test_checkers_agree_on_the_fixtures(scfq):
    assert hasattr(scfq, "merge_device")
    r1, r2, il = (open(os.path.join(PAIRS, f), "rb").read() for f in ("r1.fq", "r2.fq", "interleaved.fq"))
    check_agree(r1, r2, "pairs")
    check_agree(il, None, "interleaved", q0s=(33,))
    two, one = merge_of(r1, r2), merge_of(il)
    assert two["merged"] == one["merged"] and (two["merged_pairs"], two["not_overlapped"], two["too_long"]) == (66, 22, 0)
    lines = one["unmerged1"].split(b"\n")[:-1]
    assert b"".join(lines[k] + b"\n" for k in range(len(lines)) if k % 8 < 4) == two["unmerged1"]
    assert b"".join(lines[k] + b"\n" for k in range(len(lines)) if k % 8 >= 4) == two["unmerged2"]
    for name in ("dup.fq", "illumina_8.fq", os.path.join("edge", "crlf.fq"), os.path.join("edge", "trunc6.fq"), os.path.join("edge", "n_rich.fq")):
        data = open(os.path.join(GOLDEN, name), "rb").read()
        check_agree(data, None, name, param_sets=((30, 5, 20), (1, 65535, 100)), q0s=(33,))
        check_agree(data, data[: len(data) // 2], name, param_sets=((1, 65535, 100),), q0s=(64,))


def test_golden_outputs(scfq):
    """the checker's outputs for the pairs fixture are committed: a change of the contract shows as a diff of FASTQ text"""
    assert hasattr(scfq, "format_merge_stats_tsv")
    r1, r2 = (open(os.path.join(PAIRS, f), "rb").read() for f in ("r1.fq", "r2.fq"))
    got = merge_of(r1, r2)
    for name, key in (("merged.fq", "merged"), ("unmerged1.fq", "unmerged1"), ("unmerged2.fq", "unmerged2")):
        path = os.path.join(PAIRS, name)
        assert open(path, "rb").read() == got[key], name
        assert 0 < os.path.getsize(path) < 64 * 1024, name
    assert stats_text(got) == "88\t66\t75.0\t22\t0\t0\t10550\t5812\t26\t18\t0\t0\t22016\t6684\t6842"


@pytest.mark.parametrize("kind", ["ascii", "dense_nl", "sparse_nl", "crlf"])
def test_checkers_agree_on_random_buffers(scfq, kind):
    assert hasattr(scfq, "merge_host")
    rng = np.random.default_rng(73)
    for n in (0, 1, 2, 17, 255, 4096):
        a = random_fastq_like(rng, n, kind)
        b = random_fastq_like(rng, n // 2 + 3, kind)
        for cut in (n, n - 1, 2 * n // 3):
            if cut >= 0:
                check_agree(bytes(a[:cut]), None, (kind, n, cut, "interleaved"), param_sets=((1, 65535, 100), (3, 1, 50)), q0s=(33,))
                check_agree(bytes(a[:cut]), bytes(b), (kind, n, cut, "two"), param_sets=((1, 65535, 100),), q0s=(64,))


def test_checkers_agree_on_random_qualities(scfq):
    assert hasattr(scfq, "merge_stages")
    rng = np.random.default_rng(79)
    a, b = paired_block(rng, 300, 150, 120, errors=0.03)
    a, b = with_random_qualities(rng, a), with_random_qualities(rng, b)
    # substitutions, so that the row "both valid, different" occurs
    for arr in (a, b):
        idx = np.flatnonzero(np.isin(arr, np.frombuffer(b"ACGT", np.uint8)) & (rng.random(arr.size) < 0.01))
        seq_line = np.zeros(arr.size, bool)
        s, e = line_spans_np(arr)
        for s0, e0 in zip(s[1::4], e[1::4]):
            seq_line[s0:e0] = True
        idx = idx[seq_line[idx]]
        arr[idx] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, idx.size)]
    params = (30, 30, 30)                       # (enough room for pairs with an N in both mates at one place)
    p = merge_of(a.tobytes(), b.tobytes(), params)
    assert same(p, merge_of_np(a, b, params))
    assert p["took_mate1"] > 0 and p["took_mate2"] > 0 and p["neither_valid"] > 0 and p["merged_pairs"] > 100
    ins = insert_of(a.tobytes(), b.tobytes(), params)
    assert (p["overlap_bases"], p["mismatches"]) == (ins["overlap_bases"], ins["mismatches"])

"""fq-complexity without a device: the two per-read functions of the checker (_complexity_check.py) against each other and against
hand-worked cases, the fixture against its generator, the ABI (symbols, struct layout, C99 header), the formatters and the grammar
of `sc fq-complexity`."""
import ctypes
import gzip
import importlib.util
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG, ROOT
from _complexity_check import (FIELDS, MAX_LEN, NO_FIRST, REC_HEADER, REPORT_FIELDS, SCORE_BINS, STATS_HEADER, STATS_WORDS, complexity_of, masked_text,
                               read_def, read_rows, rec_text, triplets)
from _readstats_check import lines_of

SC = os.path.join(PKG, "sc")
CPLX = os.path.join(GOLDEN, "complexity")
NEW = ("scfq_cplx_buffers", "scfq_cplx_files", "scfq_format_cplx_stats_tsv", "scfq_format_cplx_rec_tsv", "scfq_cplx_error_detail")
COMBOS = [(w, t) for w in (8, 16, 64) for t in (1, 20, 309)]


def run(*args):
    return subprocess.run([SC] + list(args), capture_output=True, text=True, stdin=subprocess.DEVNULL)


def load_generator():
    spec = importlib.util.spec_from_file_location("make_complexity", os.path.join(CPLX, "make_complexity.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def bits(mask):
    return [p for p in range(mask.bit_length()) if mask >> p & 1]


# ---- the fixture ------------------------------------------------------------------------------------------------------------
def test_fixture_is_what_its_generator_writes():
    m = load_generator()
    files, w = m.make_files()
    assert sorted(files) == sorted(n for n in os.listdir(CPLX) if not n.endswith(".py") and n != "__pycache__")
    for name, data in files.items():
        have = open(os.path.join(CPLX, name), "rb").read()
        if name.endswith(".gz"):       # (the compressed bytes are zlib's business)
            have, data = gzip.decompress(have), gzip.decompress(data)
        assert have == data, name
        assert len(have) < 1 << 20
    assert w["reads_in"] == 300 and w["too_long"] == 1 and 0 < w["low_reads"] < w["dropped_reads"] and w["max_masked_pct"] == 30
    assert files["out1.fq"].count(b"\n") == files["out2.fq"].count(b"\n") == 2 * w["reads_out"]
    one = complexity_of(files["interleaved.fq"], interleaved=True, max_masked_pct=30)
    assert one["recs"] == w["recs"] and one["out1_bytes"] == w["out1_bytes"] + w["out2_bytes"] and one["hist"] == w["hist"]
    assert sum(w["hist"]) == w["reads_in"] and w["hist"][SCORE_BINS - 1] == 1


# ---- the checker ------------------------------------------------------------------------------------------------------------
def test_the_two_functions_agree_on_the_fixture():
    """every read of the fixture, by the definition and by the recurrence, at the defaults (the too-long read is no input of either)"""
    seqs = set()
    for name in ("r1.fq", "r2.fq"):
        ls = lines_of(open(os.path.join(CPLX, name), "rb").read())
        seqs |= {s for s in ls[1::4] if len(s) <= MAX_LEN}
    assert len(seqs) > 290
    for s in sorted(seqs):
        assert read_def(s) == read_rows(s), s


def test_the_two_functions_agree_on_planted_reads():
    """300 reads of 0 .. 150 bases with planted units of period 1 .. 6 and with N, every (window, threshold) in turn"""
    rng = np.random.default_rng(20261022)
    masked = 0
    for i in range(300):
        n = int(rng.integers(0, 151))
        s = bytearray(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes())
        if n > 8:
            unit = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 1 + i % 6)].tobytes()
            run_len, at = int(rng.integers(5, 61)), int(rng.integers(0, n))
            s[at:at + run_len] = (unit * 61)[:min(run_len, n - at)]
            if i % 4 == 1:
                s[int(rng.integers(0, n))] = ord("N")
            if i % 7 == 3:
                s[at + 3:at + 4] = b"N"[:max(0, min(1, n - at - 3))]
        s = bytes(s)
        window, threshold = COMBOS[i % len(COMBOS)]
        a, b = read_def(s, window, threshold), read_rows(s, window, threshold)
        assert a == b, (s, window, threshold, a, b)
        masked += a[0] != 0
    assert 60 < masked < 290, masked


def test_hand_computed_anchors():
    # k equal triplets in a row: c = k (k - 1) / 2 over l - 1 = k - 1, so the score is k / 2: high at the defaults from k = 5 on
    assert read_def(b"A" * 6) == read_rows(b"A" * 6) == (0, 20, 0, NO_FIRST)              # 10 * 6 = 20 * 3: equality is not high
    assert read_def(b"A" * 7) == read_rows(b"A" * 7) == (127, 25, 1, 0)                   # 10 * 10 > 20 * 4: all seven bases
    assert read_rows(b"A" * 150)[:2] == ((1 << 150) - 1, 310) and read_rows(b"A" * 150)[3] == 0      # 1891 / 61 = 31
    for n in range(4):
        for s in (b"A" * n, b"ACG"[:n]):
            assert read_def(s) == read_rows(s) == (0, 0, 0, NO_FIRST)
    assert read_rows(b"AAAA") == (0, 10, 0, NO_FIRST) and read_rows(b"ACGT") == (0, 0, 0, NO_FIRST)
    # threshold 25 on seven A: 10 c == T (l - 1) exactly for the whole interval (c = 10, l - 1 = 4), which is not high
    assert read_def(b"A" * 7, 64, 25) == read_rows(b"A" * 7, 64, 25) == (0, 25, 0, NO_FIRST)
    assert read_rows(b"A" * 7, 64, 24)[0] == 127
    # a window of 8 bases holds six triplets: c = 15 over 5, and nothing longer
    assert read_rows(b"A" * 40, 8, 20)[1] == 30 and read_rows(b"A" * 40, 64, 20)[1] == 190
    assert read_rows(b"A" * 40, 64, 310) == (0, 190, 0, NO_FIRST)
    # (AC)n: two codes in turn.  Four triplets ACA CAC ACA CAC: c = 2 over 3; the sub-intervals [0, 2] and [1, 3] have 1 over 2, which is
    # less.  At threshold 5 ([0, 3]: 20 > 15) the interval is perfect and so are [0, 2] and [1, 3] (10 > 10 is false: they are not high)
    s = b"ACACAC"
    assert [t for t in triplets(s)] == [4, 17, 4, 17]
    assert read_def(s, 64, 5) == read_rows(s, 64, 5) == (63, 6, 1, 0)
    s = b"ACACACAC"                               # six triplets, three of each code: c([0, 5]) = 6 over 5; no sub-interval reaches 6 / 5
    whole = read_def(s, 64, 5)
    assert whole == read_rows(s, 64, 5) and whole[0] == 255 and whole[1] == 12
    # a perfect interval with equal-scoring sub-intervals is still perfect: AAAACAAAA has the triplets AAA AAA AAC ACA CAA AAA AAA.  [0, 6]
    # holds four AAA: c = 6 over 6.  [0, 1] and [5, 6] have 1 over 1, the same score; nothing inside scores more ([0, 5]: 3 over 5).  At
    # threshold 9 all three are high (60 > 54, 10 > 9) and perfect; [1, 6] (3 over 5: 30 > 45 is false) is not high
    s = b"AAAACAAAA"
    assert triplets(s) == [0, 0, 1, 4, 16, 0, 0]
    assert read_def(s, 64, 9) == read_rows(s, 64, 9) == (511, 10, 3, 0)
    assert read_def(s, 64, 10) == read_rows(s, 64, 10) == (0, 10, 0, NO_FIRST)               # 60 > 60 is false
    # lower case and N are no bases
    assert read_rows(b"a" * 50) == read_rows(b"N" * 50) == (0, 0, 0, NO_FIRST)
    assert masked_text(b"ACGTNacgt*", 0b1111111111, 1) == b"acgtnacgt*" and masked_text(b"ACGTNacgt*", 0b1111100000, 2) == b"ACGTNNNNNN"
    assert masked_text(b"ACGT", 15, 0) == b"ACGT"


def test_planted_run_inside_random_sequence():
    rng = np.random.default_rng(3)
    for trial in range(5):
        flank = [np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 40)].tobytes() for _ in range(2)]
        if read_rows(flank[0] + b"G" + flank[1])[0]:
            continue
        s = flank[0] + b"AC" * 15 + flank[1]
        got = bits(read_rows(s)[0])
        assert got == list(range(got[0], got[-1] + 1)) and 38 <= got[0] <= 40 and 69 <= got[-1] <= 71, got


# ---- the ABI ----------------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_listed(scfq):
    header = open(os.path.join(ROOT, "include", "sc_fqcount.h")).read()
    debug = open(os.path.join(ROOT, "include", "sc_fqcount_debug.h")).read()
    L = scfq.lib()
    for name in NEW:
        assert name + "(" in header and name in scfq.EXPORTS and hasattr(L, name), name
    assert "scfq_debug_cplx_stages(" in debug and "scfq_debug_cplx_stages" in scfq.EXPORTS and len(scfq.cplx_stages()) == 4
    assert (scfq.SCFQ_CPLX_INTERLEAVED, scfq.SCFQ_CPLX_MASK_NONE, scfq.SCFQ_CPLX_MASK_LOWER, scfq.SCFQ_CPLX_MASK_N) == (1, 0, 1, 2)
    assert (scfq.SCFQ_CPLX_MAX_LEN, scfq.SCFQ_CPLX_SCORE_BINS) == (MAX_LEN, SCORE_BINS)
    for name in ("CplxOpts", "CplxRec", "CplxStats", "cplx_opts", "cplx_resident", "cplx_host", "cplx_files", "format_cplx_stats_tsv", "format_cplx_rec_tsv"):
        assert hasattr(scfq, name), name


def test_struct_layout(scfq, tmp_path):
    S = scfq.CplxStats
    names = tuple(f[0] for f in S._fields_)
    assert names == scfq.CPLX_STATS_FIELDS and len(names) == STATS_WORDS and set(FIELDS) < set(names)
    for i, name in enumerate(names):
        assert getattr(S, name).offset == 8 * i and getattr(S, name).size == 8, name
    assert ctypes.sizeof(S) == 8 * STATS_WORDS and ctypes.sizeof(scfq.CplxOpts) == 40 and ctypes.sizeof(scfq.CplxRec) == 8
    assert np.dtype(scfq.CPLX_REC_DTYPE).itemsize == 8
    src = tmp_path / "t.c"
    offsets = " && ".join("offsetof(scfq_cplx_stats, %s) == %d" % (name, 8 * i) for i, name in enumerate(names))
    src.write_text('#include <stddef.h>\n#include "sc_fqcount.h"\n#include "sc_fqcount_debug.h"\n'
                   "typedef char sizes[sizeof(scfq_cplx_stats) == 232 && sizeof(scfq_cplx_opts) == 40 && sizeof(scfq_cplx_rec) == 8 ? 1 : -1];\n"
                   "typedef char at[" + offsets + " ? 1 : -1];\n"
                   "typedef char consts[SCFQ_CPLX_MAX_LEN == 512 && SCFQ_CPLX_SCORE_BINS == 312 && SCFQ_CPLX_MASK_N == 2 && offsetof(scfq_cplx_opts, reserved) == 28 ? 1 : -1];\n"
                   "int main(void){ scfq_cplx_stats s; scfq_cplx_opts o; scfq_cplx_rec r; uint64_t h[SCFQ_CPLX_SCORE_BINS]; double ms[4]; char b[8];\n"
                   "  s.struct_size = sizeof s; o.struct_size = sizeof o;\n"
                   "  return scfq_cplx_buffers(0, 0, 0, 0, 0, &o, &r, 1, h, 0, 0, 0, 0, 0, &s) + scfq_cplx_files(\"x\", 0, 0, &o, -1, -1, -1, h, &s)\n"
                   "         + scfq_format_cplx_stats_tsv(&s, 0, b, 8) + scfq_format_cplx_rec_tsv(1, &r, 2, b, 8) + scfq_debug_cplx_stages(ms, 4)\n"
                   "         + (scfq_cplx_error_detail() != 0) == 12345; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)])


def test_formatters(scfq):
    assert scfq.format_cplx_stats_tsv(None, header=True) == STATS_HEADER
    s = scfq.CplxStats()
    s.struct_size = ctypes.sizeof(s)
    for i, name in enumerate(REPORT_FIELDS):
        setattr(s, name, 1000 + i)
    assert scfq.format_cplx_stats_tsv(s) == "\t".join(str(1000 + i) for i in range(len(REPORT_FIELDS)))
    s.reads_in = 2 ** 64 - 1
    assert scfq.format_cplx_stats_tsv(s).startswith("18446744073709551615\t1001\t")
    assert scfq.format_cplx_rec_tsv(0, None, 0) == REC_HEADER
    for read, rec, length in ((0, (25, 7, 0, 1), 7), (2 ** 40, (0xFFFF, 0, 0xFFFF, 0), 600), (5, (10, 0, 0xFFFF, 0), 4), (9, (310, 512, 0, 27511), 512)):
        assert scfq.format_cplx_rec_tsv(read, rec, length) == rec_text(read, rec, length)
    assert scfq.format_cplx_rec_tsv(3, (0xFFFF, 0, 0xFFFF, 0), 513) == "3\t513\t-\t0\t-\t0"
    L = scfq.lib()
    r = scfq.CplxRec(12, 3, 4, 1)
    assert L.scfq_format_cplx_rec_tsv(7, ctypes.byref(r), 50, None, 0) == len("7\t50\t12\t3\t4\t1")
    small = ctypes.create_string_buffer(b"#" * 8, 8)
    assert L.scfq_format_cplx_rec_tsv(7, ctypes.byref(r), 50, small, 5) == 13 and small.raw == b"7\t50\0###"
    assert L.scfq_format_cplx_stats_tsv(None, 0, None, 0) == scfq.SCFQ_EARG


def test_argument_checks_come_before_the_device(scfq):
    """none of these needs a device: without one, a call that got past the checks returns SCFQ_EHIP"""
    L = scfq.lib()
    detail = L.scfq_cplx_error_detail
    fastq = b"@h\nACGTACGTAAAAAAAAAA\n+\nIIIIIIIIIIIIIIIIII\n"
    buf = ctypes.create_string_buffer(fastq)

    def call(opts, r2=None, n2=0, out2=None, cap2=0):
        s = scfq.CplxStats()
        s.struct_size = ctypes.sizeof(s)
        return L.scfq_cplx_buffers(buf, len(fastq), r2, n2, 0, ctypes.byref(opts), None, 0, None, None, 0, out2, cap2, 0, ctypes.byref(s))

    for kw, text in ((dict(flags=6), b"unknown flag bits 0x6"), (dict(window=7), b"window 7"), (dict(window=65), b"window 65"), (dict(threshold=0), b"threshold 0"),
                     (dict(threshold=311), b"threshold 311"), (dict(mask=3), b"mask 3"), (dict(max_masked_pct=101), b"max_masked_pct 101"),
                     (dict(reserved=(1, 0, 0)), b"reserved")):
        assert call(scfq.cplx_opts(**kw)) == scfq.SCFQ_EARG and text in detail(), (kw, detail())
    out = ctypes.create_string_buffer(16)
    assert call(scfq.cplx_opts(), out2=out, cap2=16) == scfq.SCFQ_EARG and b"out2" in detail()
    assert call(scfq.cplx_opts(interleaved=True), r2=buf, n2=len(fastq)) == scfq.SCFQ_EARG and b"interleaved" in detail()
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(scfq.ScfqError) as e:
            scfq.cplx_host(fastq)
        assert e.value.rc == scfq.SCFQ_EHIP


# ---- the command ------------------------------------------------------------------------------------------------------------
def test_cli_without_a_device():
    r = run("fq-complexity", "--help")
    assert r.returncode == 0 and r.stderr == "" and "fq-complexity [options] IN.fq > out.fq" in r.stdout
    assert "fq-complexity [options] --out1=PATH --out2=PATH R1.fq R2.fq" in r.stdout and "fq-complexity [options] --interleaved IN.fq > out.fq" in r.stdout
    for opt in ("--window=N", "--threshold=N", "--mask=lower|n|none", "--max-masked-pct=N", "--report", "--stats", "--hist", "--per-read=PATH", "--out=PATH",
                "--out1=PATH", "--out2=PATH", "--interleaved", "-t, --header"):
        assert opt in r.stdout, opt
    assert run("fq-complexity").stdout == r.stdout and run("fq-complexity", "-h").stdout == r.stdout
    assert "fq-complexity" not in run("--help").stdout                                       # listed in its own help only
    r = run("fq-complexity", "does_not_exist.fq")
    assert (r.returncode, r.stderr, r.stdout) == (2, "\x1b[31mError 2: Unable to open file: does_not_exist.fq\x1b[0m\n", "")
    r = run("fq-complexity", "-t")
    assert (r.returncode, r.stderr) == (3, "\x1b[31mError 3: No FASTQ specified\x1b[0m\n")
    r1, r2 = os.path.join(CPLX, "r1.fq"), os.path.join(CPLX, "r2.fq")
    usage = ["--window=7", "--window=65", "--window=", "--window=x", "--threshold=0", "--threshold=311", "--mask=x", "--mask=", "--mask=LOWER", "--max-masked-pct=101",
             "--bogus", "--report=1", "--out=", "--per-read="]
    forms = [(r1, r2, r1), (r1, r2, "--interleaved"), (r1, r2, "--out=x.fq"), (r1, r2, "--out1=x.fq"), (r1, "--out1=x.fq", "--out2=y.fq"), (r1, "--report", "--out=x.fq")]
    for bad in [(u, r1) for u in usage] + forms:
        r = run("fq-complexity", *bad)
        assert r.returncode == 1 and "Error" in r.stderr and "Usage:" in r.stdout, bad
    assert run("fq-complexity", "--window=7", r1).stderr == "\x1b[31mError 1: Error: Bad value for --window: 7\x1b[0m\n"
    assert not os.path.exists("x.fq") and not os.path.exists("y.fq")

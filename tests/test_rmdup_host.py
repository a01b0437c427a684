"""fq-rmdup without a device: the checker (_rmdup_check.py) against an all-pairs statement of the definition and against hand-worked cases,
the fixture against its generator, the ABI (symbols, struct layout, C99 header), the formatters, the argument checks, the grammar of
`sc fq-rmdup`, and what the caller-case inputs of tests/_caller_cases.py hold for tests/test_gpu_rmdup_callers.py."""
import ctypes
import gzip
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import _caller_cases as T
from conftest import GOLDEN, PKG, ROOT
from _rmdup_check import (FIELDS, HASH_FIELDS, HIST_BINS, REC_HEADER, REPORT_FIELDS, STATS_HEADER, STATS_WORDS, check_identities, classes_by_pairs, classes_of,
                          hist_text, key_of, pct_text, per_read_text, rec_text, rmdup_of, stats_text)

SC = os.path.join(PKG, "sc")
RMDUP = os.path.join(GOLDEN, "rmdup")
NEW = ("scfq_rmdup_buffers", "scfq_rmdup_files", "scfq_format_rmdup_stats_tsv", "scfq_format_rmdup_rec_tsv", "scfq_rmdup_error_detail")
CALLER_OPTS = dict(prefix=10, swapped=True)


def run(*args):
    return subprocess.run([SC] + list(args), capture_output=True, text=True, stdin=subprocess.DEVNULL)


def load_generator():
    spec = importlib.util.spec_from_file_location("make_rmdup", os.path.join(RMDUP, "make_rmdup.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def fq(seqs, name="r"):
    return b"".join(b"@%s%d\n%s\n+\n%s\n" % (name.encode(), i, s, b"I" * len(s)) for i, s in enumerate(seqs))


# ---- the checker ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix", (0, 1, 3))
@pytest.mark.parametrize("form", ("single", "paired", "swapped"))
def test_the_dictionary_agrees_with_all_pairs(form, prefix):
    """200 random units over the alphabet AC with texts of 0 .. 6 bytes: classes abound"""
    rng = np.random.default_rng([20261023, prefix, len(form)])
    mates = 1 if form == "single" else 2
    units = [tuple(bytes(rng.choice(np.frombuffer(b"AC", np.uint8), int(rng.integers(0, 7))).tobytes()) for _ in range(mates)) for _ in range(200)]
    keys = [tuple(key_of(S, prefix) for S in u) for u in units]
    a, b = classes_of(keys, form == "swapped"), classes_by_pairs(keys, form == "swapped")
    assert a == b
    classes = sum(1 for _, c in a if c)
    assert 1 < classes < 200 and max(c for _, c in a) >= 3 and sum(c for _, c in a) == 200
    if prefix == 1:
        assert classes <= (3 if mates == 1 else 9)                      # the keys are "", "A" and "C"
    # the whole restatement on the same units: the table is this one
    if mates == 1:
        w = rmdup_of(fq([u[0] for u in units]), prefix=prefix)
    else:
        w = rmdup_of(fq([u[0] for u in units]), fq([u[1] for u in units]), prefix=prefix, swapped=form == "swapped")
    assert w["recs"] == a
    check_identities(w, w["hist"], w["recs"])


def test_hand_computed_anchors():
    # single-end: the first of equal texts is kept; a text that is a proper prefix of another is another key; the empty text is a key
    w = rmdup_of(fq([b"ACGT", b"ACG", b"ACGT", b"", b"acgt", b"", b"ACGN", b"ACGT"]))
    assert w["recs"] == [(0, 3), (1, 1), (0, 0), (3, 2), (4, 1), (3, 0), (6, 1), (0, 0)]
    assert (w["units_in"], w["units_out"], w["duplicate_units"], w["duplicated_classes"], w["max_copies"]) == (8, 5, 3, 2, 3)
    assert (w["bases_in"], w["bases_out"]) == (23, 15) and w["hist"][1:4] == [3, 1, 1] and sum(w["hist"]) == 5
    assert w["out1"] == b"@r0\nACGT\n+\nIIII\n@r1\nACG\n+\nIII\n@r3\n\n+\n\n@r4\nacgt\n+\nIIII\n@r6\nACGN\n+\nIIII\n"
    # prefix 3: ACGT, ACG, ACGN are one key (ACG with length 3); acgt is not; prefix 2 makes no difference to the empty texts
    w = rmdup_of(fq([b"ACGT", b"ACG", b"ACGT", b"", b"acgt", b"", b"ACGN", b"ACGT"]), prefix=3)
    assert w["recs"] == [(0, 5), (0, 0), (0, 0), (3, 2), (4, 1), (3, 0), (0, 0), (0, 0)] and w["prefix"] == 3
    # a text shorter than the prefix keeps its own length: AC is not ACG
    assert rmdup_of(fq([b"ACG", b"AC", b"ACGG"]), prefix=3)["recs"] == [(0, 2), (1, 1), (0, 0)]
    # pairs: both mates have to agree; exchanged mates agree under the flag only; (a, a) and (b, b) are two classes either way
    a, b = b"AAAA", b"CCCC"
    m1, m2 = fq([a, b, a, b, a, a]), fq([b, a, a, b, b, b"GGGG"])
    assert rmdup_of(m1, m2)["recs"] == [(0, 2), (1, 1), (2, 1), (3, 1), (0, 0), (5, 1)]
    w = rmdup_of(m1, m2, swapped=True)
    assert w["recs"] == [(0, 3), (0, 0), (2, 1), (3, 1), (0, 0), (5, 1)] and w["flags"] == 2
    assert w["out1"] == b"@r0\nAAAA\n+\nIIII\n@r2\nAAAA\n+\nIIII\n@r3\nCCCC\n+\nIIII\n@r5\nAAAA\n+\nIIII\n"
    assert w["out2"] == b"@r0\nCCCC\n+\nIIII\n@r2\nAAAA\n+\nIIII\n@r3\nCCCC\n+\nIIII\n@r5\nGGGG\n+\nIIII\n"
    assert (w["reads_in"], w["reads_out"], w["pairs"], w["unpaired"], w["bases_in"], w["bases_out"]) == (12, 8, 6, 0, 48, 32)
    # interleaved: the same pairs, one output; an odd last record is unpaired and goes nowhere
    il = b"".join(x + y for x, y in zip((b"@" + r for r in m1.split(b"@")[1:]), (b"@" + r for r in m2.split(b"@")[1:]))) + b"@odd\nAC\n+\nII\n"
    v = rmdup_of(il, interleaved=True, swapped=True)
    assert v["recs"] == w["recs"] and v["unpaired"] == 1 and v["out1_bytes"] == w["out1_bytes"] + w["out2_bytes"] and v["out2"] == b""
    # reads1 != reads2: the pairs are the shorter file's
    v = rmdup_of(m1, fq([b, a, a]))
    assert (v["pairs"], v["unpaired"], v["units_in"]) == (3, 3, 3) and v["recs"] == [(0, 1), (1, 1), (2, 1)]
    # CR LF and a last record without newline: the texts are compared, the echo has '\n' alone
    v = rmdup_of(b"@x\r\nACGT\r\n+\r\nIIII\r\n@y\nACGT\n+\nIIII")
    assert v["recs"] == [(0, 2), (0, 0)] and v["out1"] == b"@x\nACGT\n+\nIIII\n"
    # a truncated last record has the lines it has; one without a sequence line has the empty text
    v = rmdup_of(b"@x\n\n+\n\n@y")
    assert v["recs"] == [(0, 2), (0, 0)] and v["lines1"] == 5
    assert rmdup_of(b"")["units_in"] == 0 and rmdup_of(b"")["max_copies"] == 0 and sum(rmdup_of(b"")["hist"]) == 0
    # classes of 1024 and more share the last bin
    w = rmdup_of(fq([b"A"] * 1023 + [b"C"] * 1024 + [b"G"] * 1500))
    assert (w["hist"][1023], w["hist"][1024], sum(w["hist"])) == (1, 2, 3) and hist_text(w) == "1023\t1\t1023\n1024+\t2\t2524\n"
    assert [pct_text(d, u) for d, u in ((0, 0), (1, 3), (3, 3), (2, 3), (1, 10000), (1, 10001), (0, 5))] == ["0.00", "33.33", "100.00", "66.66", "0.01", "0.00", "0.00"]


# ---- the fixture ------------------------------------------------------------------------------------------------------------
def test_fixture_is_what_its_generator_writes():
    m = load_generator()
    files, w = m.make_files()
    assert sorted(files) == sorted(n for n in os.listdir(RMDUP) if not n.endswith(".py") and n != "__pycache__")
    for name, data in files.items():
        have = open(os.path.join(RMDUP, name), "rb").read()
        if name.endswith(".gz"):       # (the compressed bytes are zlib's business)
            have, data = gzip.decompress(have), gzip.decompress(data)
        assert have == data, name
        assert len(have) < 1 << 20
    check_identities(w, w["hist"], w["recs"])
    assert (w["units_in"], w["pairs"], w["prefix"], w["flags"], w["max_copies"]) == (150, 150, 50, 2, 40) and w["hist"][40] == 1
    assert files["out1.fq"].count(b"\n") == files["out2.fq"].count(b"\n") == 4 * w["units_out"]
    r1, r2 = files["r1.fq"], files["r2.fq"]
    assert not r1.endswith(b"\n") and not r2.endswith(b"\n") and b"\r" not in r1 + r2
    one = rmdup_of(files["interleaved.fq"], interleaved=True, prefix=50, swapped=True)
    assert one["recs"] == w["recs"] and one["out1_bytes"] == w["out1_bytes"] + w["out2_bytes"] and one["hist"] == w["hist"]


def test_fixture_holds_what_it_plants():
    m = load_generator()
    files, w = m.make_files()
    r1, r2 = files["r1.fq"], files["r2.fq"]
    recs = {k: rmdup_of(r1, r2, **kw)["recs"] for k, kw in dict(plain={}, swapped=dict(swapped=True), prefix=dict(prefix=50), both=dict(prefix=50, swapped=True),
                                                                short=dict(prefix=30)).items()}
    assert recs["both"] == w["recs"]
    assert len(m.BIG) == 40 and m.PAIRS == 150
    for p in range(m.PAIRS):
        got = {k: v[p][0] for k, v in recs.items()}
        r = p % 14 if p < m.RULES_BELOW else -1
        if p in m.BIG:
            assert set(got.values()) == {m.BIG[0]} and recs["plain"][m.BIG[0]][1] == 40, p
        elif p in m.ALL_G:
            assert set(got.values()) == {m.ALL_G[0]} and recs["plain"][m.ALL_G[0]][1] == len(m.ALL_G), p
        elif r == 2:
            assert set(got.values()) == {p - 2}, p                                            # exact duplicates, whatever the options
        elif r == 9:
            assert (got["plain"], got["prefix"], got["swapped"], got["both"]) == (p, p, p - 2, p - 2), p
        elif r in (3, 10):
            assert set(got.values()) == {p}, p                                                # one mate alone never suffices
        elif r == 4:
            assert (got["plain"], got["swapped"], got["prefix"], got["both"], got["short"]) == (p, p, p - 4, p - 4, p - 4), p
        elif r == 11:
            assert (got["plain"], got["prefix"], got["both"], got["short"]) == (p, p, p, p - 4), p       # a proper prefix: equal once both are cut to it
    one = rmdup_of(r1, prefix=50)                                                             # mate 1 alone: more duplicates than pairs have
    assert one["duplicate_units"] > w["duplicate_units"]


# ---- the ABI ----------------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_listed(scfq):
    header = open(os.path.join(ROOT, "include", "sc_fqcount.h")).read()
    debug = open(os.path.join(ROOT, "include", "sc_fqcount_debug.h")).read()
    L = scfq.lib()
    for name in NEW:
        assert name + "(" in header and name in scfq.EXPORTS and hasattr(L, name), name
    assert "scfq_debug_rmdup_stages(" in debug and "scfq_debug_rmdup_stages" in scfq.EXPORTS and len(scfq.rmdup_stages()) == 7
    assert (scfq.SCFQ_RMDUP_INTERLEAVED, scfq.SCFQ_RMDUP_SWAPPED, scfq.SCFQ_RMDUP_HIST_BINS, scfq.SCFQ_RMDUP_MAX_PREFIX) == (1, 2, HIST_BINS, 65535)
    for name in ("RmdupOpts", "RmdupRec", "RmdupStats", "rmdup_opts", "rmdup_resident", "rmdup_host", "rmdup_files", "format_rmdup_stats_tsv", "format_rmdup_rec_tsv"):
        assert hasattr(scfq, name), name
    assert not hasattr(scfq, "rmdup_device")


def test_struct_layout(scfq, tmp_path):
    S = scfq.RmdupStats
    names = tuple(f[0] for f in S._fields_)
    assert names == scfq.RMDUP_STATS_FIELDS and len(names) == STATS_WORDS and set(FIELDS) | set(HASH_FIELDS) | {"struct_size", "abi_version"} == set(names)
    for i, name in enumerate(names):
        assert getattr(S, name).offset == 8 * i and getattr(S, name).size == 8, name
    assert ctypes.sizeof(S) == 8 * STATS_WORDS and ctypes.sizeof(scfq.RmdupOpts) == 32 and ctypes.sizeof(scfq.RmdupRec) == 8
    assert np.dtype(scfq.RMDUP_REC_DTYPE).itemsize == 8
    src = tmp_path / "t.c"
    offsets = " && ".join("offsetof(scfq_rmdup_stats, %s) == %d" % (name, 8 * i) for i, name in enumerate(names))
    src.write_text('#include <stddef.h>\n#include "sc_fqcount.h"\n#include "sc_fqcount_debug.h"\n'
                   "typedef char sizes[sizeof(scfq_rmdup_stats) == 208 && sizeof(scfq_rmdup_opts) == 32 && sizeof(scfq_rmdup_rec) == 8 ? 1 : -1];\n"
                   "typedef char at[" + offsets + " ? 1 : -1];\n"
                   "typedef char consts[SCFQ_RMDUP_HIST_BINS == 1025 && SCFQ_RMDUP_SWAPPED == 2 && SCFQ_RMDUP_INTERLEAVED == 1 && SCFQ_RMDUP_MAX_PREFIX == 65535\n"
                   "                    && offsetof(scfq_rmdup_opts, prefix) == 12 && offsetof(scfq_rmdup_opts, hash_bits) == 16 && offsetof(scfq_rmdup_opts, reserved) == 20\n"
                   "                    && offsetof(scfq_rmdup_rec, copies) == 4 ? 1 : -1];\n"
                   "int main(void){ scfq_rmdup_stats s; scfq_rmdup_opts o; scfq_rmdup_rec r; uint64_t h[SCFQ_RMDUP_HIST_BINS]; double ms[7]; char b[8];\n"
                   "  s.struct_size = sizeof s; o.struct_size = sizeof o;\n"
                   "  return scfq_rmdup_buffers(0, 0, 0, 0, 0, &o, &r, 1, h, 0, 0, 0, 0, 0, &s) + scfq_rmdup_files(\"x\", 0, &o, 0, -1, -1, -1, h, &s)\n"
                   "         + scfq_format_rmdup_stats_tsv(&s, 0, b, 8) + scfq_format_rmdup_rec_tsv(1, &r, b, 8) + scfq_debug_rmdup_stages(ms, 7)\n"
                   "         + (scfq_rmdup_error_detail() != 0) == 12345; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)])


def test_formatters(scfq):
    assert scfq.format_rmdup_stats_tsv(None, header=True) == STATS_HEADER

    def stats(**kw):
        s = scfq.RmdupStats()
        s.struct_size = ctypes.sizeof(s)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    plain = [n for n in REPORT_FIELDS if n != "duplicate_pct"]
    w = {name: 1000 + i for i, name in enumerate(plain)}
    assert scfq.format_rmdup_stats_tsv(stats(**w)) == stats_text(w) and "\t100.20\t" in stats_text(w)      # (1002 of 1000: the function divides what it is given)
    for dup, units, text in ((0, 0, "0.00"), (1, 3, "33.33"), (3, 3, "100.00"), (2, 3, "66.66"), (1, 10001, "0.00"), (2 ** 62, 2 ** 63, "50.00"),
                             (2 ** 64 - 2, 2 ** 64 - 1, "99.99")):
        row = scfq.format_rmdup_stats_tsv(stats(units_in=units, duplicate_units=dup, units_out=units - dup)).split("\t")
        assert row[:4] == [str(units), str(units - dup), str(dup), text] and text == pct_text(dup, units), (dup, units, row)
    assert scfq.format_rmdup_rec_tsv(0, None) == REC_HEADER
    for unit, rec in ((0, (0, 1)), (2 ** 40, (2 ** 32 - 1, 0)), (5, (3, 0)), (9, (9, 2 ** 31))):
        assert scfq.format_rmdup_rec_tsv(unit, rec) == rec_text(unit, rec)
    L = scfq.lib()
    r = scfq.RmdupRec(12, 3)
    assert L.scfq_format_rmdup_rec_tsv(7, ctypes.byref(r), None, 0) == len("7\t12\t3")
    small = ctypes.create_string_buffer(b"#" * 8, 8)
    assert L.scfq_format_rmdup_rec_tsv(7, ctypes.byref(r), small, 5) == 6 and small.raw == b"7\t12\0###"
    assert L.scfq_format_rmdup_stats_tsv(None, 0, None, 0) == scfq.SCFQ_EARG
    w = rmdup_of(fq([b"A", b"A", b"C"]))
    assert per_read_text(w, header=True) == "unit\trep\tcopies\n0\t0\t2\n1\t0\t0\n2\t2\t1\n"


def test_argument_checks_come_before_the_device(scfq):
    """none of these needs a device: without one, a call that got past the checks returns SCFQ_EHIP"""
    L = scfq.lib()
    detail = L.scfq_rmdup_error_detail
    fastq = b"@h\nACGTACGTAAAAAAAAAA\n+\nIIIIIIIIIIIIIIIIII\n"
    buf = ctypes.create_string_buffer(fastq)

    def call(opts, r2=None, n2=0, out2=None, cap2=0, stats_size=None, recs_cap=0):
        s = scfq.RmdupStats()
        s.struct_size = ctypes.sizeof(s) if stats_size is None else stats_size
        return L.scfq_rmdup_buffers(buf, len(fastq), r2, n2, 0, ctypes.byref(opts), None, recs_cap, None, None, 0, out2, cap2, 0, ctypes.byref(s))

    for kw, text in ((dict(flags=4), b"unknown flag bits 0x4"), (dict(flags=0x12), b"unknown flag bits 0x10"), (dict(prefix=65536), b"prefix 65536"),
                     (dict(hash_bits=65), b"hash_bits 65"), (dict(reserved=(0, 0, 7)), b"reserved"), (dict(swapped=True), b"single-end")):
        assert call(scfq.rmdup_opts(**kw)) == scfq.SCFQ_EARG and text in detail(), (kw, detail())
    out = ctypes.create_string_buffer(16)
    assert call(scfq.rmdup_opts(), out2=out, cap2=16) == scfq.SCFQ_EARG and b"out2" in detail()
    assert call(scfq.rmdup_opts(interleaved=True), r2=buf, n2=len(fastq)) == scfq.SCFQ_EARG and b"interleaved" in detail()
    # without text: sizes that are not the structs', a capacity without memory
    assert call(scfq.rmdup_opts(), stats_size=200) == scfq.SCFQ_EARG and detail() == b""
    bad = scfq.rmdup_opts()
    bad.struct_size = 40
    assert call(bad) == scfq.SCFQ_EARG and detail() == b""
    assert call(scfq.rmdup_opts(), recs_cap=4) == scfq.SCFQ_EARG and detail() == b""
    assert call(scfq.rmdup_opts(), cap2=4) == scfq.SCFQ_EARG and detail() == b""
    s = scfq.RmdupStats()
    s.struct_size = ctypes.sizeof(s)
    o = scfq.rmdup_opts(swapped=True)
    assert L.scfq_rmdup_files(b"x.fq", None, ctypes.byref(o), None, -1, -1, -1, None, ctypes.byref(s)) == scfq.SCFQ_EARG and b"single-end" in detail()
    assert L.scfq_rmdup_files(None, None, None, None, -1, -1, -1, None, ctypes.byref(s)) == scfq.SCFQ_EARG
    o = scfq.rmdup_opts()
    assert L.scfq_rmdup_files(b"x.fq", None, ctypes.byref(o), None, -1, 5, -1, None, ctypes.byref(s)) == scfq.SCFQ_EARG and b"out2" in detail()
    import torch
    if not torch.cuda.is_available():
        for opts in (None, scfq.rmdup_opts(prefix=65535, hash_bits=64), scfq.rmdup_opts(hash_bits=1)):
            with pytest.raises(scfq.ScfqError) as e:
                scfq.rmdup_host(fastq, opts=opts)
            assert e.value.rc == scfq.SCFQ_EHIP
        with pytest.raises(scfq.ScfqError) as e:
            scfq.rmdup_host(fastq, fastq, opts=scfq.rmdup_opts(swapped=True))
        assert e.value.rc == scfq.SCFQ_EHIP


# ---- the command ------------------------------------------------------------------------------------------------------------
def test_cli_without_a_device(tmp_path):
    r = run("fq-rmdup", "--help")
    assert r.returncode == 0 and r.stderr == "" and "fq-rmdup [options] IN.fq > out.fq" in r.stdout
    assert "fq-rmdup [options] --out1=PATH --out2=PATH R1.fq R2.fq" in r.stdout and "fq-rmdup [options] --interleaved IN.fq > out.fq" in r.stdout
    for opt in ("--prefix=N", "--swapped", "--report", "--stats", "--hist", "--per-read=PATH", "--out=PATH", "--out1=PATH", "--out2=PATH", "--interleaved",
                "-t, --header"):
        assert opt in r.stdout, opt
    assert run("fq-rmdup").stdout == r.stdout and run("fq-rmdup", "-h").stdout == r.stdout
    assert "fq-rmdup" not in run("--help").stdout                                            # listed in its own help only
    r = run("fq-rmdup", "does_not_exist.fq")
    assert (r.returncode, r.stderr, r.stdout) == (2, "\x1b[31mError 2: Unable to open file: does_not_exist.fq\x1b[0m\n", "")
    r = run("fq-rmdup", "-t")
    assert (r.returncode, r.stderr) == (3, "\x1b[31mError 3: No FASTQ specified\x1b[0m\n")
    r1, r2 = os.path.join(RMDUP, "r1.fq"), os.path.join(RMDUP, "r2.fq")
    usage = ["--prefix=65536", "--prefix=", "--prefix=x", "--prefix=-1", "--swapped", "--swapped=1", "--bogus", "--report=1", "--out=", "--per-read=", "--hash-bits=8"]
    forms = [(r1, r2, r1), (r1, r2, "--interleaved"), (r1, r2, "--out=x.fq"), (r1, r2, "--out1=x.fq"), (r1, "--out1=x.fq", "--out2=y.fq"), (r1, "--report", "--out=x.fq")]
    for bad in [(u, r1) for u in usage] + forms:
        r = subprocess.run([SC, "fq-rmdup"] + list(bad), capture_output=True, text=True, stdin=subprocess.DEVNULL, cwd=str(tmp_path))
        assert r.returncode == 1 and "Error" in r.stderr and "Usage:" in r.stdout, bad
    assert run("fq-rmdup", "--prefix=65536", r1).stderr == "\x1b[31mError 1: Error: Bad value for --prefix: 65536\x1b[0m\n"
    assert os.listdir(str(tmp_path)) == []


# ---- the caller cases -------------------------------------------------------------------------------------------------------
class Shape(T.TwoOutputs):
    """the inputs of tests/test_gpu_rmdup_callers.py's row, without a device"""
    rec = (8, "units_in")

    def wanted(self, inputs, base=None):
        a1, a2 = self.texts(inputs)
        return rmdup_of(a1.tobytes(), None if a2 is None else a2.tobytes(), interleaved=self.interleaved, **CALLER_OPTS)


@pytest.mark.parametrize("kind", ("pair", "interleaved"))
def test_caller_case_inputs_have_duplicates(kind):
    """with prefix=10 and swapped pairs every worker seed but the single-pair one has duplicates, and fewer than half of its units: 11 .. 21 among
    300 .. 377 pairs.  The short-lines seed, whose 2000 records of 8 bytes hold texts of a byte or two, has 2010 among 2307: there the bound is
    units_in.  The decoy differs from the real input in every part that is compared"""
    job = Shape("rmdup_resident " + kind, kind=kind)
    for seed in T.WORKER_SEEDS:
        w, other = job.wanted(job.make(seed)), job.wanted(job.make(seed, True))
        check_identities(w, w["hist"], w["recs"])
        if seed == T.SINGLE:
            assert (w["units_in"], w["duplicate_units"]) == (1, 0)
        elif seed == T.SHORT_LINES:
            assert 0 < w["units_in"] // 2 < w["duplicate_units"] < w["units_in"], (seed, w["duplicate_units"], w["units_in"])
        else:
            assert 0 < w["duplicate_units"] < w["units_in"] // 2 and w["duplicated_classes"] > 0, (seed, w["duplicate_units"], w["units_in"])
        names = ("recs", "out1", "hist") + (() if kind == "interleaved" else ("out2",))
        assert all(w[n] != other[n] for n in names), seed
        assert {k: w[k] for k in FIELDS} != {k: other[k] for k in FIELDS}

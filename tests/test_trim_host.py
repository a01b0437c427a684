"""fq-trim without a device: the ABI (symbols, struct layout, C99 header), argument checks that return before the device is touched, the
stats formatter, the CLI's help / error behaviour, hand-worked cases of every rule of the contract, the two checkers of _trim_check.py
against each other, the identities, and the golden outputs of the trim fixture."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG, ROOT
from _insert_size_check import paired_block, planted
from _merge_check import with_random_qualities
from _trim_check import DEFAULT_PROBES, FIELDS, PARAM_FIELDS, STATS_HEADER, check_identities, same, stats_text, trim_of, trim_of_np

SC = os.path.join(PKG, "sc")
TRIM = os.path.join(GOLDEN, "trim")
NEW = ("scfq_trim_buffers", "scfq_trim_files", "scfq_format_trim_stats_tsv", "scfq_trim_error_detail")
SCALARS = tuple(f for f in FIELDS if f != "adapter_reads")
FASTQ = b"@h\nACGTN\n+\nIIIII\n"
FIXTURE = dict(poly_g=10, window_quality=20)       # tests/golden/trim/make_trim.py's PARAMS
UNIVERSAL = DEFAULT_PROBES[0]                      # AGATCGGAAGAG
BODY = b"ACCA" * 10                                # 40 bases no probe is near to


def run(*args):
    return subprocess.run([SC] + list(args), capture_output=True, text=True, stdin=subprocess.DEVNULL)


def as_array(data):
    return None if data is None else np.frombuffer(bytes(data), dtype=np.uint8)


def both(data1, data2=None, **kw):
    """the plain checker's result, after the numpy one has agreed with it and the identities hold"""
    w = trim_of(data1, data2, **kw)
    v = trim_of_np(as_array(data1), as_array(data2), **kw)
    assert same(w, v), [k for k in w if w[k] != v.get(k)]
    check_identities(w)
    return w


def one(seq, qual=None, **kw):
    """a single read through the checkers: (the record that comes out or b"", the result)"""
    qual = b"I" * len(seq) if qual is None else qual
    w = both(b"@r\n" + seq + b"\n+\n" + qual + b"\n", **kw)
    return w["out1"], w


def test_symbols_declared_exported_and_listed(scfq):
    header = open(os.path.join(ROOT, "include", "sc_fqcount.h")).read()
    debug = open(os.path.join(ROOT, "include", "sc_fqcount_debug.h")).read()
    L = scfq.lib()
    for name in NEW:
        assert name + "(" in header and name in scfq.EXPORTS and hasattr(L, name), name
    assert "scfq_debug_trim_stages(" in debug and "scfq_debug_trim_stages" in scfq.EXPORTS and hasattr(L, "scfq_debug_trim_stages")
    assert len(scfq.trim_stages()) == 4
    assert (scfq.SCFQ_TRIM_INTERLEAVED, scfq.SCFQ_TRIM_NO_OVERLAP, scfq.SCFQ_TRIM_NO_ADAPTERS) == (1, 2, 4)
    for name in ("SCFQ_TRIM_INTERLEAVED", "SCFQ_TRIM_NO_OVERLAP", "SCFQ_TRIM_NO_ADAPTERS", "SCFQ_TRIM_MAX_LEN", "SCFQ_TRIM_MAX_PROBES"):
        assert name in header, name
    for name in ("TrimOpts", "TrimStats", "trim_opts", "trim_device", "trim_host", "trim_file", "format_trim_stats_tsv", "trim_stages"):
        assert hasattr(scfq, name), name
    # the default set: the built-in adapters without the entries named poly*
    name, seq = ctypes.c_char_p(), ctypes.c_char_p()
    L.scfq_adapters_default.argtypes = [ctypes.c_uint32, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_char_p)]
    left = []
    for i in range(L.scfq_adapters_default(0, None, None)):
        L.scfq_adapters_default(i, ctypes.byref(name), ctypes.byref(seq))
        if not name.value.startswith(b"poly"):
            left.append(seq.value)
    assert tuple(left) == DEFAULT_PROBES and len(left) == 5


def test_struct_layout(scfq):
    O, S = scfq.TrimOpts, scfq.TrimStats
    assert ctypes.sizeof(O) == 128
    assert [(n, getattr(O, n).offset) for n, _ in O._fields_] == [("struct_size", 0)] + [(n, 8 + 4 * k) for k, n in enumerate(PARAM_FIELDS)] + \
        [("reserved", 56), ("probes", 64)]
    assert tuple(f[0] for f in S._fields_) == ("struct_size", "abi_version") + FIELDS
    at = 0
    for name, _ in S._fields_:
        size = 64 if name == "adapter_reads" else 8
        assert getattr(S, name).offset == at and getattr(S, name).size == size, name
        at += size
    assert ctypes.sizeof(S) == at == 8 * 49


def test_header_is_c99_and_sizes_agree(tmp_path):
    src = tmp_path / "t.c"
    names, at = [], 16
    for name in FIELDS:
        names.append("offsetof(scfq_trim_stats, %s) == %d" % (name, at))
        at += 64 if name == "adapter_reads" else 8
    offsets = " && ".join(names) + " && offsetof(scfq_trim_opts, flags) == 8 && offsetof(scfq_trim_opts, n_probes) == 52"
    offsets += " && offsetof(scfq_trim_opts, reserved) == 56 && offsetof(scfq_trim_opts, probes) == 64"
    src.write_text('#include <stddef.h>\n#include "sc_fqcount.h"\n#include "sc_fqcount_debug.h"\n'
                   "typedef char stats_size[sizeof(scfq_trim_stats) == 8 * 49 ? 1 : -1];\n"
                   "typedef char opt_size[sizeof(scfq_trim_opts) == 128 ? 1 : -1];\n"
                   "typedef char at[" + offsets + " ? 1 : -1];\n"
                   "typedef char consts[SCFQ_TRIM_INTERLEAVED == 1 && SCFQ_TRIM_NO_OVERLAP == 2 && SCFQ_TRIM_NO_ADAPTERS == 4 && SCFQ_TRIM_MAX_LEN == 512"
                   " && SCFQ_TRIM_MAX_PROBES == 8 ? 1 : -1];\n"
                   "int main(void){ scfq_trim_stats s; scfq_trim_opts o; double ms[4]; char out[8];\n"
                   "  s.struct_size = sizeof s; o.struct_size = sizeof o; o.flags = 0; o.n_probes = 1; o.probes[0] = \"ACGT\"; o.reserved[0] = 0;\n"
                   "  return scfq_trim_buffers(0, 0, 0, 0, 0, &o, out, 8, 0, 0, 0, &s) + scfq_format_trim_stats_tsv(&s, 0, 0)\n"
                   "         + scfq_trim_files(\"x\", \"y\", 0, &o, 1, -1, &s) + scfq_debug_trim_stages(ms, 4)\n"
                   "         + (scfq_trim_error_detail() != 0) == 12345; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-fsyntax-only", str(src)])


def test_argument_checks(scfq):
    L = scfq.lib()
    s = scfq._new_trim_stats()
    buf = ctypes.create_string_buffer(FASTQ)
    n = len(FASTQ)
    out = ctypes.create_string_buffer(64)
    ok = ctypes.byref(s)
    detail = L.scfq_trim_error_detail
    B, F = L.scfq_trim_buffers, L.scfq_trim_files
    none = (None, 0, None, 0, 0)
    # without text
    assert B(buf, n, buf, n, 0, None, *none, None) == scfq.SCFQ_EARG                                    # NULL stats
    bad = scfq.TrimStats()                                                                            # struct_size not set
    assert B(buf, n, buf, n, 0, None, *none, ctypes.byref(bad)) == scfq.SCFQ_EARG
    bad.struct_size = ctypes.sizeof(scfq.TrimStats) - 8
    assert B(buf, n, buf, n, 0, None, *none, ctypes.byref(bad)) == scfq.SCFQ_EARG
    assert B(None, n, buf, n, 0, None, *none, ok) == scfq.SCFQ_EARG                                     # NULL pointer with n > 0
    assert B(buf, n, None, n, 0, None, *none, ok) == scfq.SCFQ_EARG
    for k in range(2):                                                                                # NULL output with a capacity
        caps = [None, 0, None, 0, 0]
        caps[2 * k + 1] = 8
        assert B(buf, n, buf, n, 0, None, *caps, ok) == scfq.SCFQ_EARG, k
    small = scfq.trim_opts()
    small.struct_size -= 4
    assert B(buf, n, buf, n, 0, ctypes.byref(small), *none, ok) == scfq.SCFQ_EARG                       # wrong size of the options
    assert F(None, b"y.fq", None, None, -1, -1, ok) == scfq.SCFQ_EARG
    assert F(b"x.fq", b"y.fq", None, None, -1, -1, ctypes.byref(bad)) == scfq.SCFQ_EARG
    assert F(b"x.fq", b"y.fq", None, ctypes.byref(small), -1, -1, ok) == scfq.SCFQ_EARG
    assert detail() == b""

    def refused(opts, *texts):
        for call in (lambda: B(buf, n, buf, n, 0, ctypes.byref(opts), *none, ok), lambda: F(b"x.fq", b"y.fq", None, ctypes.byref(opts), -1, -1, ok)):
            assert call() == scfq.SCFQ_EARG, texts
            for t in texts:
                assert t in detail(), (t, detail())

    refused(scfq.trim_opts(min_overlap=0), b"min_overlap 0", b"1 .. 512")
    refused(scfq.trim_opts(min_overlap=513), b"min_overlap 513")
    refused(scfq.trim_opts(max_mismatches=65536), b"max_mismatches 65536")
    refused(scfq.trim_opts(max_mismatch_pct=101), b"max_mismatch_pct 101")
    refused(scfq.trim_opts(min_adapter_overlap=0), b"min_adapter_overlap 0", b"1 .. 32")
    refused(scfq.trim_opts(min_adapter_overlap=33), b"min_adapter_overlap 33")
    refused(scfq.trim_opts(adapter_mismatch_pct=101), b"adapter_mismatch_pct 101", b"0 .. 100")
    refused(scfq.trim_opts(poly_g=513), b"poly_g 513", b"0 .. 512")
    refused(scfq.trim_opts(window=0), b"window 0", b"1 .. 32")
    refused(scfq.trim_opts(window=33), b"window 33")
    refused(scfq.trim_opts(window_quality=94), b"window_quality 94", b"0 .. 93")
    refused(scfq.trim_opts(min_length=513), b"min_length 513", b"0 .. 512")
    for q0 in (0, 32, 34, 63, 65, 126):
        refused(scfq.trim_opts(phred_offset=q0), b"phred_offset %d" % q0, b"33 or 64")
    for k in range(2):
        o = scfq.trim_opts()
        o.reserved[k] = 7
        refused(o, b"reserved", b"7")
    o = scfq.trim_opts()
    o.flags = 24
    refused(o, b"unknown flag bits 0x18")
    refused(scfq.trim_opts(interleaved=True), b"interleaved", b"no second")                             # the flag with two inputs
    # the probes
    o = scfq.trim_opts()
    o.n_probes = 9
    refused(o, b"9 probes")
    o = scfq.trim_opts(probes=[b"ACGT"])
    o.flags |= scfq.SCFQ_TRIM_NO_ADAPTERS
    refused(o, b"SCFQ_TRIM_NO_ADAPTERS")
    o = scfq.trim_opts(probes=[b"ACGT", b"AC"])
    o.probes[1] = None
    refused(o, b"probe 1 is NULL")
    refused(scfq.trim_opts(probes=[b""]), b"probe 0 is empty")
    refused(scfq.trim_opts(probes=[b"A" * 33]), b"probe 0 is longer than 32")
    for text in (b"ACGN", b"acgt", b"ACG T"):
        refused(scfq.trim_opts(probes=[b"ACGT", text]), b"probe 1 holds the byte", b"only A C G T")
    # a second output without a second input; the flag with a second buffer
    il = scfq.trim_opts(interleaved=True)
    assert B(buf, n, None, 5, 0, ctypes.byref(il), *none, ok) == scfq.SCFQ_EARG
    for opts in (ctypes.byref(il), None):
        assert B(buf, n, None, 0, 0, opts, None, 0, out, 64, 0, ok) == scfq.SCFQ_EARG and b"out2" in detail()
        assert F(b"x.fq", None, None, opts, -1, 5, ok) == scfq.SCFQ_EARG and b"out2" in detail()
    with pytest.raises(scfq.ScfqError) as e:
        scfq.trim_host(FASTQ, FASTQ, scfq.trim_opts(window=40))
    assert e.value.rc == scfq.SCFQ_EARG and "window 40" in str(e.value) and isinstance(e.value.stats, scfq.TrimStats)
    # the edges of the ranges are allowed: what fails then is the missing device or nothing
    for kw in (dict(min_adapter_overlap=1, adapter_mismatch_pct=0, poly_g=1, window=1, window_quality=1, min_length=0, phred_offset=64),
               dict(min_adapter_overlap=32, adapter_mismatch_pct=100, poly_g=512, window=32, window_quality=93, min_length=512),
               dict(probes=[b"A", b"ACGT" * 8] + [b"ACGT"] * 6), dict(no_adapters=True, no_overlap=True)):
        for second in (FASTQ, None):
            try:
                scfq.trim_host(FASTQ, second, scfq.trim_opts(**kw))
            except scfq.ScfqError as err:
                assert err.rc == scfq.SCFQ_EHIP, err


def test_no_gpu_means_loud_failure(scfq, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r1, r2, il = (os.path.join(TRIM, f) for f in ("r1.fq", "r2.fq", "interleaved.fq"))
    for call in (lambda: scfq.trim_host(FASTQ, FASTQ), lambda: scfq.trim_host(FASTQ, None), lambda: scfq.trim_host(b"", b""),
                 lambda: scfq.trim_host(FASTQ, FASTQ, caps=(100, 100)), lambda: scfq.trim_file(r1, r2), lambda: scfq.trim_file(r1),
                 lambda: scfq.trim_file(r1, r2 + ".gz", scfq.trim_opts(**FIXTURE)), lambda: scfq.trim_file(il, None, scfq.trim_opts(interleaved=True))):
        with pytest.raises(scfq.ScfqError) as e:
            call()
        assert e.value.rc == scfq.SCFQ_EHIP
    for a, b in ((os.path.join(TRIM, "does_not_exist.fq"), r2), (os.path.join(TRIM, "does_not_exist.fq"), None)):
        with pytest.raises(scfq.ScfqError) as e:
            scfq.trim_file(a, b)
        assert e.value.rc == scfq.SCFQ_EOPEN
    o1, o2 = tmp_path / "o1.fq", tmp_path / "o2.fq"
    r = run("fq-trim", "--out1=" + str(o1), "--out2=" + str(o2), r1, r2)
    assert r.returncode == 1 and r.stdout == "" and "HIP" in r.stderr
    assert not o1.exists() and not o2.exists()                # a call that fails leaves no output file behind


def test_stats_formatter(scfq):
    names = ("reads_in", "reads_out", "dropped_reads", "short_reads", "too_long", "pairs", "unpaired", "overlapped_pairs", "bases_in", "bases_out",
             "bases_dropped", "cut_overlap", "bases_overlap", "cut_adapter", "bases_adapter", "cut_polyg", "bases_polyg", "cut_quality", "bases_quality")
    w = {k: 101 + 7 * i for i, k in enumerate(names)}
    w.update(adapter_reads=[5, 0, 9, 1, 2, 3, 4, 6], n_probes=3, out1_bytes=123456789012, out2_bytes=77)
    s = scfq._new_trim_stats()
    for k, v in w.items():
        if k == "adapter_reads":
            for j, x in enumerate(v):
                s.adapter_reads[j] = x
        else:
            setattr(s, k, v)
    text = "\t".join(str(w[k]) for k in names) + "\t5,0,9\t123456789012\t77"
    assert scfq.format_trim_stats_tsv(s) == text == stats_text(w)
    assert len(STATS_HEADER.split("\t")) == len(text.split("\t")) == 22
    zero = scfq._new_trim_stats()
    assert scfq.format_trim_stats_tsv(zero) == "\t".join(["0"] * 19 + ["-", "0", "0"]) == stats_text(dict({k: 0 for k in names}, adapter_reads=[0] * 8, n_probes=0, out1_bytes=0, out2_bytes=0))
    s.n_probes = 8
    assert scfq.format_trim_stats_tsv(s).split("\t")[19] == "5,0,9,1,2,3,4,6"
    L = scfq.lib()
    s.n_probes = 3
    assert L.scfq_format_trim_stats_tsv(ctypes.byref(s), None, 0) == len(text)                           # sizing call
    small = ctypes.create_string_buffer(5)
    assert L.scfq_format_trim_stats_tsv(ctypes.byref(s), small, 5) == len(text) and small.value == text[:4].encode()
    exact = ctypes.create_string_buffer(len(text) + 1)
    assert L.scfq_format_trim_stats_tsv(ctypes.byref(s), exact, len(text) + 1) == len(text) and exact.value.decode() == text
    assert L.scfq_format_trim_stats_tsv(None, exact, len(text) + 1) == scfq.SCFQ_EARG
    s.n_probes = 9
    assert L.scfq_format_trim_stats_tsv(ctypes.byref(s), exact, len(text) + 1) == scfq.SCFQ_EARG


def test_cli_without_a_device(tmp_path):
    r = run("fq-trim", "--help")
    assert r.returncode == 0
    for usage in ("fq-trim [options] IN.fq > out.fq", "fq-trim [options] --out1=PATH --out2=PATH R1.fq R2.fq", "fq-trim [options] --interleaved IN.fq > out.fq"):
        assert usage in r.stdout, usage
    for opt in ("--interleaved", "--out1=PATH", "--out2=PATH", "--adapter=NAME:SEQ", "--no-adapters", "--min-adapter-overlap=N", "--adapter-mismatch-pct=N",
                "--poly-g=N", "--window=N", "--window-quality=N", "--min-length=N", "--no-overlap-trim", "--min-overlap=N", "--max-mismatches=N",
                "--max-mismatch-pct=N", "--phred-offset=N", "--stats", "-h, --help"):
        assert opt in r.stdout, opt
    assert run("fq-trim").stdout == r.stdout and run("fq-trim", "-h").stdout == r.stdout
    # the top-level help is pinned by tests/golden/cli_grammar.json and does not list the command yet; an unknown command answers as before
    assert "fq-trim" not in run("--help").stdout
    r = run("bogus")
    assert r.returncode == 1 and "Unknown command: bogus" in r.stderr and r.stdout == run("--help").stdout
    r = run("fq-trim", "does_not_exist.fq")
    c = run("fq-cycles", "does_not_exist.fq")
    assert (r.returncode, r.stderr, r.stdout) == (c.returncode, c.stderr, c.stdout) == (2, "\x1b[31mError 2: Unable to open file: does_not_exist.fq\x1b[0m\n", "")
    r1 = os.path.join(TRIM, "r1.fq")
    o1, o2 = tmp_path / "never_made1.fq", tmp_path / "never_made2.fq"
    r = run("fq-trim", "--out1=" + str(o1), "--out2=" + str(o2), r1, "nor_this.fq")
    assert (r.returncode, r.stdout) == (2, "") and "Unable to open file: nor_this.fq" in r.stderr and not o1.exists() and not o2.exists()
    r, c = run("fq-trim", "--interleaved", "missing.fq.gz"), run("fq-cycles", "missing.fq.gz")
    assert (r.returncode, r.stderr) == (c.returncode, c.stderr) and r.returncode == 1
    r = run("fq-trim", "--stats")
    assert (r.returncode, r.stderr) == (3, "\x1b[31mError 3: No FASTQ specified\x1b[0m\n")
    r, c = run("fq-trim", "--bogus"), run("fq-cycles", "--bogus")
    assert (r.returncode, r.stderr) == (c.returncode, c.stderr) and r.returncode == 1
    assert run("fq-trim", "-x").returncode == 1
    # the number of files, and which outputs go with which input form
    for args in (["a.fq", "b.fq", "c.fq"], ["--interleaved", "a.fq", "b.fq"], ["a.fq", "b.fq"], ["--out1=o.fq", "a.fq", "b.fq"], ["--out2=o.fq", "a.fq", "b.fq"],
                 ["--out1=o.fq", "a.fq"], ["--out1=o.fq", "--out2=p.fq", "a.fq"], ["--interleaved", "--out1=o.fq", "a.fq"],
                 ["--no-adapters", "--adapter=x:ACGT", "a.fq"]):
        r = run("fq-trim", *args)
        assert r.returncode == 1 and "Error" in r.stderr and "@" not in r.stdout, args
    assert not os.path.exists("o.fq") and not os.path.exists("p.fq")
    for bad in (["--min-overlap=0"], ["--min-overlap=513"], ["--max-mismatches=65536"], ["--max-mismatch-pct=101"], ["--phred-offset=34"], ["--phred-offset=x"],
                ["--min-adapter-overlap=0"], ["--min-adapter-overlap=33"], ["--min-adapter-overlap="], ["--adapter-mismatch-pct=101"], ["--adapter-mismatch-pct=2.5"],
                ["--poly-g=513"], ["--poly-g=-1"], ["--poly-g"], ["--window=0"], ["--window=33"], ["--window=x"], ["--window-quality=94"], ["--min-length=513"],
                ["--min-length=1e2"], ["--out1="], ["--out2="], ["--no-adapters=1"], ["--stats=1"],
                # --adapter: fq-adapters' rule
                ["--adapter=ACGT"], ["--adapter=:ACGT"], ["--adapter=x:"], ["--adapter=x:ACGN"], ["--adapter=x:acgt"], ["--adapter=x:" + "A" * 33],
                ["--adapter=a\tb:ACGT"], ["--adapter=n%d:ACGT" % k for k in range(9)]):
        r = run("fq-trim", *bad, r1)
        assert r.returncode == 1 and "Error" in r.stderr and "@" not in r.stdout, bad
    for bad in ("--adapter=ACGT", "--adapter=x:ACGN"):
        r, c = run("fq-trim", bad, r1), run("fq-adapters", bad, r1)
        assert r.returncode == c.returncode == 1 and r.stderr == c.stderr, bad
    r, c = run("fq-trim", "--window=x"), run("fq-cycles", "--max-cycles=x")
    assert r.returncode == c.returncode == 1 and r.stderr == c.stderr.replace("--max-cycles", "--window")


def test_fixture_and_its_golden_outputs():
    r1, r2, il = (open(os.path.join(TRIM, f), "rb").read() for f in ("r1.fq", "r2.fq", "interleaved.fq"))
    gold = {f: open(os.path.join(TRIM, f), "rb").read() for f in ("single.fq", "paired1.fq", "paired2.fq", "interleaved_out.fq")}
    import gzip
    assert gzip.open(os.path.join(TRIM, "r2.fq.gz")).read() == r2
    single, two, inter = both(r1, **FIXTURE), both(r1, r2, **FIXTURE), both(il, interleaved=True, **FIXTURE)
    assert (single["out1"], two["out1"], two["out2"], inter["out1"]) == tuple(gold[k] for k in ("single.fq", "paired1.fq", "paired2.fq", "interleaved_out.fq"))
    assert (two["pairs"], two["reads_in"], two["unpaired"], single["reads_in"], single["pairs"]) == (56, 112, 0, 56, 0)
    for k in ("cut_overlap", "cut_adapter", "cut_polyg", "cut_quality", "dropped_reads", "overlapped_pairs"):
        assert two[k] > 0, k
    assert single["cut_overlap"] == 0 and single["cut_adapter"] > two["cut_adapter"]      # what the overlap step took first in the pairs
    # the interleaved form is the paired one, the outputs record by record in turn
    split = lambda d: [b"".join(x + b"\n" for x in d.split(b"\n")[:-1][k:k + 4]) for k in range(0, d.count(b"\n"), 4)]
    assert inter["out1"] == b"".join(a + b for a, b in zip(split(two["out1"]), split(two["out2"])))
    for k in SCALARS:
        if k not in ("reads1", "reads2", "lines1", "lines2", "input_bytes1", "input_bytes2", "out1_bytes", "out2_bytes", "flags"):
            assert inter[k] == two[k], k
    # every record of the outputs is a prefix of its input record, line by line
    recs_in = {r.split(b"\n")[0]: r.split(b"\n") for r in split(r1) + split(r2)}
    for rec in split(two["out1"]) + split(two["out2"]):
        h, s, p, q, _ = rec.split(b"\n")
        src = recs_in[h]
        assert src[1].startswith(s) and src[3].startswith(q) and len(s) == len(q) >= 15 and p == src[2]


def test_checkers_agree_on_random_blocks():
    rng = np.random.default_rng(401)
    r1, r2 = paired_block(rng, 400, 100, 90)
    r1, r2 = with_random_qualities(rng, r1, 35, 73), with_random_qualities(rng, r2, 35, 73)
    for kw in ({}, dict(poly_g=3, window_quality=15), dict(no_overlap=True, window_quality=22, window=7, min_adapter_overlap=3, adapter_mismatch_pct=20),
               dict(no_adapters=True, poly_g=1, min_length=0), dict(probes=[b"ACG", b"T" * 32, b"GATTACA"], min_adapter_overlap=2, window=32, window_quality=20),
               dict(min_overlap=20, max_mismatches=1, max_mismatch_pct=3, phred_offset=64, window_quality=1, window=1)):
        w = both(r1.tobytes(), r2.tobytes(), **kw)
        assert w["reads_in"] == 800
        both(r1.tobytes(), None, **kw)
        both(r1.tobytes()[:-1], None, interleaved=True, **kw)
    # ragged inputs: "\r\n", a record cut short, reads1 != reads2, quality texts shorter and longer than their sequences
    a = b"@a\r\nACGTACGTACGTACGTACGT\r\n+a\r\nIIIIIIII\r\n@b\r\n" + BODY + b"\r\n+\r\n" + b"I" * 50 + b"\r\n@c\r\nACGT"
    b = b"@a\n" + BODY + UNIVERSAL + b"\n+\n" + b"I" * 52 + b"\n"
    for kw in (dict(min_length=0), dict(min_length=0, window_quality=30, poly_g=2), {}):
        w = both(a, b, **kw)
        assert (w["pairs"], w["unpaired"]) == (1, 2)
        both(a, None, **kw)
        both(a, None, interleaved=True, **kw)
        both(b"", None, **kw), both(b"", b"", **kw), both(b"\n", None, **kw)
    w = both(a, None, min_length=0)
    assert w["out1"] == b"@a\nACGTACGTACGTACGTACGT\n+a\nIIIIIIII\n@b\n" + BODY + b"\n+\n" + b"I" * 40 + b"\n@c\nACGT\n\n\n"      # always four lines


# ---- hand-worked cases of every rule ---------------------------------------------------------------------------------------
def test_adapter_overlap_threshold():
    # t = min_adapter_overlap - 1 against t = min_adapter_overlap, at the read's end
    out, w = one(BODY + UNIVERSAL[:4])
    assert out == b"@r\n" + BODY + UNIVERSAL[:4] + b"\n+\n" + b"I" * 44 + b"\n" and w["cut_adapter"] == 0
    out, w = one(BODY + UNIVERSAL[:5])
    assert out == b"@r\n" + BODY + b"\n+\n" + b"I" * 40 + b"\n" and (w["cut_adapter"], w["bases_adapter"], w["adapter_reads"][0]) == (1, 5, 1)
    out, w = one(BODY + UNIVERSAL[:5], min_adapter_overlap=6)
    assert w["cut_adapter"] == 0
    # the whole probe inside the read: t = m whatever follows
    out, w = one(BODY + UNIVERSAL + b"TTTT", min_adapter_overlap=12)
    assert (w["cut_adapter"], w["bases_adapter"], w["bases_out"]) == (1, 16, 40)


def test_adapter_mismatches_by_percent():
    bad = UNIVERSAL[:4] + b"T" + UNIVERSAL[5:]           # one letter changed
    assert bad != UNIVERSAL and len(bad) == 12
    out, w = one(BODY + bad[:10])                        # one mismatch in t = 10: 100 <= 10 * 10
    assert (w["cut_adapter"], w["bases_adapter"]) == (1, 10)
    out, w = one(BODY + bad[:9], probes=[UNIVERSAL])     # one mismatch in t = 9: 100 > 90
    assert w["cut_adapter"] == 0
    out, w = one(BODY + bad[:9], probes=[UNIVERSAL], adapter_mismatch_pct=12)
    assert (w["cut_adapter"], w["bases_adapter"]) == (1, 9)
    out, w = one(BODY + bad[:10], adapter_mismatch_pct=0)
    assert w["cut_adapter"] == 0


def test_adapter_tie_goes_to_the_lowest_probe_and_the_smallest_position_wins():
    short, long_ = b"ACGTACGTAC", b"ACGTACGTACGG"
    out, w = one(BODY + long_, probes=[long_, short])
    assert w["adapter_reads"][:2] == [1, 0] and w["bases_adapter"] == 12
    out, w = one(BODY + long_, probes=[short, long_])
    assert w["adapter_reads"][:2] == [1, 0] and w["bases_adapter"] == 12
    # a later probe at a smaller position beats an earlier probe at a larger one
    out, w = one(BODY + b"TTTTTTTT" + b"GGGGGGGG", probes=[b"GGGGGGGG", b"TTTTTTTT"])
    assert w["adapter_reads"][:2] == [0, 1] and w["bases_adapter"] == 16


def test_n_and_lower_case_are_mismatches():
    for letter in (b"N", b"g"):                          # UNIVERSAL[4] is 'C'; 'g' is no letter of a probe either
        hit = UNIVERSAL[:4] + letter + UNIVERSAL[5:]
        out, w = one(BODY + hit)                         # one mismatch in 12: 100 <= 120
        assert (w["cut_adapter"], w["bases_adapter"]) == (1, 12), letter
        out, w = one(BODY + hit, adapter_mismatch_pct=0)
        assert w["cut_adapter"] == 0, letter
    out, w = one(BODY + UNIVERSAL.lower())
    assert w["cut_adapter"] == 0
    out, w = one(BODY + UNIVERSAL[:4] + b"c" + UNIVERSAL[5:], adapter_mismatch_pct=0)      # the right letter in lower case
    assert w["cut_adapter"] == 0


def test_poly_g_threshold():
    read = BODY + b"G" * 9
    out, w = one(read, poly_g=10, no_adapters=True)
    assert (w["cut_polyg"], w["bases_out"]) == (0, 49)
    out, w = one(read, poly_g=9, no_adapters=True)
    assert (w["cut_polyg"], w["bases_polyg"], w["bases_out"]) == (1, 9, 40) and out == b"@r\n" + BODY + b"\n+\n" + b"I" * 40 + b"\n"
    out, w = one(BODY + b"G" * 5 + b"g" + b"G" * 4, poly_g=4, no_adapters=True)           # 'g' ends the tail
    assert (w["bases_polyg"], w["bases_out"]) == (4, 46)
    out, w = one(b"G" * 30, poly_g=30, no_adapters=True, min_length=0)                    # the whole read
    assert out == b"@r\n\n+\n\n" and (w["reads_out"], w["bases_out"], w["bases_polyg"]) == (1, 0, 30)
    # the tail is looked for below the adapter's cut
    out, w = one(BODY + b"GGGGGG" + UNIVERSAL, poly_g=6)
    assert (w["bases_adapter"], w["bases_polyg"], w["bases_out"]) == (12, 6, 40)


def test_quality_window_rule():
    q = lambda *v: bytes(33 + x for x in v)
    seq = b"ACGTACGTAC"
    # a window whose sum equals the threshold is no cut: 4 x 20 = 80
    out, w = one(seq, q(*[20] * 10), window_quality=20, no_adapters=True, min_length=0)
    assert (w["cut_quality"], w["bases_out"]) == (0, 10)
    out, w = one(seq, q(20, 20, 20, 20, 20, 20, 19, 20, 20, 20), window_quality=20, no_adapters=True, min_length=0)
    assert (w["cut_quality"], w["bases_quality"], w["bases_out"]) == (1, 7, 3) and out == b"@r\nACG\n+\n" + q(20, 20, 20) + b"\n"      # the first window with the 19: p = 3
    # only whole windows below e count: a bad base in the last window - 1 positions is kept when no whole window is bad
    out, w = one(seq, q(40, 40, 40, 40, 40, 40, 40, 40, 40, 2), window_quality=20, no_adapters=True, min_length=0)
    assert w["cut_quality"] == 0                         # 40 + 40 + 40 + 2 = 122 >= 80
    out, w = one(seq, q(40, 40, 40, 40, 40, 40, 2, 2, 2, 2), window_quality=20, no_adapters=True, min_length=0)
    assert w["bases_out"] == 5                           # p = 5: 40 + 2 + 2 + 2 = 46 < 80; p = 4: 40 + 40 + 2 + 2 = 84
    out, w = one(seq, q(*[2] * 10), window=32, window_quality=40, no_adapters=True, min_length=0)
    assert w["cut_quality"] == 0                         # the read is shorter than the window
    # a quality byte below the offset counts as a negative number: offset 64, '5' is -11
    qual = b"h" * 6 + b"5" + b"h" * 3                    # 'h' is 40
    out, w = one(seq, qual, window=4, window_quality=28, phred_offset=64, no_adapters=True, min_length=0)
    assert w["bases_out"] == 3                           # 3 x 40 - 11 = 109 < 112
    out, w = one(seq, qual, window=4, window_quality=27, phred_offset=64, no_adapters=True, min_length=0)
    assert w["cut_quality"] == 0                         # 109 >= 108
    # LQ < L: the missing quality bytes count as 0, and the quality text comes out as far as it goes
    out, w = one(seq, b"IIIIII", window=4, window_quality=10, no_adapters=True, min_length=0)
    assert w["bases_out"] == 6 and out == b"@r\nACGTAC\n+\nIIIIII\n"      # p = 4: 40 + 40 + 0 + 0 = 80; p = 5: 40 < 40 is false; p = 6: 0 < 40
    out, w = one(seq, b"IIIIII", no_adapters=True, min_length=0)
    assert out == b"@r\n" + seq + b"\n+\nIIIIII\n"
    out, w = one(seq, b"I" * 14, no_adapters=True, min_length=0)      # LQ > L: cut to the sequence's length
    assert out == b"@r\n" + seq + b"\n+\n" + b"I" * 10 + b"\n"


def test_minimum_length_and_pairs_stay_in_step():
    out, w = one(b"ACGTACGTACGTAC")                     # 14 < 15
    assert out == b"" and (w["short_reads"], w["dropped_reads"], w["bases_dropped"], w["reads_out"]) == (1, 1, 14, 0)
    out, w = one(b"ACGTACGTACGTACG")
    assert w["reads_out"] == 1
    good, bad = b"@g\n" + BODY + b"\n+\n" + b"I" * 40 + b"\n", b"@b\nACGT\n+\nIIII\n"
    w = both(good + bad, bad + good, no_overlap=True)
    assert (w["short_reads"], w["dropped_reads"], w["bases_dropped"], w["reads_out"], w["out1"], w["out2"]) == (2, 4, 88, 0, b"", b"")
    w = both(good + bad + good, good + good + good, no_overlap=True)
    assert (w["short_reads"], w["dropped_reads"], w["out1"], w["out2"]) == (1, 2, good + good, good + good)
    w = both(good + bad + good + bad, None, interleaved=True, no_overlap=True)
    assert w["out1"] == b"" and w["dropped_reads"] == 4
    # a too-long mate is never short and is echoed as it is; its pair still goes when the other mate is short
    big = b"@L\n" + b"A" * 513 + b"\n+\nII\n"
    w = both(big + big, good + bad, no_overlap=True)
    assert (w["too_long"], w["short_reads"], w["dropped_reads"], w["out1"], w["out2"], w["bases_dropped"]) == (2, 1, 2, big, good, 513 + 4)
    w = both(big, None)
    assert w["out1"] == big and w["bases_in"] == w["bases_out"] == 513


def test_overlap_step():
    rng = np.random.default_rng(409)
    a, b = planted(rng, 100, 100, 60)                   # a fragment of 60: both mates read 40 bases into what follows
    rec = lambda n, s: b"@" + n + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n"
    w = both(rec(b"1", a), rec(b"2", b), no_adapters=True)
    assert (w["overlapped_pairs"], w["cut_overlap"], w["bases_overlap"], w["bases_out"]) == (1, 2, 80, 120)
    assert w["out1"] == rec(b"1", a[:60]) and w["out2"] == rec(b"2", b[:60])
    w = both(rec(b"1", a), rec(b"2", b), no_adapters=True, no_overlap=True)
    assert (w["overlapped_pairs"], w["cut_overlap"], w["bases_out"]) == (0, 0, 200)
    a, b = planted(rng, 100, 80, 150)                   # the mates overlap by 30 inside the fragment: nothing to cut
    w = both(rec(b"1", a), rec(b"2", b), no_adapters=True)
    assert (w["overlapped_pairs"], w["cut_overlap"], w["bases_out"]) == (1, 0, 180)
    a, b = planted(rng, 100, 80, 90)                    # insert 90: only mate 1 is longer
    w = both(rec(b"1", a), rec(b"2", b), no_adapters=True)
    assert (w["overlapped_pairs"], w["cut_overlap"], w["bases_overlap"]) == (1, 1, 10)
    w = both(rec(b"1", a) + rec(b"2", b), None, interleaved=True, no_adapters=True)
    assert w["out1"] == rec(b"1", a[:90]) + rec(b"2", b)

"""fq-adapters without a device: the ABI (symbols, struct layout, C99 header), argument checks, the built-in set, the row formatter,
the CLI's header / help / error behaviour, and the two checkers of _adapters_check.py against each other and literal tables."""
import ctypes
import glob
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG, ROOT
from _adapters_check import COLS, MAX_PROBES, adapters_of, adapters_of_np, cli_text, nim, same, totals_text
from test_gpu_parity import random_fastq_like

SC = os.path.join(PKG, "sc")
BUILTIN = [("illumina_universal", "AGATCGGAAGAG"), ("illumina_small_rna_3p", "TGGAATTCTCGG"), ("illumina_small_rna_5p", "GATCGTCGGACT"),
           ("nextera", "CTGTCTCTTATA"), ("polya", "AAAAAAAAAAAA"), ("polyg", "GGGGGGGGGGGG"), ("solid_small_rna", "CGCCTTGGCCGT")]
HEADER = "position\t" + "\t".join(n for n, _ in BUILTIN) + "\tany"
TOTALS_HEADER = "adapter\tsequence\treads\treads_with\tpercent\thits"
NEW = ("scfq_adapters_buffer", "scfq_adapters_file", "scfq_adapters_default", "scfq_format_adapter_row_tsv", "scfq_adapters_error_detail")
FASTQ = b"@h\nACGTN\n+\nIIIII\n"
HEAD = ("struct_size", "abi_version", "reads", "lines", "input_bytes", "n_probes", "max_seq_len", "positions")
PROBE_SETS = (("A", "AC", "ACGT", "ACGTACGTACGTACGTA"), ("G", "GT", "TTT", "CA"), tuple(s for _, s in BUILTIN))


def run(*args):
    return subprocess.run([SC] + list(args), capture_output=True, text=True, stdin=subprocess.DEVNULL)


def test_symbols_declared_exported_and_listed(scfq):
    header = open(os.path.join(ROOT, "include", "sc_fqcount.h")).read()
    debug = open(os.path.join(ROOT, "include", "sc_fqcount_debug.h")).read()
    L = scfq.lib()
    for name in NEW:
        assert name + "(" in header and name in scfq.EXPORTS and hasattr(L, name), name
    assert "scfq_debug_adapters_stages(" in debug and "scfq_debug_adapters_stages" in scfq.EXPORTS and hasattr(L, "scfq_debug_adapters_stages")
    assert len(scfq.adapters_stages()) == 4
    assert (scfq.ADAPTERS_MAX_PROBES, scfq.ADAPTERS_MAX_LEN, scfq.ADAPTERS_MAX_CAP) == (8, 32, 1 << 24)
    for name in ("SCFQ_ADAPTERS_MAX_PROBES", "SCFQ_ADAPTERS_MAX_LEN", "SCFQ_ADAPTERS_MAX_CAP"):
        assert name in header, name
    for name in ("AdapterRow", "AdapterSummary", "adapters_device", "adapters_host", "adapters_file", "adapters_default", "format_adapter_row_tsv",
                 "adapters_stages"):
        assert hasattr(scfq, name), name


def test_struct_layout(scfq):
    R, S = scfq.AdapterRow, scfq.AdapterSummary
    assert ctypes.sizeof(R) == 72 and R.first.offset == 0 and R.first.size == 64 and R.any.offset == 64
    assert tuple(f[0] for f in S._fields_) == HEAD + ("probe_len", "hits", "tail", "total")
    for k, name in enumerate(HEAD):
        assert getattr(S, name).offset == 8 * k and getattr(S, name).size == 8, name
    assert (S.probe_len.offset, S.hits.offset, S.tail.offset, S.total.offset) == (64, 128, 192, 264)
    assert ctypes.sizeof(S) == 8 * 42


def test_header_is_c99_and_sizes_agree(tmp_path):
    src = tmp_path / "t.c"
    offsets = " && ".join("offsetof(scfq_adapter_summary, %s) == %d" % (name, 8 * k) for k, name in enumerate(HEAD))
    offsets += " && offsetof(scfq_adapter_summary, probe_len) == 64 && offsetof(scfq_adapter_summary, hits) == 128"
    offsets += " && offsetof(scfq_adapter_summary, tail) == 192 && offsetof(scfq_adapter_summary, total) == 264"
    offsets += " && offsetof(scfq_adapter_row, first) == 0 && offsetof(scfq_adapter_row, any) == 64"
    src.write_text('#include <stddef.h>\n#include "sc_fqcount.h"\n#include "sc_fqcount_debug.h"\n'
                   "typedef char sum_size[sizeof(scfq_adapter_summary) == 8 * 42 ? 1 : -1];\n"
                   "typedef char row_size[sizeof(scfq_adapter_row) == 8 * 9 ? 1 : -1];\n"
                   "typedef char at[" + offsets + " ? 1 : -1];\n"
                   "typedef char consts[SCFQ_ADAPTERS_MAX_PROBES == 8 && SCFQ_ADAPTERS_MAX_LEN == 32 && SCFQ_ADAPTERS_MAX_CAP == 16777216 ? 1 : -1];\n"
                   "int main(void){ scfq_adapter_summary s; scfq_adapter_row r[2]; double ms[4]; const char* p[1]; const char *name, *seq;\n"
                   "  p[0] = \"ACGT\"; s.struct_size = sizeof s;\n"
                   "  return scfq_adapters_buffer(0, 0, 0, p, 1, r, 2, &s) + scfq_format_adapter_row_tsv(r, 1, 2, 0, 0, 0)\n"
                   "         + scfq_adapters_file(\"x\", 0, p, 1, 0, 0, &s) + scfq_debug_adapters_stages(ms, 4) + scfq_adapters_default(0, &name, &seq)\n"
                   "         + (scfq_adapters_error_detail() != 0) == 12345; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-fsyntax-only", str(src)])


def probe_array(*probes):
    return (ctypes.c_char_p * max(len(probes), 1))(*probes)


def test_argument_checks(scfq):
    L = scfq.lib()
    s = scfq._new_adapter_summary()
    buf = ctypes.create_string_buffer(FASTQ)
    n = len(FASTQ)
    rows = (scfq.AdapterRow * 4)()
    ok = ctypes.byref(s)
    one = probe_array(b"ACGT")
    detail = L.scfq_adapters_error_detail
    # without text
    assert L.scfq_adapters_buffer(buf, n, 0, one, 1, rows, 4, None) == scfq.SCFQ_EARG                   # NULL summary
    bad = scfq.AdapterSummary()                                                                        # struct_size not set
    assert L.scfq_adapters_buffer(buf, n, 0, one, 1, rows, 4, ctypes.byref(bad)) == scfq.SCFQ_EARG
    bad.struct_size = ctypes.sizeof(scfq.AdapterSummary) - 8
    assert L.scfq_adapters_buffer(buf, n, 0, one, 1, rows, 4, ctypes.byref(bad)) == scfq.SCFQ_EARG
    assert L.scfq_adapters_buffer(None, n, 0, one, 1, rows, 4, ok) == scfq.SCFQ_EARG                    # NULL pointer with n > 0
    assert L.scfq_adapters_buffer(buf, n, 0, one, 1, None, 4, ok) == scfq.SCFQ_EARG                     # NULL rows with cap > 0
    assert L.scfq_adapters_buffer(buf, n, 0, None, 1, rows, 4, ok) == scfq.SCFQ_EARG                    # NULL probes
    assert L.scfq_adapters_file(None, None, one, 1, rows, 4, ok) == scfq.SCFQ_EARG
    assert L.scfq_adapters_file(b"x.fq", None, one, 1, rows, 4, ctypes.byref(bad)) == scfq.SCFQ_EARG
    assert L.scfq_adapters_file(b"x.fq", None, one, 1, None, 4, ok) == scfq.SCFQ_EARG
    assert L.scfq_adapters_file(b"x.fq", None, None, 1, rows, 4, ok) == scfq.SCFQ_EARG
    assert detail() == b""

    def both(probes, n_probes, cap, *texts):
        for call in (lambda: L.scfq_adapters_buffer(buf, n, 0, probes, n_probes, rows if cap else None, cap, ok),
                     lambda: L.scfq_adapters_file(b"x.fq", None, probes, n_probes, rows if cap else None, cap, ok)):
            assert call() == scfq.SCFQ_EARG, texts
            for t in texts:
                assert t in detail(), (t, detail())

    both(one, 0, 4, b"0 probes", b"8")
    both(probe_array(*[b"A"] * 9), 9, 4, b"9 probes", b"8")
    both(probe_array(b"ACGT", None), 2, 4, b"probe 1", b"NULL")
    both(probe_array(b"ACGT", b"A", b""), 3, 4, b"probe 2", b"empty")
    both(probe_array(b"A" * 33), 1, 0, b"probe 0", b"longer than 32")
    both(probe_array(b"ACGT", b"ACGN"), 2, 4, b"probe 1", b"0x4e", b"at 3", b"A C G T")
    both(probe_array(b"acgt"), 1, 4, b"probe 0", b"0x61", b"at 0")
    both(probe_array(b"AC\rGT"), 1, 4, b"probe 0", b"0x0d", b"at 2")
    big = (1 << 24) + 1
    assert L.scfq_adapters_buffer(buf, n, 0, one, 1, rows, big, ok) == scfq.SCFQ_EARG                   # cap above the limit
    assert b"cap 16777217" in detail() and b"16777216" in detail()
    assert L.scfq_adapters_file(b"x.fq", None, one, 1, rows, big, ok) == scfq.SCFQ_EARG and b"cap 16777217" in detail()
    with pytest.raises(scfq.ScfqError) as e:
        scfq.adapters_host(FASTQ, ["ACGU"])
    assert e.value.rc == scfq.SCFQ_EARG and "0x55" in str(e.value)
    with pytest.raises(scfq.ScfqError) as e:
        scfq.adapters_host(FASTQ, [])
    assert e.value.rc == scfq.SCFQ_EARG and "0 probes" in str(e.value)
    # 32 letters are allowed, and the same probe twice: what fails then is the missing device or nothing
    for probes in (["A" * 32], ["ACGT", "ACGT"]):
        try:
            scfq.adapters_host(FASTQ, probes)
        except scfq.ScfqError as err:
            assert err.rc == scfq.SCFQ_EHIP, err


def test_no_gpu_means_loud_failure(scfq):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    for cap in (0, 5):
        for probes in (None, ["ACGT"], ["A" * 17]):
            with pytest.raises(scfq.ScfqError) as e:
                scfq.adapters_host(FASTQ, probes, cap)
            assert e.value.rc == scfq.SCFQ_EHIP
            with pytest.raises(scfq.ScfqError) as e:
                scfq.adapters_file(os.path.join(GOLDEN, "dup.fq"), probes, cap)
            assert e.value.rc == scfq.SCFQ_EHIP
    with pytest.raises(scfq.ScfqError) as e:
        scfq.adapters_file(os.path.join(GOLDEN, "does_not_exist.fq"), None, 5)
    assert e.value.rc == scfq.SCFQ_EOPEN


def test_builtin_set(scfq):
    assert scfq.adapters_default() == BUILTIN and len(BUILTIN) == 7
    L = scfq.lib()
    name, seq = ctypes.c_char_p(), ctypes.c_char_p()
    for i, (nm, sq) in enumerate(BUILTIN):
        assert L.scfq_adapters_default(i, ctypes.byref(name), ctypes.byref(seq)) == 7 and (name.value, seq.value) == (nm.encode(), sq.encode())
        assert L.scfq_adapters_default(i, None, None) == 7
        assert len(sq) == 12 and set(sq) <= set("ACGT")
    for i in (7, 8, 1 << 31):
        assert L.scfq_adapters_default(i, ctypes.byref(name), ctypes.byref(seq)) == scfq.SCFQ_EARG


def test_row_formatter(scfq):
    row = [3, 0, 1, 0, 0, 0, 0, 0, 4]
    assert scfq.format_adapter_row_tsv(row, 3, 8, counts=True) == "3\t0\t1\t4"
    assert scfq.format_adapter_row_tsv(row, 3, 8) == "37.5\t0.0\t12.5\t50.0"
    assert scfq.format_adapter_row_tsv(row, 1, 3) == "100.0\t%s" % nim(400, 3) == "100.0\t133.3333333333333"
    assert scfq.format_adapter_row_tsv(row, 1, 7) == "%s\t%s" % (nim(300, 7), nim(400, 7))
    assert scfq.format_adapter_row_tsv([0] * 9, 2, 0) == "nan\tnan\tnan"                              # 0 / 0
    assert scfq.format_adapter_row_tsv([0] * 9, 2, 0, counts=True) == "0\t0\t0"
    full = [2 ** 64 - 1] * 9
    assert scfq.format_adapter_row_tsv(full, 8, 1, counts=True) == "\t".join(["18446744073709551615"] * 9)
    assert scfq.format_adapter_row_tsv(list(range(1, 10)), 8, 200) == "\t".join(nim(100 * v, 200) for v in range(1, 10))
    # only the first n_probes columns and `any` are printed
    assert scfq.format_adapter_row_tsv([1, 2, 3, 4, 5, 6, 7, 8, 9], 2, 1, counts=True) == "1\t2\t9"
    L = scfq.lib()
    r = scfq.AdapterRow((ctypes.c_uint64 * 8)(3, 0, 1), 4)
    text = "3\t0\t1\t4"
    assert L.scfq_format_adapter_row_tsv(ctypes.byref(r), 3, 8, 1, None, 0) == len(text)                # sizing call
    small = ctypes.create_string_buffer(5)
    assert L.scfq_format_adapter_row_tsv(ctypes.byref(r), 3, 8, 1, small, 5) == len(text) and small.value == text[:4].encode()
    exact = ctypes.create_string_buffer(len(text) + 1)
    assert L.scfq_format_adapter_row_tsv(ctypes.byref(r), 3, 8, 1, exact, len(text) + 1) == len(text) and exact.value.decode() == text
    pct = "37.5\t0.0\t12.5\t50.0"
    assert L.scfq_format_adapter_row_tsv(ctypes.byref(r), 3, 8, 0, None, 0) == len(pct)
    for n_probes in (0, 9, 1 << 31):
        assert L.scfq_format_adapter_row_tsv(ctypes.byref(r), n_probes, 8, 1, None, 0) == scfq.SCFQ_EARG
    assert L.scfq_format_adapter_row_tsv(None, 3, 8, 1, None, 0) == scfq.SCFQ_EARG


def test_cli_without_a_device():
    r = run("fq-adapters", "--help")
    assert r.returncode == 0 and "fq-adapters [options] [fastq ...]" in r.stdout
    for opt in ("--adapter=NAME:SEQ", "--max-positions=N", "--counts", "--totals", "-t, --header", "-b, --basename", "-a, --absolute", "-h, --help"):
        assert opt in r.stdout, opt
    assert run("fq-adapters").stdout == r.stdout and run("fq-adapters", "-h").stdout == r.stdout
    top = run("--help").stdout
    assert "Adapter content by read position of a FASTQ" in top and top.index("fq-kmers") < top.index("fq-adapters") < top.index("FASTA")
    r = run("fq-adapters", "-t", "-b")
    assert (r.returncode, r.stdout, r.stderr) == (0, HEADER + "\tbasename\n", "")
    assert run("fq-adapters", "-tba").stdout == HEADER + "\tbasename\tabsolute\n"
    assert run("fq-adapters", "--header", "--counts", "--max-positions=0").stdout == HEADER + "\n"
    assert run("fq-adapters", "-t", "--adapter=mine:ACGT", "--adapter=other one:" + "T" * 32).stdout == "position\tmine\tother one\tany\n"
    assert run("fq-adapters", "-t", "-a", "--adapter=x:A").stdout == "position\tx\tany\tabsolute\n"
    assert run("fq-adapters", "-t", *["--adapter=p%d:ACG" % k for k in range(8)]).stdout == "position\t" + "\t".join("p%d" % k for k in range(8)) + "\tany\n"
    assert run("fq-adapters", "--header", "--totals").stdout == TOTALS_HEADER + "\n"
    assert run("fq-adapters", "-tba", "--totals", "--adapter=x:A").stdout == TOTALS_HEADER + "\tbasename\tabsolute\n"
    r = run("fq-adapters", "does_not_exist.fq")
    c = run("fq-cycles", "does_not_exist.fq")
    assert (r.returncode, r.stderr, r.stdout) == (c.returncode, c.stderr, c.stdout) == (2, "\x1b[31mError 2: Unable to open file: does_not_exist.fq\x1b[0m\n", "")
    r, c = run("fq-adapters", "missing.fq.gz"), run("fq-cycles", "missing.fq.gz")
    assert (r.returncode, r.stderr) == (c.returncode, c.stderr) and r.returncode == 1
    r, c = run("fq-adapters", "-b"), run("fq-cycles", "-b")
    assert (r.returncode, r.stderr) == (c.returncode, c.stderr) == (3, "\x1b[31mError 3: No FASTQ specified\x1b[0m\n")
    r, c = run("fq-adapters", "--bogus"), run("fq-cycles", "--bogus")
    assert (r.returncode, r.stderr) == (c.returncode, c.stderr) and r.returncode == 1
    r, c = run("fq-adapters", "-x"), run("fq-cycles", "-x")
    assert (r.returncode, r.stderr) == (c.returncode, c.stderr) and r.returncode == 1
    nine = ["--adapter=p%d:ACG" % k for k in range(9)]
    for bad in (["--adapter=x"], ["--adapter=:ACGT"], ["--adapter=n:ACGN"], ["--adapter=n:acgt"], ["--adapter=n:"], ["--adapter=n:" + "A" * 33], nine,
                ["--adapter=a\tb:ACGT"], ["--adapter=a:b:ACGT"], ["--adapter="], ["--adapter"],
                ["--max-positions="], ["--max-positions=x"], ["--max-positions=16777217"], ["--max-positions=-1"], ["--max-positions"]):
        for totals in ((), ("--totals",)):
            r = run("fq-adapters", "-t", *bad, *totals)
            assert r.returncode == 1 and "position\t" not in r.stdout and TOTALS_HEADER not in r.stdout and "Error" in r.stderr, bad
    r, c = run("fq-adapters", "--max-positions=x"), run("fq-cycles", "--max-cycles=x")
    assert r.returncode == c.returncode == 1 and r.stderr == c.stderr.replace("--max-cycles", "--max-positions")
    assert "Bad value for --adapter: n:ACGN" in run("fq-adapters", "--adapter=n:ACGN").stderr


def golden_files():
    return sorted(glob.glob(os.path.join(GOLDEN, "*.fq")) + glob.glob(os.path.join(GOLDEN, "edge", "*.fq")))


def check_agree(data, ctx, probe_sets=PROBE_SETS):
    """the plain checker against the numpy one; the identities every result has to keep"""
    a = np.frombuffer(data, dtype=np.uint8)
    for probes in probe_sets:
        p = adapters_of(data, probes)
        q = adapters_of_np(a, probes)
        assert same(p, q), (ctx, probes, p[1:], q[1:])
        rows, hits, total, max_len, lines = p
        reads = (lines + 3) // 4
        assert rows.shape == (max_len, COLS) and rows.dtype == np.uint64, ctx
        assert [int(v) for v in rows.sum(axis=0)] == total, (ctx, probes)
        k = len(probes)
        assert all(v == 0 for v in hits[k:]) and all(v == 0 for v in total[k:MAX_PROBES]), (ctx, probes)
        assert all(h >= t for h, t in zip(hits, total)), (ctx, probes)
        assert max(total[:MAX_PROBES]) <= total[MAX_PROBES] <= min(reads, sum(total[:MAX_PROBES])), (ctx, probes)


def test_checkers_agree_on_the_fixtures(scfq):
    assert hasattr(scfq, "adapters_file")
    files = golden_files()
    assert len(files) >= 30
    for path in files:
        data = open(path, "rb").read()
        check_agree(data, path, PROBE_SETS if len(data) < 200_000 else PROBE_SETS[:1])


@pytest.mark.parametrize("kind", ["uniform", "ascii", "dense_nl", "sparse_nl", "crlf"])
def test_checkers_agree_on_random_buffers(scfq, kind):
    assert hasattr(scfq, "adapters_device")
    rng = np.random.default_rng(53)
    for n in (0, 1, 2, 15, 16, 17, 255, 4096, 20_000):
        a = random_fastq_like(rng, n, kind)
        for cut in (n, n - 1, 2 * n // 3):
            if cut >= 0:
                check_agree(bytes(a[:cut]), (kind, n, cut), (("A", "GC", "ACGTA"), ("G", "TT", "T", "GGGGG")))


def first_positions(rows, col):
    return {int(p): int(rows[p, col]) for p in np.flatnonzero(rows[:, col])}


def test_literal_tables(scfq):
    assert hasattr(scfq, "format_adapter_row_tsv")
    gold = lambda *parts: open(os.path.join(GOLDEN, *parts), "rb").read()
    rows, hits, total, max_len, lines = adapters_of(gold("edge", "many_short.fq"), ["ACGT"])
    assert (first_positions(rows, 0), first_positions(rows, 8), hits[0], total[0], total[8], lines) == ({0: 300}, {0: 300}, 300, 300, 300, 1200)
    rows, hits, total, max_len, lines = adapters_of(gold("edge", "n_rich.fq"), ["ACGT"])
    assert (first_positions(rows, 0), hits[0], total[0], total[8]) == ({4: 1}, 1, 1, 1)
    rows, hits, total, max_len, lines = adapters_of(gold("edge", "long_line_50k.fq"), ["ACGT"])
    assert (first_positions(rows, 0), hits[0], total[0], total[8]) == ({0: 1}, 5000, 1, 1)
    rows, hits, total, max_len, lines = adapters_of(gold("sra.fq"), ["ACGT"])
    assert first_positions(rows, 0) == {13: 1} and total[0] == 1
    rows, hits, total, max_len, lines = adapters_of(gold("sra.fq"), ["AC"])
    assert (first_positions(rows, 0), hits[0], total[0], total[8]) == ({10: 1, 33: 1}, 7, 2, 2)
    builtin = [s for _, s in BUILTIN]
    for path in golden_files():
        rows, hits, total, max_len, lines = adapters_of_np(np.frombuffer(open(path, "rb").read(), dtype=np.uint8), builtin)
        assert not rows.any() and hits == [0] * 8 and total == [0] * 9, path
    # A C G T are legal quality bytes: nothing comes from the quality line, the header or the separator
    polya = dict(BUILTIN)["polya"]
    rows, hits, total, max_len, lines = adapters_of(b"@h\nAAAAAAAAAAAAAAAAAAAA\n+\nAAAAAAAAAAAAAAAAAAAA\n", [polya])
    assert (first_positions(rows, 0), hits[0], total[0], total[8], max_len) == ({0: 1}, 9, 1, 1, 20)
    want = adapters_of(b"@AAAAAAAAAAAAAAAA\nCCCC\n+AAAAAAAAAAAAAAAA\nIIII\n", [polya, "AAAA"])
    assert not want[0].any() and want[1] == [0] * 8 and want[2] == [0] * 9 and want[3:] == (4, 4)
    # the texts the CLI prints
    want = adapters_of(b"@h\nTTACGT\n+\nIIIIII\n@g\nACGTAC\n+\nIIIIII\n@f\nGGGGGG\n+\nIIIIII\n@e\nGGGGAC\n+\nIIIIII\n", ["ACGT", "AC"])
    assert cli_text(want, 2, counts=True) == "1\t1\t1\t1\n2\t0\t0\t0\n3\t1\t1\t1\n4\t0\t0\t0\n5\t0\t1\t1\n6\t0\t0\t0\n"
    assert cli_text(want, 2) == "1\t25.0\t25.0\t25.0\n2\t25.0\t25.0\t25.0\n3\t50.0\t50.0\t50.0\n4\t50.0\t50.0\t50.0\n5\t50.0\t75.0\t75.0\n6\t50.0\t75.0\t75.0\n"
    assert cli_text(want, 2, max_positions=2, suffix="\tx") == "1\t25.0\t25.0\t25.0\tx\n2\t25.0\t25.0\t25.0\tx\n>2\t50.0\t75.0\t75.0\tx\n"
    assert cli_text(want, 2, max_positions=2, counts=True) == "1\t1\t1\t1\n2\t0\t0\t0\n>2\t1\t2\t2\n"
    assert cli_text(want, 2, max_positions=5) == cli_text(want, 2)[:-len("6\t50.0\t75.0\t75.0\n")]      # nothing beyond: no ">5" row
    assert totals_text(want, ["x", "y"], ["ACGT", "AC"], "\tf.fq") == "x\tACGT\t4\t2\t50.0\t2\tf.fq\ny\tAC\t4\t3\t75.0\t4\tf.fq\nany\t*\t4\t3\t75.0\t6\tf.fq\n"

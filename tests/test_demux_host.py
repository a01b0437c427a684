"""fq-demux without a device: the ABI (symbols, struct layouts, the C99 header), every argument and sheet error of the library (each is
decided before any device call), the row formatter, the command's help and usage errors, the checker against hand-worked cases whose
expected bytes and numbers stand here literally, and the fixtures against the script that makes them."""
import ctypes
import gzip
import importlib.util
import os
import subprocess

import pytest

from conftest import GOLDEN, PKG, ROOT
from _demux_check import AMBIGUOUS, ASSIGNED, NO_BARCODE, REPORT_HEADER, UNMATCHED, assign, candidates, check_identities, demux_of, report_text

SC = os.path.join(PKG, "sc")
DEMUX = os.path.join(GOLDEN, "demux")
NEW_SYMBOLS = ("scfq_demux_sheet_new", "scfq_demux_sheet_free", "scfq_demux_sheet_samples", "scfq_demux_sheet_name", "scfq_demux_buffers",
               "scfq_demux_files", "scfq_format_demux_row_tsv", "scfq_demux_error_detail", "scfq_debug_demux_stages")
NONE = (0xFFFF, 0xFF, 0xFF)


def run(*args):
    return subprocess.run([SC] + list(args), capture_output=True, text=True, stdin=subprocess.DEVNULL)


def rec(header, seq, qual=None, sep=b"+"):
    return b"@" + header + b"\n" + seq + b"\n" + sep + b"\n" + (b"I" * len(seq) if qual is None else qual) + b"\n"


def case(name, samples, d1, d2, kw, recs, out1, out2=b"", units=None, **stats):
    return dict(name=name, samples=samples, d1=d1, d2=d2, kw=kw, recs=recs, out1=out1, out2=out2, units=units, stats=stats)


ONE = [("a", "ACGT")]
LONG = [("a", "ACGTACGT")]
MM_READS = b"".join(rec(b"m%d" % i, s) for i, s in enumerate((b"ACGTACGTAA", b"TCGTACGTAA", b"TGGTACGTAA", b"TGCTACGTAA", b"TGCAACGTAA")))
MM_ECHO = [rec(b"m%d" % i, s) for i, s in enumerate((b"ACGTACGTAA", b"TCGTACGTAA", b"TGGTACGTAA", b"TGCTACGTAA", b"TGCAACGTAA"))]
MM_CLIP = [rec(b"m%d" % i, b"AA") for i in range(5)]
TIE = [("a", "AAAA"), ("b", "AAAT")]
PREFIX = [("p", "ACGT"), ("q", "ACGTAA")]
DUAL = [("a", "ACGT", "TTGA")]
HEADERS = (b"r0 no colon here", b"r1 1:N:0:", b"r2 1:N:0:ACGT+TTGA", b"r3 1:N:0:+TTGA", b"r4 1:N:0:ACGT+", b"r5 1:N:0:ACGT+TTG+", b"r6 1:N:0:ACGT++TGA",
           b"r7:ACGT", b"r8 1:N:0:ACGTTTGA")
HEADER_READS = [rec(h, b"GGGGGG") for h in HEADERS]

# one per rule of the contract in include/sc_fqcount.h; every expected byte and number is written out
HAND = [
    case("N in the barcode is a mismatch", ONE, rec(b"r", b"ANGTTT"), None, {}, [(0, 1, 0, ASSIGNED)], rec(b"r", b"TT"), units=[1, 0],
         perfect=0, mismatched=1, bases_in=6, bases_out=2, bases_clipped=4),
    case("N in the barcode, no mismatch allowed", ONE, rec(b"r", b"ANGTTT"), None, dict(mismatches=0), [NONE + (UNMATCHED,)], rec(b"r", b"ANGTTT"), units=[0, 1],
         unmatched=1, undetermined=1, bases_out=6, bases_clipped=0),
    case("lower case is a mismatch", ONE, rec(b"r", b"AcGTTT"), None, {}, [(0, 1, 0, ASSIGNED)], rec(b"r", b"TT"), units=[1, 0], mismatched=1),
    case("L < m: no sample is eligible", ONE, rec(b"r", b"ACG"), None, {}, [NONE + (NO_BARCODE,)], rec(b"r", b"ACG"), units=[0, 1], no_barcode=1, unmatched=0),
    case("L = m: an empty sequence line", ONE, rec(b"r", b"ACGT"), None, {}, [(0, 0, 0, ASSIGNED)], b"@r\n\n+\n\n", units=[1, 0], perfect=1, bases_out=0, bases_clipped=4),
    case("M = 0", LONG, MM_READS, None, dict(mismatches=0), [(0, 0, 0, ASSIGNED)] + [NONE + (UNMATCHED,)] * 4, MM_CLIP[0] + b"".join(MM_ECHO[1:]), units=[1, 4]),
    case("M = 1", LONG, MM_READS, None, dict(mismatches=1), [(0, 0, 0, ASSIGNED), (0, 1, 0, ASSIGNED)] + [NONE + (UNMATCHED,)] * 3,
         b"".join(MM_CLIP[:2] + MM_ECHO[2:]), units=[2, 3], perfect=1, mismatched=1),
    case("M = 2", LONG, MM_READS, None, dict(mismatches=2), [(0, 0, 0, ASSIGNED), (0, 1, 0, ASSIGNED), (0, 2, 0, ASSIGNED)] + [NONE + (UNMATCHED,)] * 2,
         b"".join(MM_CLIP[:3] + MM_ECHO[3:]), units=[3, 2]),
    case("M = 3", LONG, MM_READS, None, dict(mismatches=3), [(0, k, 0, ASSIGNED) for k in range(4)] + [NONE + (UNMATCHED,)], b"".join(MM_CLIP[:4] + MM_ECHO[4:]),
         units=[4, 1], perfect=1, mismatched=3, unmatched=1),
    case("a tie at the same t is ambiguous; a smaller t wins", TIE, rec(b"x", b"AAACGG") + rec(b"y", b"AAAAGG") + rec(b"z", b"AAATGG"), None, {},
         [NONE + (AMBIGUOUS,), (0, 0, 0, ASSIGNED), (1, 0, 0, ASSIGNED)], rec(b"y", b"GG") + rec(b"z", b"GG") + rec(b"x", b"AAACGG"), units=[1, 1, 1],
         ambiguous=1, perfect=2, undetermined=1),
    case("a tie without a mismatch allowed is no match at all", TIE, rec(b"x", b"AAACGG"), None, dict(mismatches=0), [NONE + (UNMATCHED,)], rec(b"x", b"AAACGG"),
         units=[0, 0, 1]),
    case("a longer barcode beats its prefix, a smaller t beats a longer barcode", PREFIX,
         rec(b"x", b"ACGTAAGG") + rec(b"y", b"ACGTACGG") + rec(b"z", b"ACGTA") + rec(b"w", b"ACGTATGG", b"ABCDEFGH"), None, {},
         [(1, 0, 0, ASSIGNED), (0, 0, 0, ASSIGNED), (0, 0, 0, ASSIGNED), (0, 0, 0, ASSIGNED)],
         rec(b"y", b"ACGG") + rec(b"z", b"A") + rec(b"w", b"ATGG", b"EFGH") + rec(b"x", b"GG"), units=[3, 1, 0], perfect=4, bases_clipped=18),
    case("header mode: no ':', ':' last, '+' first, last and twice", DUAL, b"".join(HEADER_READS), None, dict(header=True),
         [NONE + (NO_BARCODE,), NONE + (NO_BARCODE,), (0, 0, 0, ASSIGNED), NONE + (NO_BARCODE,), NONE + (NO_BARCODE,), (0, 0, 1, ASSIGNED), (0, 0, 1, ASSIGNED),
          NONE + (NO_BARCODE,), NONE + (NO_BARCODE,)],
         b"".join(HEADER_READS[i] for i in (2, 5, 6, 0, 1, 3, 4, 7, 8)), units=[3, 6], perfect=1, mismatched=2, no_barcode=6, bases_clipped=0, bases_out=54),
    case("header mode, a single-index sheet: the tail without a '+' is X1, X2 is not needed", ONE, b"".join(HEADER_READS), None, dict(header=True),
         [NONE + (NO_BARCODE,), NONE + (NO_BARCODE,), (0, 0, 0, ASSIGNED), NONE + (NO_BARCODE,), (0, 0, 0, ASSIGNED), (0, 0, 0, ASSIGNED), (0, 0, 0, ASSIGNED),
          (0, 0, 0, ASSIGNED), (0, 0, 0, ASSIGNED)],
         b"".join(HEADER_READS[i] for i in (2, 4, 5, 6, 7, 8, 0, 1, 3)), units=[6, 3]),
    case("header mode reads mate 1's header only", DUAL, rec(b"p 1:N:0:ACGT+TTGA", b"CCCC"), rec(b"p 2:N:0:GGGG+GGGG", b"AAAA"), dict(header=True),
         [(0, 0, 0, ASSIGNED)], rec(b"p 1:N:0:ACGT+TTGA", b"CCCC"), rec(b"p 2:N:0:GGGG+GGGG", b"AAAA"), units=[1, 0], pairs=1, reads_in=2),
    case("a single-index sheet ignores X2 and leaves mate 2 whole", ONE, rec(b"p/1", b"ACGTCC"), rec(b"p/2", b"GGGGGG"), {}, [(0, 0, 0, ASSIGNED)],
         rec(b"p/1", b"CC"), rec(b"p/2", b"GGGGGG"), units=[1, 0], bases_in=12, bases_out=8, bases_clipped=4),
    case("two barcodes: each mate loses its own, each within M on its own", DUAL,
         rec(b"p/1", b"ACGTCC") + rec(b"q/1", b"ACGACC") + rec(b"s/1", b"AGGACC"), rec(b"p/2", b"TTGAGGG") + rec(b"q/2", b"TTGCGGG") + rec(b"s/2", b"TTGAGGG"), {},
         [(0, 0, 0, ASSIGNED), (0, 1, 1, ASSIGNED), NONE + (UNMATCHED,)], rec(b"p/1", b"CC") + rec(b"q/1", b"CC") + rec(b"s/1", b"AGGACC"),
         rec(b"p/2", b"GGG") + rec(b"q/2", b"GGG") + rec(b"s/2", b"TTGAGGG"), units=[2, 1], perfect=1, mismatched=1, unmatched=1, bases_clipped=16),
    case("interleaved: one output, mate 1 then mate 2", DUAL, rec(b"u/1", b"GGGGGG") + rec(b"u/2", b"TTGAGGG") + rec(b"p/1", b"ACGTCC") + rec(b"p/2", b"TTGAGGG"), None,
         dict(interleaved=True), [NONE + (UNMATCHED,), (0, 0, 0, ASSIGNED)], rec(b"p/1", b"CC") + rec(b"p/2", b"GGG") + rec(b"u/1", b"GGGGGG") + rec(b"u/2", b"TTGAGGG"),
         units=[1, 1], pairs=2, reads_in=4, out2_bytes=0),
    case("keep-barcode", ONE, rec(b"r", b"ANGTTT"), None, dict(keep_barcode=True), [(0, 1, 0, ASSIGNED)], rec(b"r", b"ANGTTT"), units=[1, 0], bases_clipped=0, bases_out=6),
    case("\\r\\n comes out as \\n", ONE, b"@r\r\nACGTTT\r\n+\r\nIIIIII\r\n", None, {}, [(0, 0, 0, ASSIGNED)], b"@r\nTT\n+\nII\n", units=[1, 0], lines1=4),
    case("\\r\\n under a clip that takes as many bytes as the four \\r", [("a", "AC")], b"@r\r\nACGT\r\n+\r\nIIII\r\n@s\r\nACG\r\n+\r\nI\r\n", None, {},
         [(0, 0, 0, ASSIGNED), (0, 0, 0, ASSIGNED)], b"@r\nGT\n+\nII\n@s\nG\n+\n\n", units=[2, 0], bases_clipped=4),
    case("a last line without a newline gains one", ONE, b"@r\nACGTTT\n+\nIIIIII", None, {}, [(0, 0, 0, ASSIGNED)], b"@r\nTT\n+\nII\n", units=[1, 0]),
    case("a truncated last record has four lines all the same; a short quality line", ONE, b"@r\nACGTTT\n+x\nII\n@t\nACGTGG", None, {},
         [(0, 0, 0, ASSIGNED), (0, 0, 0, ASSIGNED)], b"@r\nTT\n+x\n\n@t\nGG\n\n\n", units=[2, 0], lines1=6, reads1=2),
    case("the surplus of the longer input is unpaired and goes nowhere", ONE, rec(b"p/1", b"ACGTCC") + rec(b"q/1", b"ACGTCC"), rec(b"p/2", b"GG"), {},
         [(0, 0, 0, ASSIGNED)], rec(b"p/1", b"CC"), rec(b"p/2", b"GG"), units=[1, 0], reads1=2, reads2=1, pairs=1, unpaired=1, units_in=1, reads_in=2, reads_out=2),
    case("no input", ONE, b"", None, {}, [], b"", units=[0, 0], units_in=0),
]


@pytest.mark.parametrize("c", HAND, ids=[c["name"] for c in HAND])
def test_checker_on_hand_worked_cases(c):
    w = demux_of(c["d1"], c["d2"], c["samples"], **c["kw"])
    assert w["recs"] == c["recs"]
    assert w["out1"] == c["out1"] and w["out2"] == c["out2"]
    assert [r["units"] for r in w["rows"]] == c["units"]
    for k, v in c["stats"].items():
        assert w[k] == v, (k, w[k], v)
    check_identities(w, w["rows"])


def test_rules_by_hand():
    assert candidates(b"@x") == (b"", b"") and candidates(b"@x:") == (b"", b"") and candidates(b"@a:b:CC+GG") == (b"CC", b"GG")
    assert candidates(b"@a:CC+GG+TT") == (b"CC", b"GG+TT") and candidates(b"@a+b:CC") == (b"CC", b"")
    sheet = [(b"a", b"ACGT", b""), (b"b", b"ACGTAA", b"")]
    assert assign(b"ACGTAA", b"", sheet, 1) == (1, 0, 0, ASSIGNED) and assign(b"ACGTAC", b"", sheet, 1) == (0, 0, 0, ASSIGNED)
    assert assign(b"ACG", b"", sheet, 3) == NONE + (NO_BARCODE,) and assign(b"TTTTTT", b"", sheet, 2) == NONE + (UNMATCHED,)      # (three of ACGT differ)
    # mismatches are counted per barcode, not together: 2 + 2 passes M = 2, 3 + 0 does not
    dual = [(b"a", b"AAAA", b"CCCC")]
    assert assign(b"AATT", b"CCGG", dual, 2) == (0, 2, 2, ASSIGNED) and assign(b"ATTT", b"CCCC", dual, 2) == NONE + (UNMATCHED,)


def test_symbols_declared_exported_and_listed(scfq):
    text = open(os.path.join(ROOT, "include", "sc_fqcount.h")).read() + open(os.path.join(ROOT, "include", "sc_fqcount_debug.h")).read()
    L = scfq.lib()
    for name in NEW_SYMBOLS:
        assert name + "(" in text and name in scfq.EXPORTS and hasattr(L, name), name
    for name in ("DemuxOpts", "DemuxStats", "DemuxRow", "DemuxRec", "demux_sheet", "demux_opts", "demux_device", "demux_host", "demux_file",
                 "format_demux_row_tsv", "demux_stages"):
        assert hasattr(scfq, name), name


def test_struct_layouts_and_c99_header(scfq, tmp_path):
    assert ctypes.sizeof(scfq.DemuxRec) == 8 and [getattr(scfq.DemuxRec, f).offset for f in ("sample", "mm1", "mm2", "state", "reserved")] == [0, 2, 3, 4, 5]
    assert ctypes.sizeof(scfq.DemuxRow) == 64 and scfq.DemuxRow.bytes1.offset == 32 and scfq.DemuxRow.off1.offset == 48
    assert ctypes.sizeof(scfq.DemuxOpts) == 24 and scfq.DemuxOpts.flags.offset == 8 and scfq.DemuxOpts.mismatches.offset == 12
    assert ctypes.sizeof(scfq.DemuxStats) == 29 * 8
    assert [getattr(scfq.DemuxStats, f).offset // 8 for f in ("reads1", "unpaired", "units_in", "mismatched", "reads_in", "bases_in", "out1_bytes", "flags", "dual")] == \
        [2, 9, 10, 17, 18, 20, 23, 25, 28]
    assert ctypes.sizeof(scfq.DemuxSample) == 3 * ctypes.sizeof(ctypes.c_void_p)
    src = tmp_path / "t.c"
    src.write_text('#include "sc_fqcount.h"\n#include "sc_fqcount_debug.h"\n'
                   "typedef char rec_is_8[sizeof(scfq_demux_rec) == 8 ? 1 : -1];\ntypedef char row_is_64[sizeof(scfq_demux_row) == 64 ? 1 : -1];\n"
                   "typedef char stats_are_29[sizeof(scfq_demux_stats) == 232 ? 1 : -1];\ntypedef char opts_are_24[sizeof(scfq_demux_opts) == 24 ? 1 : -1];\n"
                   "int main(void){ scfq_demux_sample s; scfq_demux_opts o; (void)s; (void)o; return SCFQ_DEMUX_MAX_SAMPLES == 1024 && SCFQ_DEMUX_NO_BARCODE == 3 ? 0 : 1; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)])


def sheet_error(scfq, samples):
    with pytest.raises(scfq.ScfqError) as e:
        scfq.demux_sheet(samples)
    assert e.value.rc == scfq.SCFQ_EARG
    return str(e.value)


def test_sheet_errors(scfq):
    """each with its text; the sheet never touches a device"""
    assert "0 samples: 1 .. 1024 are allowed" in sheet_error(scfq, [])
    assert "1025 samples" in sheet_error(scfq, [("s%d" % i, "ACGT") for i in range(1025)])
    assert "the name of sample 0 has 0 bytes" in sheet_error(scfq, [("", "ACGT")]) and "has 64 bytes: 1 .. 63" in sheet_error(scfq, [("n" * 64, "ACGT")])
    assert "sample 1 has no name" in sheet_error(scfq, [("a", "ACGT"), (None, "ACGA")])
    for bad in ("a b", "a/b", "a\tb", "a:b", "a+b", "\xe9"):
        assert "holds a byte other than A-Z a-z 0-9 . _ -" in sheet_error(scfq, [(bad, "ACGT")]), bad
    assert "starts with '.'" in sheet_error(scfq, [(".hidden", "ACGT")])
    assert "is named undetermined" in sheet_error(scfq, [("a", "ACGT"), ("undetermined", "ACGA")])
    assert "samples 0 and 2 are both named a" in sheet_error(scfq, [("a", "ACGT"), ("b", "ACGA"), ("a", "ACGG")])
    assert "sample 0 has no barcode1" in sheet_error(scfq, [("a", None)])
    assert "barcode1 of sample 0 has 0 letters" in sheet_error(scfq, [("a", "")]) and "barcode1 of sample 0 has 33 letters: 1 .. 32" in sheet_error(scfq, [("a", "A" * 33)])
    assert "barcode2 of sample 1 has 33 letters" in sheet_error(scfq, [("a", "ACGT", "A"), ("b", "ACGA", "C" * 33)])
    for bad in ("ACGN", "acgt", "ACG T", "ACGU"):
        assert "barcode1 of sample 0 holds a byte that is not A, C, G or T" in sheet_error(scfq, [("a", bad)]), bad
    assert "barcode2 of sample 0 holds a byte" in sheet_error(scfq, [("a", "ACGT", "ACGN")])
    assert "sample 1 has no second barcode, sample 0 has one" in sheet_error(scfq, [("a", "ACGT", "AC"), ("b", "ACGA")])
    assert "sample 1 has a second barcode, sample 0 has none" in sheet_error(scfq, [("a", "ACGT"), ("b", "ACGA", "AC")])
    assert "samples 0 and 1 have the same barcode ACGT" in sheet_error(scfq, [("a", "ACGT"), ("b", "ACGT")])
    assert "samples 0 and 1 have the same barcodes ACGT+AC" in sheet_error(scfq, [("a", "ACGT", "AC"), ("b", "ACGT", "AC")])
    # what is allowed: the same barcode1 with another barcode2, a barcode that is a prefix of another, every name byte, 32 letters, 1024 samples
    with scfq.demux_sheet([("a", "ACGT", "AC"), ("b", "ACGT", "AG"), ("Az09._-", "ACGTA", "A"), ("n" * 63, "T" * 32, "G" * 32)]) as sh:
        assert sh.n == 4 and sh.names == ["a", "b", "Az09._-", "n" * 63, "undetermined"]
    bases = "ACGT"
    with scfq.demux_sheet([("s%d" % i, "".join(bases[(i >> (2 * k)) & 3] for k in range(5))) for i in range(1024)]) as sh:
        assert sh.n == 1024 and sh.names[1023] == "s1023" and sh.names[1024] == "undetermined"
    L = scfq.lib()
    assert L.scfq_demux_sheet_new(None, 0, None) == scfq.SCFQ_EARG
    assert L.scfq_demux_sheet_samples(None) == 0 and L.scfq_demux_sheet_name(None, 0) is None
    L.scfq_demux_sheet_free(None)
    with scfq.demux_sheet(ONE) as sh:
        assert L.scfq_demux_sheet_name(sh.handle, 2) is None


def test_call_argument_errors(scfq):
    """each with its text and before any device call: this test runs without a device"""
    data = rec(b"r", b"ACGTACGT")
    single, dual = scfq.demux_sheet(ONE), scfq.demux_sheet(DUAL)

    def error(sheet, opts, d2=None, caps=(0, None)):
        with pytest.raises(scfq.ScfqError) as e:
            scfq.demux_host(sheet, data, d2, opts, caps=caps)
        assert e.value.rc == scfq.SCFQ_EARG
        return str(e.value)

    assert "unknown flag bits 0x8" in error(single, scfq.demux_opts(flags=0xF))
    assert "mismatches 4 is not in 0 .. 3" in error(single, scfq.demux_opts(mismatches=4))
    assert "a reserved word is not 0" in error(single, scfq.demux_opts(reserved=(0, 7)))
    assert "one input has no second output (out2)" in error(single, None, caps=(10, 10))
    assert "interleaved input takes no second buffer" in error(single, scfq.demux_opts(interleaved=True), d2=data)
    assert "the sheet is NULL" in error(None, None)
    assert "a sheet with second barcodes needs paired input in inline mode" in error(dual, None) and "needs paired input" in error(dual, scfq.demux_opts(keep_barcode=True))
    with pytest.raises(scfq.ScfqError) as e:
        scfq.demux_file(single, "/nonexistent.fq", opts=scfq.demux_opts(mismatches=9))
    assert e.value.rc == scfq.SCFQ_EARG and "mismatches 9" in str(e.value)
    with pytest.raises(scfq.ScfqError) as e:
        scfq.demux_device(single, 0, 0, row_cap=1)
    assert e.value.rc == scfq.SCFQ_EARG and "the rows hold 1 entries, the sheet needs 2" in str(e.value)
    with pytest.raises(scfq.ScfqError) as e:
        scfq.demux_file(dual, "/nonexistent.fq")
    assert e.value.rc == scfq.SCFQ_EARG and "needs paired input" in str(e.value)
    with pytest.raises(scfq.ScfqError) as e:
        scfq.demux_file(single, "/nonexistent.fq", "/nonexistent2.fq", scfq.demux_opts(interleaved=True))
    assert e.value.rc == scfq.SCFQ_EARG and "interleaved input takes no second file" in str(e.value)
    with pytest.raises(scfq.ScfqError) as e:
        scfq.demux_file(single, "/nonexistent.fq", out_dir="/nonexistent_dir")
    assert e.value.rc == scfq.SCFQ_EARG and "/nonexistent_dir is not a directory" in str(e.value)
    with pytest.raises(scfq.ScfqError) as e:
        scfq.demux_file(single, "/nonexistent.fq")
    assert e.value.rc == scfq.SCFQ_EOPEN
    # wrong struct sizes
    o = scfq.demux_opts()
    o.struct_size = 8
    with pytest.raises(scfq.ScfqError):
        scfq.demux_host(single, data, None, o, caps=(0, None))
    s = scfq.DemuxStats()
    rows = (scfq.DemuxRow * 2)()
    assert scfq.lib().scfq_demux_buffers(single.handle, None, 0, None, 0, 0, None, None, 0, rows, 2, None, 0, None, 0, 0, ctypes.byref(s)) == scfq.SCFQ_EARG


def test_row_formatter(scfq):
    s = scfq.DemuxStats()
    s.struct_size = ctypes.sizeof(scfq.DemuxStats)
    s.units_in, s.n_samples = 3, 1
    row = scfq.DemuxRow(2, 1, 1, 100, 300, 310, 0, 0)
    with scfq.demux_sheet(ONE) as single, scfq.demux_sheet([("a", "ACGT", "TTGA"), ("b", "ACGA", "TTGA")]) as dual:
        assert scfq.format_demux_row_tsv(s, single, 0, row) == "a\tACGT\t2\t66.66\t1\t1\t100\t300\t310"
        assert scfq.format_demux_row_tsv(s, single, 1, scfq.DemuxRow(1, 0, 0, 50, 150, 155, 300, 310)) == "undetermined\t-\t1\t33.33\t0\t0\t50\t150\t155"
        s.units_in = 0
        assert scfq.format_demux_row_tsv(s, single, 0, scfq.DemuxRow()) == "a\tACGT\t0\t0.00\t0\t0\t0\t0\t0"
        s.units_in, s.n_samples = 2, 2
        assert scfq.format_demux_row_tsv(s, dual, 1, row) == "b\tACGA+TTGA\t2\t100.00\t1\t1\t100\t300\t310"
        L = scfq.lib()
        buf = ctypes.create_string_buffer(8)
        assert L.scfq_format_demux_row_tsv(ctypes.byref(s), dual.handle, 1, ctypes.byref(row), buf, 8) == 36 and buf.value == b"b\tACGA+"
        for args in ((None, dual.handle, 0, ctypes.byref(row)), (ctypes.byref(s), None, 0, ctypes.byref(row)), (ctypes.byref(s), dual.handle, 3, ctypes.byref(row)),
                     (ctypes.byref(s), dual.handle, 0, None), (ctypes.byref(s), single.handle, 0, ctypes.byref(row))):
            assert L.scfq_format_demux_row_tsv(*args, buf, 8) == scfq.SCFQ_EARG


def test_cli_help_and_usage_errors(tmp_path):
    h = run("fq-demux", "--help")
    assert h.returncode == 0 and h.stderr == "" and "fq-demux [options] (--sheet=PATH | --sample=NAME:BC1[+BC2] ...) [--out-dir=DIR] IN.fq" in h.stdout
    for opt in ("--sheet=PATH", "--sample=NAME:BC1[+BC2]", "--out-dir=DIR", "--barcodes=inline|header", "--mismatches=N", "--keep-barcode", "--interleaved",
                "--per-read=PATH", "-t, --header", "-b, --basename", "-a, --absolute"):
        assert opt in h.stdout, opt
    assert run("fq-demux").stdout == h.stdout and run("fq-demux", "-h").stdout == h.stdout
    top = run("--help").stdout
    assert "fq-demux" not in top and "fq-count" in top           # the top-level help is pinned by tests/golden/cli_grammar.json
    sheet = "--sheet=" + os.path.join(DEMUX, "sheet.tsv")
    r1, r2 = os.path.join(DEMUX, "r1.fq"), os.path.join(DEMUX, "r2.fq")

    def usage(*args):
        r = run("fq-demux", *args)
        assert r.returncode == 1 and r.stdout == h.stdout, args
        return r.stderr

    assert "fq-demux needs its samples" in usage(r1) and "fq-demux needs its samples" in usage(sheet, "--sample=a:ACGT", r1)
    assert "Bad value for --mismatches: 4" in usage(sheet, "--mismatches=4", r1) and "Bad value for --mismatches: 01" in usage(sheet, "--mismatches=01", r1)
    assert "Bad value for --barcodes: index" in usage(sheet, "--barcodes=index", r1)
    assert "Bad value for --sample: a" in usage("--sample=a", r1) and "Bad value for --sample: :ACGT" in usage("--sample=:ACGT", r1)
    assert "Bad value for --sample: a:" in usage("--sample=a:", r1)
    assert "Unknown option: --sample" in usage("--sample", r1) and "Unknown option: --keep-barcode=1" in usage(sheet, "--keep-barcode=1", r1)
    assert "Unknown option: --out1=x" in usage(sheet, "--out1=x", r1)
    assert "takes one FASTQ, R1.fq and R2.fq" in usage(sheet, r1, r2, r1) and "takes one FASTQ" in usage(sheet, "--interleaved", r1, r2)
    r = run("fq-demux", sheet)
    assert r.returncode == 3 and "No FASTQ specified" in r.stderr
    # inputs, sheet and directory are looked at before anything is created, and the sheet's errors are the library's
    out = tmp_path / "out"
    out.mkdir()
    r = run("fq-demux", sheet, "--out-dir=%s" % out, str(tmp_path / "missing.fq"))
    assert r.returncode == 2 and "Unable to open file: " + str(tmp_path / "missing.fq") in r.stderr
    r = run("fq-demux", "--sheet=%s" % (tmp_path / "nothing.tsv"), "--out-dir=%s" % out, r1)
    assert r.returncode == 2 and "Unable to open file: " + str(tmp_path / "nothing.tsv") in r.stderr and r.stdout == ""
    r = run("fq-demux", sheet, "--out-dir=%s" % (tmp_path / "nowhere"), r1, r2)
    assert r.returncode == 1 and "Not a directory: " + str(tmp_path / "nowhere") in r.stderr
    for text, message in (("a\tACGT\nb\tACGN\n", "barcode1 of sample 1 holds a byte that is not A, C, G or T"), ("a\tACGT\n\n#c\na\tACGA\n", "samples 0 and 1 are both named a"),
                          ("a\tACGT\tAC\nb\tACGA\n", "sample 1 has no second barcode"), ("a\n", "line 1 is not name<TAB>barcode1"), ("a\tA\tC\tG\n", "line 1 is not"),
                          ("# nothing\n\n", "no sample"), ("undetermined\tACGT\r\n", "is named undetermined")):
        bad = tmp_path / "bad.tsv"
        bad.write_text(text)
        r = run("fq-demux", "--sheet=%s" % bad, "--out-dir=%s" % out, r1)
        assert r.returncode == 1 and message in r.stderr and r.stdout == "", (text, r.stderr)
    r = run("fq-demux", "--sample=a:ACGT+AC", "--sample=b:ACGT+AC", "--out-dir=%s" % out, r1, r2)
    assert r.returncode == 1 and "samples 0 and 1 have the same barcodes ACGT+AC" in r.stderr
    r = run("fq-demux", sheet, "--out-dir=%s" % out, r1)       # a dual sheet, one input, inline
    assert r.returncode == 1 and "needs paired input in inline mode" in r.stderr
    assert os.listdir(out) == []


def load_maker():
    spec = importlib.util.spec_from_file_location("make_demux", os.path.join(DEMUX, "make_demux.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_fixtures_are_what_their_script_writes():
    m = load_maker()
    files, two = m.build()
    on_disk = sorted(f for f in os.listdir(DEMUX) if f != "make_demux.py" and not f.startswith("__"))
    assert on_disk == sorted(files) and len(files) == 4 + 10 + 2
    for name, data in files.items():
        have = open(os.path.join(DEMUX, name), "rb").read()
        if name.endswith(".gz"):       # (the compressed bytes are zlib's business)
            have, data = gzip.decompress(have), gzip.decompress(data)
        assert have == data and len(have) < 64 << 10, name
    # the fixture holds what it is meant to hold
    b1 = [s[1] for s in m.SAMPLES]
    assert sum(x != y for x, y in zip(b1[0], b1[1])) == 2 and m.SAMPLES[0][2] == m.SAMPLES[1][2] and len(m.SAMPLES) == 4 and two["units_in"] <= 200
    assert min(two[k] for k in ("perfect", "mismatched", "no_barcode", "unmatched", "ambiguous", "bases_clipped")) > 0 and all(r["units"] for r in two["rows"])
    assert any(rec[1] and rec[2] and rec[3] == ASSIGNED for rec in two["recs"])                    # a mismatch in each barcode
    assert b"\n\n+\n\n" in two["out1"] and b"\n\n+\n\n" not in files["r1.fq"]                    # a mate that was all barcode
    # the checker's result is the files': per destination, and once more from the interleaved input
    one = demux_of(files["interleaved.fq"], None, m.SAMPLES, interleaved=True)
    assert one["recs"] == two["recs"] and [r["units"] for r in one["rows"]] == [r["units"] for r in two["rows"]]
    names = [s[0] for s in m.SAMPLES] + ["undetermined"]
    for d, name in enumerate(names):
        r = two["rows"][d]
        assert files[name + "_R1.fq"] == two["out1"][r["off1"]:r["off1"] + r["bytes1"]] and files[name + "_R2.fq"] == two["out2"][r["off2"]:r["off2"] + r["bytes2"]]
    assert files["report.tsv"].decode().splitlines() == [REPORT_HEADER] + report_text(two, m.SAMPLES)
    # the sheet file is the samples, as the command reads it
    rows = [line.split("\t") for line in files["sheet.tsv"].decode().splitlines() if line and not line.startswith("#")]
    assert [tuple(r) for r in rows] == list(m.SAMPLES)

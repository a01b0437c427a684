"""fq-screen without a device: the checker's own hand-worked cases, the two checkers against each other, the fixtures against the script
that makes them, every argument error of the library (each is decided before any device call) and the command's help and usage errors."""
import gzip
import importlib.util
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG
from _screen_check import (MAX_REFS, REPORT_HEADER, check_identities, contigs_of, decide, hits_of, index_of, index_of_np, key_of, pct_text, report_rows, same,
                           screen_of, screen_of_np, slots_of, windows_np)

SC = os.path.join(PKG, "sc")
SCREEN = os.path.join(GOLDEN, "screen")
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s):
    return s.translate(COMP)[::-1]


def run(*args):
    return subprocess.run([SC] + list(args), capture_output=True, text=True, stdin=subprocess.DEVNULL)


def fastq(seqs):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(seqs))


def test_keys_by_hand():
    # A=0 C=1 G=2 T=3, the first base on top: ACGTACGA is 0b00_01_10_11_00_01_10_00; its reverse complement TCGTACGT is larger
    assert key_of(b"ACGTACGA") == 0b0001101100011000
    assert key_of(b"TCGTACGT") == key_of(b"ACGTACGA")
    rng = np.random.default_rng(5)
    for k in (8, 9, 16, 31, 32):
        for _ in range(20):
            s = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), k))
            assert key_of(s) == key_of(revcomp(s)) < 1 << (2 * k)
    # a palindrome is its own reverse complement: both indexes are equal
    assert revcomp(b"ACGTACGT") == b"ACGTACGT" and key_of(b"ACGTACGT") == 0b0001101100011011
    # k = 32: all T is all ones forward, its reverse complement all A is 0 — the key an empty slot holds is never a k-mer's
    assert key_of(b"T" * 32) == 0 == key_of(b"A" * 32)
    assert key_of(b"G" * 32) == key_of(b"C" * 32) == int("01" * 32, 2)
    assert key_of(b"T" * 31 + b"G") == key_of(b"C" + b"A" * 31) == 1 << 62


def test_windows_np_agrees_with_key_of():
    rng = np.random.default_rng(6)
    a = rng.choice(np.frombuffer(b"ACGTACGTACGTNacgt", np.uint8), 400)
    for k in (8, 31, 32):
        key, valid = windows_np(a, k)
        assert key.size == 400 - k + 1
        for p in range(key.size):
            w = a[p:p + k].tobytes()
            ok = all(b in b"ACGT" for b in w)
            assert bool(valid[p]) == ok and (not ok or int(key[p]) == key_of(w)), (k, p)
    assert windows_np(a[:7], 8)[0].size == 0


def test_reference_rules_by_hand():
    # header lines break windows, line ends do not; lower case is upper-cased; '\r' and blanks are no sequence bytes
    fa = b"acgtacg\r\nTAC\r\n>two x\nGGGGGGGG\n>three\n>four\nAC GT\tAC\nGT"
    assert contigs_of(fa) == [b"ACGTACGTAC", b"GGGGGGGG", b"", b"ACGTACGT"]
    ix = index_of([("a", fa)], 8)
    assert ix["refs"][0] == dict(contigs=4, bases=26, windows=3 + 1 + 0 + 1, kmers=5, distinct=4, shared=0)      # ACGTACGT twice
    assert set(ix["keys"]) == {key_of(b"ACGTACGT"), key_of(b"CGTACGTA"), key_of(b"GTACGTAC"), key_of(b"GGGGGGGG")}
    # no window crosses the boundary of two contigs: the 8-mer that would is not in the index
    two = index_of([("a", b">1\nAAAACCCC\n>2\nGGGGTTTA\n")], 8)
    assert key_of(b"CCCCGGGG") not in two["keys"] and len(two["keys"]) == 2
    # an N breaks k-mers on both sides; a reference shorter than k has none
    n = index_of([("a", b">1\nACGTACGTNACGTACG\n"), ("b", b"ACGT")], 8)
    assert n["refs"][0]["windows"] == 9 and n["refs"][0]["kmers"] == 1 and n["refs"][1] == dict(contigs=1, bases=4, windows=0, kmers=0, distinct=0, shared=0)
    # shared keys, whichever strand a reference holds
    s = index_of([("a", b"ACGTTGCAAG"), ("b", revcomp(b"ACGTTGCAAG")), ("c", b"CGTTGCAAGG")], 8)
    assert [i["distinct"] for i in s["refs"]] == [3, 3, 3] and [i["shared"] for i in s["refs"]] == [3, 3, 2] and s["distinct"] == 4
    assert sorted(s["keys"].values()) == [0b011, 0b100, 0b111, 0b111]
    assert slots_of(0) == 1024 == slots_of(512) and slots_of(513) == 2048 and s["slots"] == 1024


def test_decision_by_hand():
    # the percent rule is an integer comparison: 7 of 70 k-mers are 10 percent, 6 of 70 are not 9 (600 < 630), 7 of 71 are not 10
    h = [0] * MAX_REFS
    h[2] = 7
    assert decide(70, h, 1, 10) == (0b100, 2, 7) and decide(71, h, 1, 10) == (0, 0xFF, 0)
    h[2] = 6
    assert decide(70, h, 1, 9) == (0, 0xFF, 0) and decide(70, h, 1, 8) == (0b100, 2, 6) and decide(70, h, 7, 0) == (0, 0xFF, 0)
    # min_hits 0 cannot be asked for, and no hit is never a match, even with 0 percent of 0 k-mers
    assert decide(0, [0] * MAX_REFS, 1, 0) == (0, 0xFF, 0)
    # best: the most hits, the lowest reference on a tie, among the matching ones only
    assert decide(50, [3, 9, 9, 2] + [0] * 12, 3, 0) == (0b0111, 1, 9)
    assert pct_text(1, 3) == "33.33" and pct_text(2, 3) == "66.66" and pct_text(0, 0) == "0.00" and pct_text(5, 5) == "100.00"


def test_reads_by_hand():
    ref = b"ACGTTGCAAGGCTTAACC"
    ix = index_of([("a", ref), ("b", b"TTTTTTTTTT")], 8)
    # forward, reverse complement, one N in the middle, lower case, shorter than k
    assert hits_of(ref, ix)[:2] == (11, 11) and hits_of(revcomp(ref), ix)[:2] == (11, 11)
    assert hits_of(ref[:8] + b"N" + ref[9:], ix)[:2] == (3, 3)      # the windows 0, 9 and 10
    assert hits_of(ref.lower(), ix)[:2] == (0, 0) and hits_of(ref[:7], ix)[:2] == (0, 0)
    assert hits_of(b"AAAAAAAAAAAA", ix) == (5, 5, [0, 5] + [0] * 14)      # the other strand of reference b
    w = screen_of(ix, fastq([ref, b"AAAAAAAAA", ref[:7], b"ACGTACGT" * 3, ref.lower()]), min_hits=2)
    assert w["recs"] == [(11, 11, 11, 1, 0), (2, 2, 2, 2, 1), (0, 0, 0, 0, 0xFF), (17, 0, 0, 0, 0xFF), (0, 0, 0, 0, 0xFF)]
    assert (w["reads_in"], w["reads_out"], w["matched_reads"], w["short_reads"], w["windows"], w["kmers"], w["skipped"]) == (5, 3, 2, 1, 11 + 2 + 0 + 17 + 11, 30, 11)
    assert w["out1"] == fastq([b"", b"", ref[:7], b"ACGTACGT" * 3, ref.lower()]).replace(b"@r0\n\n+\n\n@r1\n\n+\n\n", b"")
    check_identities(w)
    # a pair goes when either mate matches; keep_matched turns it round; the lines a last record does not have are not echoed
    r1, r2 = fastq([b"ACGTACGTAC", ref]), fastq([b"CCCCCCCCCC", b"GGGGGGGGGG"])[:-3]
    p = screen_of(ix, r1, r2)
    assert (p["pairs"], p["matched_pairs"], p["matched_reads"], p["dropped_reads"]) == (2, 1, 1, 2)
    assert p["out1"] == fastq([b"ACGTACGTAC"]) and p["out2"] == fastq([b"CCCCCCCCCC"])
    q = screen_of(ix, r1, r2, keep_matched=True)
    assert q["out1"] == b"@r1\n" + ref + b"\n+\n" + b"I" * 18 + b"\n" and q["out2"] == b"@r1\nGGGGGGGGGG\n+\nIIIIIIII\n"


def both(index, d1, d2=None, **kw):
    want = screen_of(index, d1, d2, **kw)
    a2 = None if d2 is None else np.frombuffer(bytes(d2), np.uint8)
    assert same(want, screen_of_np(index, np.frombuffer(bytes(d1), np.uint8), a2, **kw)), kw
    check_identities(want)
    return want


def load_maker():
    spec = importlib.util.spec_from_file_location("make_screen", os.path.join(SCREEN, "make_screen.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_fixtures_are_what_their_script_writes():
    m = load_maker()
    files, index, two = m.build()
    on_disk = sorted(f for f in os.listdir(SCREEN) if f != "make_screen.py" and not f.startswith("__"))
    assert on_disk == sorted(files)
    for name, data in files.items():
        have = open(os.path.join(SCREEN, name), "rb").read()
        if name.endswith(".gz"):       # (the compressed bytes are zlib's business)
            have, data = gzip.decompress(have), gzip.decompress(data)
        assert have == data, name
    # the fixture holds what it is meant to hold
    assert same(index, index_of_np([(n, files[n + ".fa"]) for n in m.NAMES], m.K))
    assert [i["shared"] for i in index["refs"]] == [0, 171, 171] and index["refs"][0]["contigs"] == 3
    assert two["multi_reads"] > 0 and two["short_reads"] > 0 and two["skipped"] > 0 and 0 < two["matched_pairs"] < two["pairs"]
    assert two["matched_reads"] < 2 * two["matched_pairs"]                         # pairs with one matching mate only
    hits = [r[1] for r in two["recs"]]
    assert m.PARAMS["min_hits"] - 1 in hits and m.PARAMS["min_hits"] in hits
    for kw in (dict(), dict(keep_matched=True), dict(min_hit_pct=30)):
        both(index, files["r1.fq"], files["r2.fq"], **dict(m.PARAMS, **kw))
    both(index, files["r1.fq"], **m.PARAMS)
    both(index, files["interleaved.fq"], interleaved=True, **m.PARAMS)
    assert files["report.tsv"].decode().splitlines() == [REPORT_HEADER] + report_rows(two, index)


def test_checkers_agree_on_odd_inputs():
    rng = np.random.default_rng(77)
    ref = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 600))
    for k in (8, 16, 31, 32):
        ix = index_of([("a", b">x\n" + ref[:300] + b"\n>y\n" + ref[300:]), ("b", ref[250:350])], k)
        assert same(ix, index_of_np([("a", b">x\n" + ref[:300] + b"\n>y\n" + ref[300:]), ("b", ref[250:350])], k))
        seqs = [b"", b"A", ref[:k - 1], ref[:k], ref[10:k + 11], revcomp(ref[280:320]), ref[260:340], b"N" * 40, ref[:64].lower(),
                bytes(b if i % 2 else ord("N") for i, b in enumerate(ref[:90]))]
        crlf = fastq(seqs).replace(b"\n", b"\r\n")
        for data in (fastq(seqs), crlf, fastq(seqs)[:-1], fastq(seqs) + b"@tail\nACGT"):
            both(ix, data, min_hits=2)
            both(ix, data, interleaved=True, keep_matched=True, min_hit_pct=50)
        both(ix, fastq(seqs), crlf[:-40], min_hits=1)
    both(ix, b"")
    both(ix, b"", b"", keep_matched=True)


@pytest.fixture(scope="module")
def refs():
    return [(n, open(os.path.join(SCREEN, n + ".fa"), "rb").read()) for n in ("spike", "vector", "rrna")]


def index_error(scfq, refs, k=31):
    with pytest.raises(scfq.ScfqError) as e:
        scfq.screen_index_host(refs, k)
    assert e.value.rc == scfq.SCFQ_EARG
    return str(e.value)


def test_index_argument_errors(scfq, refs, monkeypatch):
    """each with its text, and each before any device call: this test runs without a device"""
    assert "k = 7 is not in 8 .. 32" in index_error(scfq, refs, 7) and "k = 33" in index_error(scfq, refs, 33)
    assert "0 references: 1 .. 16 are allowed" in index_error(scfq, [])
    assert "17 references" in index_error(scfq, [("r%d" % i, b"ACGT") for i in range(17)])
    assert "has 0 bytes" in index_error(scfq, [("", b"ACGT")]) and "has 64 bytes" in index_error(scfq, [("x" * 64, b"ACGT")])
    for bad in ("a\tb", "a\nb", "a:b"):
        assert "holds a tab, a newline or a ':'" in index_error(scfq, [refs[0], (bad, b"ACGT")])
    assert "references 0 and 2 are both named spike" in index_error(scfq, [refs[0], refs[1], ("spike", refs[2][1])])
    for empty in (b"", b">only a header\n", b">a\n>b\n\r\n \n"):
        assert "reference 1 (e) is empty" in index_error(scfq, [refs[0], ("e", empty)])
    assert "more than 134217728 sequence bytes (reference 1)" in index_error(scfq, [refs[0], ("big", np.full((1 << 27) - 2000, ord("A"), np.uint8))])
    # a forced table has to have more slots than the references have windows (6781 here)
    monkeypatch.setenv("SCFQ_SCREEN_TABLE_BITS", "12")
    assert "SCFQ_SCREEN_TABLE_BITS=12" in index_error(scfq, refs) and "6781 windows" in index_error(scfq, refs)
    monkeypatch.delenv("SCFQ_SCREEN_TABLE_BITS")
    # a NULL handle, a wrong struct size
    h = scfq.ctypes.c_void_p()
    s = scfq.ScreenSummary()
    arr = (scfq.ScreenRef * 1)(scfq.ScreenRef(b"a", None, 0))
    assert scfq.lib().scfq_screen_index_buffers(arr, 1, 31, None, None) == scfq.SCFQ_EARG
    assert scfq.lib().scfq_screen_index_buffers(arr, 1, 31, scfq.ctypes.byref(h), scfq.ctypes.byref(s)) == scfq.SCFQ_EARG and not h.value
    assert scfq.lib().scfq_screen_index_summary(None, scfq.ctypes.byref(s)) == scfq.SCFQ_EARG
    assert scfq.lib().scfq_screen_ref_name(None, 0) is None
    scfq.lib().scfq_screen_index_free(None)
    with pytest.raises(scfq.ScfqError) as e:
        scfq.screen_index_files([os.path.join(SCREEN, "spike.fa")], ["a:b"])
    assert e.value.rc == scfq.SCFQ_EARG and "':'" in str(e.value)
    with pytest.raises(scfq.ScfqError) as e:
        scfq.screen_index_files([os.path.join(SCREEN, "spike.fa")] * 17)
    assert e.value.rc == scfq.SCFQ_EARG and "17 references" in str(e.value)
    with pytest.raises(scfq.ScfqError) as e:
        scfq.screen_index_files([os.path.join(SCREEN, "spike.fa")], k=5)
    assert e.value.rc == scfq.SCFQ_EARG and "k = 5" in str(e.value)


def test_call_argument_errors(scfq):
    data = fastq([b"ACGT" * 10])

    def error(opts, d2=None, caps=(0, None), index=None):
        with pytest.raises(scfq.ScfqError) as e:
            scfq.screen_host(index, data, d2, opts, caps=caps)
        assert e.value.rc == scfq.SCFQ_EARG
        return str(e.value)

    assert "unknown flag bits 0x4" in error(scfq.screen_opts(flags=0x7))
    assert "min_hits 0 is not in 1 .. 65535" in error(scfq.screen_opts(min_hits=0)) and "min_hits 65536" in error(scfq.screen_opts(min_hits=65536))
    assert "min_hit_pct 101 is not in 0 .. 100" in error(scfq.screen_opts(min_hit_pct=101))
    assert "the reserved word is 9, not 0" in error(scfq.screen_opts(reserved=9))
    assert "one input has no second output (out2)" in error(None, caps=(10, 10))
    assert "interleaved input takes no second buffer" in error(scfq.screen_opts(interleaved=True), d2=data)
    assert "the index is NULL" in error(None) and "the index is NULL" in error(scfq.screen_opts(keep_matched=True, min_hits=65535, min_hit_pct=100), d2=data, caps=(0, 0))
    with pytest.raises(scfq.ScfqError) as e:
        scfq.screen_file(None, "/nonexistent.fq", None, scfq.screen_opts(), out2_fd=1)
    assert e.value.rc == scfq.SCFQ_EARG and "out2" in str(e.value)
    with pytest.raises(scfq.ScfqError) as e:
        scfq.screen_file(None, "/nonexistent.fq")
    assert e.value.rc == scfq.SCFQ_EARG and "the index is NULL" in str(e.value)
    # wrong struct sizes, and the formatter without its arguments
    o = scfq.screen_opts()
    o.struct_size = 8
    with pytest.raises(scfq.ScfqError):
        scfq.screen_host(None, data, None, o, caps=(0, None))
    s = scfq.ScreenStats()
    assert scfq.lib().scfq_screen_buffers(None, None, 0, None, 0, 0, None, None, 0, None, 0, None, 0, 0, scfq.ctypes.byref(s)) == scfq.SCFQ_EARG
    assert scfq.lib().scfq_format_screen_row_tsv(scfq.ctypes.byref(s), None, 0, None, 0) == scfq.SCFQ_EARG


def test_cli_help_and_usage_errors(tmp_path):
    h = run("fq-screen", "--help")
    assert h.returncode == 0 and h.stderr == "" and "fq-screen [options] --ref=NAME:PATH [--ref=...] IN.fq" in h.stdout
    for opt in ("--ref=NAME:PATH", "--k=N", "--min-hits=N", "--min-hit-pct=N", "--keep-matched", "--interleaved", "--out=PATH", "--out1=PATH", "--out2=PATH",
                "--per-read=PATH", "-t, --header", "-b, --basename", "-a, --absolute"):
        assert opt in h.stdout, opt
    assert run("fq-screen").stdout == h.stdout and run("fq-screen", "-h").stdout == h.stdout
    assert "fq-screen" not in run("--help").stdout           # the top-level help is pinned by tests/golden/cli_grammar.json
    ref = "--ref=spike:" + os.path.join(SCREEN, "spike.fa")
    r1, r2 = os.path.join(SCREEN, "r1.fq"), os.path.join(SCREEN, "r2.fq")

    def usage(*args):
        r = run("fq-screen", *args)
        assert r.returncode == 1 and r.stdout == h.stdout, args
        return r.stderr

    assert "fq-screen needs a reference" in usage(r1)
    assert "Bad value for --k: 7" in usage(ref, "--k=7", r1) and "Bad value for --k: 33" in usage(ref, "--k=33", r1)
    assert "Bad value for --min-hits: 0" in usage(ref, "--min-hits=0", r1) and "Bad value for --min-hit-pct: 101" in usage(ref, "--min-hit-pct=101", r1)
    assert "Bad value for --ref: a\tb:x.fa" in usage("--ref=a\tb:x.fa", r1) and "Bad value for --ref: :x.fa" in usage("--ref=:x.fa", r1)
    assert "Bad value for --ref: " + "n" * 64 in usage("--ref=%s:x.fa" % ("n" * 64), r1)
    assert "Bad value for --ref: spike.fa" in usage(ref, "--ref=spike.fa", r1)                  # the same name twice
    assert "Bad value for --ref: r16:x" in usage(*(["--ref=r%d:x" % i for i in range(17)] + [r1]))
    assert "Unknown option: --ref" in usage("--ref", r1) and "Unknown option: --keep-matched=1" in usage(ref, "--keep-matched=1", r1)
    assert "takes one FASTQ, R1.fq and R2.fq" in usage(ref, r1, r2, r1) and "takes one FASTQ" in usage(ref, "--interleaved", r1, r2)
    assert "--out1=PATH and --out2=PATH go together" in usage(ref, "--out1=x", r1, r2)
    assert "R1.fq R2.fq write to --out1=PATH and --out2=PATH" in usage(ref, "--out=x", r1, r2)
    assert "one input is written to --out=PATH" in usage(ref, "--out1=x", "--out2=y", r1)
    r = run("fq-screen", ref)
    assert r.returncode == 3 and "No FASTQ specified" in r.stderr
    # inputs and references are looked at before anything is created
    out = tmp_path / "out.fq"
    r = run("fq-screen", ref, "--out=%s" % out, str(tmp_path / "missing.fq"))
    assert r.returncode == 2 and "Unable to open file: " + str(tmp_path / "missing.fq") in r.stderr and not out.exists()
    r = run("fq-screen", "--ref=%s" % (tmp_path / "nothing.fa"), "--out=%s" % out, r1)
    assert r.returncode == 2 and "Unable to open file: " + str(tmp_path / "nothing.fa") in r.stderr and not out.exists() and r.stdout == ""

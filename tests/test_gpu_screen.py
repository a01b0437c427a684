"""fq-screen on the device (csrc/scfq_screen.hip) against the checkers of tests/_screen_check.py: the index summaries, the per-read
table, the outputs compared with ==, byte for byte, every field of the statistics, and the bytes around every output buffer."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, PKG
from _screen_check import (REPORT_HEADER, assert_stats, assert_summary, check_identities, index_of, index_of_np, per_read_rows, report_rows, same, screen_of,
                           screen_of_np, stats_dict)
from test_gpu_parity import to_dev
from test_gpu_trim import Out, as_array, differ

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SC = os.path.join(PKG, "sc")
SCREEN = os.path.join(GOLDEN, "screen")
NAMES = ("spike", "vector", "rrna")
FA = [os.path.join(SCREEN, n + ".fa") for n in NAMES]
R1, R2, IL, R2GZ = (os.path.join(SCREEN, f) for f in ("r1.fq", "r2.fq", "interleaved.fq", "r2.fq.gz"))
FIXTURE = dict(min_hits=3)          # tests/golden/screen/make_screen.py's PARAMS
K = 31
WAVES, MAX_BLOCKS = 4, 2048         # of the lookup kernel (kScWaves, kScMaxBlocks): beyond their product a block makes a second round
LENGTHS = (0, 1, "k-1", "k", "k+1", 63, 64, 65, "64+k-1", 511, 512, 513, "512+k-1", "512+k", 1100)
COMP = bytes.maketrans(b"ACGT", b"TGCA")
REC = np.dtype([("kmers", "<u4"), ("hit_kmers", "<u4"), ("best_hits", "<u4"), ("mask", "<u2"), ("best", "u1"), ("reserved", "u1")])


def revcomp(s):
    return s.translate(COMP)[::-1]


def dna(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))


def fastq(seqs, eol=b"\n"):
    return b"".join(b"@r%d" % i + eol + s + eol + b"+" + eol + b"I" * len(s) + eol for i, s in enumerate(seqs))


def golden(name):
    return open(os.path.join(SCREEN, name), "rb").read()


@pytest.fixture(scope="module")
def fixture_index():
    """the checker's index of the fixture's references, computed once"""
    ix = index_of([(n, golden(n + ".fa")) for n in NAMES], K)
    assert same(ix, index_of_np([(n, golden(n + ".fa")) for n in NAMES], K))
    return ix


def check_device(torch, scfq, dindex, cindex, d1, d2=None, kw=None, ctx="", offs=(0, 0), out_offs=(1, 3), want=None, extra=7):
    """the device entry point on d1 / d2: the sizing call, then outputs of the reported sizes + extra bytes between sentinels and the
    per-read table between sentinels"""
    kw = kw or {}
    a1, a2 = as_array(d1), as_array(d2)
    if want is None:
        want = screen_of_np(cindex, a1, a2, **kw)
    check_identities(want)
    opts = scfq.screen_opts(**kw)
    t1, p1 = to_dev(torch, a1, offs[0])
    t2, p2 = to_dev(torch, a2, offs[1]) if a2 is not None else (None, None)
    n2 = a2.size if a2 is not None else 0
    assert_stats(scfq.screen_device(dindex, p1, a1.size, p2, n2, opts), want, (ctx, "sizing"))
    outs = [Out(torch, len(want["out1"]) + extra, out_offs[0]), Out(torch, len(want["out2"]) + extra, out_offs[1]) if a2 is not None else None]
    reads = want["reads_in"]
    table = Out(torch, 16 * reads + 16, 0)
    got = scfq.screen_device(dindex, p1, a1.size, p2, n2, opts, *[o.arg() if o else None for o in outs], recs=(table.ptr, reads))
    assert_stats(got, want, (ctx, kw, offs, out_offs))
    for k, o in zip(("out1", "out2"), outs):
        if o:
            differ(ctx, k, o.bytes(len(want[k])), want[k])
    recs = np.frombuffer(table.bytes(16 * reads), REC)
    have = [(int(r["kmers"]), int(r["hit_kmers"]), int(r["best_hits"]), int(r["mask"]), int(r["best"])) for r in recs]
    assert not recs["reserved"].any(), ctx
    if have != want["recs"]:
        at = next(i for i in range(reads) if have[i] != want["recs"][i])
        raise AssertionError((ctx, "read", at, have[at], want["recs"][at]))
    return want, got


def file_call(scfq, tmp_path, dindex, p1, p2, opts, which=(True, True), recs=None):
    paths = [tmp_path / ("out%d.fq" % k) for k in range(2)]
    fds = [os.open(str(p), os.O_WRONLY | os.O_CREAT | os.O_TRUNC) if w else -1 for p, w in zip(paths, which)]
    try:
        s = scfq.screen_file(dindex, p1, p2, opts, *fds, recs=recs)
    finally:
        for fd in fds:
            if fd >= 0:
                os.close(fd)
    return s, [p.read_bytes() if w else None for p, w in zip(paths, which)]


def every_entry_point(torch, scfq, tmp_path, dindex, cindex, r1, r2, kw, want, ctx, files):
    check_device(torch, scfq, dindex, cindex, r1, r2, kw, want=want, ctx=(ctx, "device"))
    opts = scfq.screen_opts(**kw)
    s, o1, o2 = scfq.screen_host(dindex, r1, r2, opts)
    assert_stats(s, want, (ctx, "host"))
    assert o1 == want["out1"] and (o2 == want["out2"] if r2 is not None else o2 is None), (ctx, "host")
    recs = (scfq.ScreenRec * want["reads_in"])()
    s, outs = file_call(scfq, tmp_path, dindex, files[0], files[1], opts, (True, r2 is not None), recs)
    assert_stats(s, want, (ctx, "file"))
    assert outs[0] == want["out1"] and (r2 is None or outs[1] == want["out2"]), (ctx, "file")
    assert [(x.kmers, x.hit_kmers, x.best_hits, x.mask, x.best) for x in recs] == want["recs"], (ctx, "file, per-read table")


def test_fixtures_every_entry_point(gpu, scfq, tmp_path, fixture_index):
    torch = gpu
    cindex = fixture_index
    r1, r2, il = golden("r1.fq"), golden("r2.fq"), golden("interleaved.fq")
    single, two, one = screen_of(cindex, r1, **FIXTURE), screen_of(cindex, r1, r2, **FIXTURE), screen_of(cindex, il, interleaved=True, **FIXTURE)
    kept = screen_of(cindex, r1, r2, keep_matched=True, **FIXTURE)
    assert (two["out1"], two["out2"], one["out1"]) == tuple(golden(f) for f in ("out1.fq", "out2.fq", "interleaved_out.fq"))
    with scfq.screen_index_files(FA) as dindex, scfq.screen_index_host([(n.upper(), golden(n + ".fa")) for n in NAMES]) as named:
        assert dindex.names == list(NAMES) and named.names == [n.upper() for n in NAMES] and dindex.k == K
        for ix in (dindex, named):
            assert_summary(ix.summary, cindex)
            assert int(ix.summary.slots) == cindex["slots"] and int(ix.summary.struct_size) == 8 * 102 and int(ix.summary.abi_version) > 0
        again = scfq.ScreenSummary()
        again.struct_size = scfq.ctypes.sizeof(scfq.ScreenSummary)
        assert scfq.lib().scfq_screen_index_summary(dindex.handle, scfq.ctypes.byref(again)) == 0
        assert_summary(again, cindex)
        every_entry_point(torch, scfq, tmp_path, dindex, cindex, r1, None, FIXTURE, single, "single", (R1, None))
        every_entry_point(torch, scfq, tmp_path, dindex, cindex, r1, r2, FIXTURE, two, "two", (R1, R2))
        every_entry_point(torch, scfq, tmp_path, dindex, cindex, r1, r2, FIXTURE, two, "two, gz", (R1, R2GZ))
        every_entry_point(torch, scfq, tmp_path, dindex, cindex, r1, r2, dict(FIXTURE, keep_matched=True), kept, "kept", (R1, R2))
        every_entry_point(torch, scfq, tmp_path, dindex, cindex, il, None, dict(FIXTURE, interleaved=True), one, "interleaved", (IL, None))
        check_device(torch, scfq, dindex, cindex, r1, r2, dict(min_hits=1, min_hit_pct=30), ctx="percent rule")
        opts = scfq.screen_opts(**FIXTURE)
        # only one output asked for; none at all
        s, o1, o2 = scfq.screen_host(dindex, r1, r2, opts, caps=(None, len(two["out2"]) + 9))
        assert_stats(s, two, "host, one output")
        assert (o1, o2) == (None, two["out2"])
        s, outs = file_call(scfq, tmp_path, dindex, R1, R2, opts, (False, True))
        assert_stats(s, two, "file, one output")
        assert outs == [None, two["out2"]]
        assert_stats(scfq.screen_file(dindex, R1, R2GZ, opts), two, "file, no output")
        assert len(scfq.screen_stages()) == 4 and dindex.build_ms() > 0
        # the report rows; the formatter's sizing convention
        rows = [scfq.format_screen_row_tsv(s, dindex, r) for r in range(4)]
        assert rows == report_rows(two, cindex) == golden("report.tsv").decode().splitlines()[1:]
        L = scfq.lib()
        for r, row in enumerate(rows):
            assert L.scfq_format_screen_row_tsv(scfq.ctypes.byref(s), dindex.handle, r, None, 0) == len(row)
            small = scfq.ctypes.create_string_buffer(b"\xff" * 16, 16)
            assert L.scfq_format_screen_row_tsv(scfq.ctypes.byref(s), dindex.handle, r, small, 8) == len(row)
            assert small.raw == row.encode()[:7] + b"\0" + b"\xff" * 8
        assert L.scfq_format_screen_row_tsv(scfq.ctypes.byref(s), dindex.handle, 4, None, 0) == scfq.SCFQ_EARG
        assert L.scfq_format_screen_row_tsv(None, dindex.handle, 0, None, 0) == scfq.SCFQ_EARG
        with scfq.screen_index_host([("a", b"ACGTACGTACGT")], 8) as other:       # statistics of another index
            assert L.scfq_format_screen_row_tsv(scfq.ctypes.byref(s), other.handle, 0, None, 0) == scfq.SCFQ_EARG
        # an output that is one byte too small: SCFQ_EARG that names it, the statistics complete, no byte written anywhere
        t1, p1 = to_dev(torch, as_array(r1), 1)
        t2, p2 = to_dev(torch, as_array(r2), 3)
        for name in ("out1", "out2"):
            outs = [Out(torch, len(two[o]) - (1 if o == name else 0), 1 + 2 * j) for j, o in enumerate(("out1", "out2"))]
            table = Out(torch, 16 * two["reads_in"], 0)
            with pytest.raises(scfq.ScfqError) as e:
                scfq.screen_device(dindex, p1, len(r1), p2, len(r2), opts, *[o.arg() for o in outs])
            assert e.value.rc == scfq.SCFQ_EARG and name in str(e.value), (name, str(e.value))
            assert str(len(two[name])) in str(e.value) and str(len(two[name]) - 1) in str(e.value), str(e.value)
            assert_stats(e.value.stats, two, ("too small", name))
            for o in outs:
                assert o.bytes(0) == b""
            with pytest.raises(scfq.ScfqError) as e:
                scfq.screen_host(dindex, r1, r2, opts, caps=tuple(len(two[o]) - (1 if o == name else 0) for o in ("out1", "out2")))
            assert e.value.rc == scfq.SCFQ_EARG and name in str(e.value)
            assert_stats(e.value.stats, two, ("too small, host", name))
        # a per-read table that is one entry too small: nothing is written to it or to the outputs
        outs = [Out(torch, len(two[o]), 1) for o in ("out1", "out2")]
        table = Out(torch, 16 * two["reads_in"], 0)
        with pytest.raises(scfq.ScfqError) as e:
            scfq.screen_device(dindex, p1, len(r1), p2, len(r2), opts, *[o.arg() for o in outs], recs=(table.ptr, two["reads_in"] - 1))
        assert e.value.rc == scfq.SCFQ_EARG and "per-read table holds %d entries" % (two["reads_in"] - 1) in str(e.value)
        assert table.bytes(0) == b"" and outs[0].bytes(0) == b"" and outs[1].bytes(0) == b""
        ti, pi = to_dev(torch, as_array(il), 2)
        out = Out(torch, len(one["out1"]) - 1, 5)
        with pytest.raises(scfq.ScfqError) as e:
            scfq.screen_device(dindex, pi, len(il), None, 0, scfq.screen_opts(interleaved=True, **FIXTURE), out.arg())
        assert e.value.rc == scfq.SCFQ_EARG and "out1" in str(e.value)
        assert_stats(e.value.stats, one, "too small, interleaved")
        assert out.bytes(0) == b""
        # inputs at every offset from a 256-byte boundary
        for off in range(4):
            check_device(torch, scfq, dindex, cindex, r1, r2, FIXTURE, want=two, ctx=("offset", off), offs=(off, 3 - off), out_offs=(off, off + 1))


def run(*args):
    return subprocess.run([SC] + list(args), capture_output=True, text=True, stdin=subprocess.DEVNULL)


def test_cli(gpu, tmp_path, fixture_index):
    cindex = fixture_index
    refs = ["--ref=%s:%s" % (n, p) for n, p in zip(NAMES, FA)]
    two = screen_of(cindex, golden("r1.fq"), golden("r2.fq"), **FIXTURE)
    report = golden("report.tsv").decode()
    o1, o2, pr = (str(tmp_path / f) for f in ("o1.fq", "o2.fq", "per_read.tsv"))
    r = run("fq-screen", *refs, "--min-hits=3", "--header", "--out1=" + o1, "--out2=" + o2, "--per-read=" + pr, R1, R2)
    assert (r.returncode, r.stderr) == (0, "") and r.stdout == report
    assert open(o1, "rb").read() == golden("out1.fq") and open(o2, "rb").read() == golden("out2.fq")
    assert open(pr).read().splitlines() == per_read_rows(two, cindex)
    # names from the file names, .gz input, no header, the file columns; reads go nowhere unless asked for
    r = run("fq-screen", *["--ref=" + p for p in FA], "--min-hits=3", "-b", R1, R2GZ)
    assert (r.returncode, r.stderr) == (0, "") and r.stdout == "".join(line + "\tr1.fq\n" for line in report.splitlines()[1:])
    kept = screen_of(cindex, golden("interleaved.fq"), interleaved=True, keep_matched=True, **FIXTURE)
    r = run("fq-screen", *refs, "--min-hits=3", "--interleaved", "--keep-matched", "--out=" + o1, IL)
    assert (r.returncode, r.stderr) == (0, "") and r.stdout.splitlines() == report_rows(kept, cindex) and open(o1, "rb").read() == kept["out1"]
    single = screen_of(index_of([(n, golden(n + ".fa")) for n in NAMES[:2]], 16), golden("r1.fq"), min_hit_pct=20)
    r = run("fq-screen", *refs[:2], "--k=16", "--min-hit-pct=20", "-t", "--out=" + o2, R1)
    assert (r.returncode, r.stderr) == (0, "") and open(o2, "rb").read() == single["out1"]
    assert r.stdout.splitlines() == [REPORT_HEADER] + report_rows(single, index_of([(n, golden(n + ".fa")) for n in NAMES[:2]], 16))
    # a reference that is rejected: the library's text, exit 1, and no output file
    empty = tmp_path / "empty.fa"
    empty.write_bytes(b">only a header\n")
    gone = str(tmp_path / "gone.fq")
    r = run("fq-screen", refs[0], "--ref=e:%s" % empty, "--out=" + gone, R1)
    assert r.returncode == 1 and "reference 1 (e) is empty" in r.stderr and r.stdout == "" and not os.path.exists(gone)


def length_of(spec, k):
    return spec if isinstance(spec, int) else eval(spec, {"k": k})


@pytest.mark.parametrize("k", (8, 16, 31, 32))
def test_read_lengths_and_chunk_boundaries(gpu, scfq, k):
    """every length of LENGTHS: random, drawn from the reference, with one k-mer of it at the first and at the last window and across
    every chunk boundary; reads that are all N, lower case, or every other byte invalid; one line of 50 000 bases"""
    rng = np.random.default_rng(400 + k)
    ref = dna(rng, 60000)
    fa = b">one\n" + b"\n".join(ref[i:i + 70] for i in range(0, 30000, 70)) + b"\n>two\n" + ref[30000:] + b"\n"
    cindex = index_of_np([("ref", fa), ("tail", b">t\n" + ref[59000:])], k)
    seqs = []
    for spec in LENGTHS:
        ln = length_of(spec, k)
        seqs.append(dna(rng, ln))
        seqs.append(ref[1000:1000 + ln])
        seqs.append(revcomp(ref[31000:31000 + ln]))
        seqs.append(b"N" * ln)
        seqs.append(ref[2000:2000 + ln].lower())
        seqs.append(bytes(b if i % 2 else ord("n") for i, b in enumerate(ref[3000:3000 + ln])))
        if ln >= k:
            base = bytearray(dna(rng, ln))
            first, last = bytearray(base), bytearray(base)
            first[:k] = ref[5000:5000 + k]
            last[ln - k:] = ref[59500:59500 + k]
            seqs += [bytes(first), bytes(last)]
            for edge in range(512, ln, 512):                  # a k-mer on each side of the boundary and every one across it
                plant = bytearray(base)
                lo, hi = max(edge - k, 0), min(edge + k, ln)
                plant[lo:hi] = revcomp(ref[7000:7000 + hi - lo])
                seqs.append(bytes(plant))
    long_ = bytearray(dna(rng, 50000))
    for edge in range(512, 50000, 512 * 7):
        long_[edge - k + 1:edge + 1] = ref[8000 + edge:8000 + edge + k]      # the window that ends at the chunk's last start
        long_[edge + 1:edge + 1 + k] = ref[100 + edge:100 + edge + k]
    long_[:k] = ref[:k]
    long_[-k:] = ref[-k:]
    seqs += [bytes(long_), ref[30000 - 25000:30000 + 25000]]        # (across the two contigs: no window of the reference crosses)
    data = fastq(seqs)
    with scfq.screen_index_host([("ref", fa), ("tail", b">t\n" + ref[59000:])], k) as dindex:
        assert_summary(dindex.summary, cindex, k)
        want, _ = check_device(gpu, scfq, dindex, cindex, data, None, dict(min_hits=1), ctx=("lengths", k))
        assert want["short_reads"] > 0 and want["multi_reads"] > 0 and want["skipped"] > 0 and 0 < want["reads_out"] < want["reads_in"]
        # the same reads as pairs, CRLF line ends, the percent rule
        check_device(gpu, scfq, dindex, cindex, fastq(seqs, b"\r\n"), None, dict(interleaved=True, min_hits=2, min_hit_pct=5), ctx=("lengths, pairs", k))


def test_index_edges(gpu, scfq):
    torch = gpu
    rng = np.random.default_rng(9)
    body = dna(rng, 300)
    reads = fastq([body[:100], revcomp(body[50:200]), dna(rng, 100), body[:31], body[1:32], body[:30]])

    def both(refs, k, kw=None):
        cindex = index_of(refs, k)
        with scfq.screen_index_host(refs, k) as dindex:
            assert_summary(dindex.summary, cindex, [n for n, _ in refs])
            return check_device(torch, scfq, dindex, cindex, reads, None, kw or {}, ctx=[n for n, _ in refs])[0], cindex

    # a reference shorter than k: no k-mer, the index is valid; alone, and beside one that has k-mers
    w, c = both([("short", body[:30])], 31)
    assert c["distinct"] == 0 and c["slots"] == 1024 and w["matched_reads"] == 0 and w["kmers"] > 0
    w, c = both([("short", b">s\nACGT\n"), ("body", body)], 31)
    assert w["ref_reads"][:2] == [0, 4]
    # a single k-mer; a contig of exactly k bases between others
    w, c = both([("one", b">x\n" + body[:31] + b"\n")], 31)
    assert c["distinct"] == 1 and w["matched_reads"] == 2 and w["hit_kmers"] == 2
    w, c = both([("three", b">a\nAC\n>b\n" + body[1:17] + b"\r\n" + body[17:32] + b"\r\n>c\n")], 31)
    assert c["refs"][0] == dict(contigs=3, bases=33, windows=1, kmers=1, distinct=1, shared=0) and w["matched_reads"] == 2
    # 16 references that all hold the same sequence: every key has the mask 0xFFFF, best is reference 0
    w, c = both([("r%d" % i, (body if i % 2 else revcomp(body))) for i in range(16)], 31, dict(min_hits=2))
    assert set(c["keys"].values()) == {0xFFFF} and w["multi_reads"] == w["matched_reads"] == 2 and w["ref_best_reads"] == [2] + [0] * 15
    assert {r[3] for r in w["recs"]} == {0, 0xFFFF}
    # k = 32 with the keys of both ends of the range: all A / all T (key 0) and all C / all G
    w, c = both([("poly", b">a\n" + b"T" * 40 + b"\n>c\n" + b"C" * 33)], 32)
    assert sorted(c["keys"]) == [0, int("01" * 32, 2)]
    cindex = index_of([("poly", b">a\n" + b"T" * 40 + b"\n>c\n" + b"C" * 33)], 32)
    with scfq.screen_index_host([("poly", b">a\n" + b"T" * 40 + b"\n>c\n" + b"C" * 33)], 32) as dindex:
        w = check_device(torch, scfq, dindex, cindex, fastq([b"A" * 40, b"G" * 32, b"T" * 31 + b"G" + b"T" * 31, b"A" * 31]), ctx="poly")[0]
        assert [r[1] for r in w["recs"]] == [9, 1, 0, 0]
    # a header-only FASTA is an empty reference
    with pytest.raises(scfq.ScfqError) as e:
        scfq.screen_index_host([("body", body), ("e", b">nothing\n")])
    assert e.value.rc == scfq.SCFQ_EARG and "reference 1 (e) is empty" in str(e.value)


def child(**env):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("SCFQ_SCREEN_")}
    r = subprocess.run([sys.executable, os.path.join(HERE, "_screen_child.py")], env=dict(clean, **env), capture_output=True, text=True)
    assert r.returncode == 0, (env, r.stdout + r.stderr)
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def child_default(fixture_index):
    """the fixture through a child process with no knob set, checked against the checker once"""
    got = child()
    want = screen_of(fixture_index, golden("r1.fq"), golden("r2.fq"), **FIXTURE)
    assert got["rc"] == 0 and got["stats"] == {k: want[k] for k in got["stats"]}
    assert got["out1"] == hashlib.sha256(want["out1"]).hexdigest() and got["out2"] == hashlib.sha256(want["out2"]).hexdigest()
    assert [tuple(r[:5]) for r in got["recs"]] == want["recs"] and not any(r[5] for r in got["recs"])
    assert got["summary"]["slots"] == fixture_index["slots"] == 16384
    return got


@pytest.mark.parametrize("env", (dict(SCFQ_SCREEN_TABLE_BITS="13"), dict(SCFQ_SCREEN_TABLE_BITS="13", SCFQ_SCREEN_PREFILTER="0"), dict(SCFQ_SCREEN_PREFILTER="0"),
                                 dict(SCFQ_SCREEN_PREFILTER="1"), dict(SCFQ_SCREEN_PREFILTER_KB="16"), dict(SCFQ_SCREEN_PREFILTER_KB="64")),
                         ids=lambda e: ",".join("%s=%s" % (k[12:], v) for k, v in e.items()))
def test_knobs_change_no_result(gpu, child_default, env):
    """the smallest legal table for the fixture's references (8192 slots for 6781 windows and 6522 keys: four slots in five are taken,
    the probe chains are long and wrap round the table's end), the prefilter off and on and at each size: records, outputs, statistics
    and the index summary are those of the automatic setting"""
    got = child(**env)
    slots = 8192 if "SCFQ_SCREEN_TABLE_BITS" in env else 16384
    assert got["summary"].pop("slots") == slots
    want = dict(child_default, summary={k: v for k, v in child_default["summary"].items() if k != "slots"})
    assert got == want


def test_table_too_small_is_an_error(gpu):
    """one bit fewer than the smallest legal table: SCFQ_EARG, at once"""
    got = child(SCFQ_SCREEN_TABLE_BITS="12")
    assert got["rc"] == -5 or "invalid argument" in got["text"], got
    assert "SCFQ_SCREEN_TABLE_BITS=12" in got["text"] and "6781 windows" in got["text"] and got["seconds"] < 5.0      # (decided on the host: no table is built, nothing can spin)
    assert child(SCFQ_SCREEN_PREFILTER_KB="48")["text"].count("16, 32 and 64 are allowed") == 1


@pytest.mark.parametrize("reads", (1, 31, 32, 33, WAVES * MAX_BLOCKS - 1, WAVES * MAX_BLOCKS + 1))
def test_partition_edges(gpu, scfq, reads):
    """read counts around a group of the write kernel and around the lookup kernel's second round, single-end and as pairs"""
    rng = np.random.default_rng(reads)
    ref = dna(rng, 500)
    refs = [("a", ref[:300]), ("b", ref[200:])]
    cindex = index_of_np(refs, 21)
    seqs = [(ref[int(at):int(at) + 40] if i % 3 == 0 else dna(rng, 40)) for i, at in enumerate(rng.integers(0, 460, reads))]
    with scfq.screen_index_host(refs, 21) as dindex:
        check_device(gpu, scfq, dindex, cindex, fastq(seqs), None, dict(), ctx=("single", reads))
        check_device(gpu, scfq, dindex, cindex, fastq(seqs), fastq(seqs[::-1] + [b"ACGT"]), dict(keep_matched=True), ctx=("two", reads))
        if reads < 100:
            check_device(gpu, scfq, dindex, cindex, fastq(seqs), None, dict(interleaved=True), ctx=("interleaved", reads))


def test_random_reads_against_the_numpy_checker(gpu, scfq):
    """a few thousand reads, a third drawn from the references with 0 - 3 substitutions, the rest random"""
    rng = np.random.default_rng(20261019)
    refs = [("r%d" % i, b">c\n" + dna(rng, int(n))) for i, n in enumerate((5000, 3000, 8000))]
    refs.append(("mix", b">m\n" + refs[0][1][1000:1400] + refs[2][1][500:900]))
    cindex = index_of_np(refs, 31)
    seqs = []
    for i in range(3000):
        ln = int(rng.integers(20, 260))
        if i % 3:
            seqs.append(dna(rng, ln))
            continue
        body = refs[int(rng.integers(0, 3))][1][3:]
        at = int(rng.integers(0, len(body) - ln))
        s = bytearray(body[at:at + ln])
        for _ in range(int(rng.integers(0, 4))):
            s[int(rng.integers(0, ln))] = int(rng.choice(np.frombuffer(b"ACGTN", np.uint8)))
        seqs.append(revcomp(bytes(s)) if i % 2 else bytes(s))
    r1, r2 = fastq(seqs[:1500]), fastq(seqs[1500:])
    with scfq.screen_index_host(refs, 31) as dindex:
        assert_summary(dindex.summary, cindex)
        w = check_device(gpu, scfq, dindex, cindex, r1, r2, dict(min_hits=2), ctx="random, two")[0]
        assert w["multi_reads"] > 0 and 0 < w["matched_pairs"] < w["pairs"]
        check_device(gpu, scfq, dindex, cindex, r1 + r2, None, dict(min_hits=5, min_hit_pct=40, keep_matched=True), ctx="random, single")

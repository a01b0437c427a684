"""fq-normalize on the device (csrc/scfq_norm.hip) against the checker of tests/_normalize_check.py: the per-read table, the
statistics, the histogram and the output bytes compared with ==, and the bytes around every output buffer.  The case sets that also
run under another environment live in _normalize_cases.py and run there through _normalize_child.py."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, PKG
from _kcount_check import kcount_of
from _normalize_check import HIST_HEADER, ROW_HEADER, assert_stats, hist_rows, normalize_of, recs_list, report_row
from _normalize_cases import BUILT_IN_C, Out, as_array, check_device, compare, device_table, dna, fastq, lengths, partition, rule, select, special_keys, table_of, to_dev

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SC = os.path.join(PKG, "sc")
NORM = os.path.join(GOLDEN, "normalize")
R1, R2, IL, R2GZ = (os.path.join(NORM, f) for f in ("r1.fq", "r2.fq", "interleaved.fq", "r2.fq.gz"))
K, BINS = 21, 1002
FIXTURE = dict(target=20, min_depth=3)         # tests/golden/normalize/make_normalize.py's settings
TWO_PASS = dict(k=K, canonical=True)


def golden(name):
    return open(os.path.join(NORM, name), "rb").read()


@pytest.fixture(scope="module")
def fixture_table():
    """the checker's table of the fixture's pairs, computed once"""
    return kcount_of([golden("r1.fq"), golden("r2.fq")], K, True).table


def file_call(scfq, tmp_path, table, p1, p2, opts, which=(True, True), recs=None, bins=0):
    paths = [tmp_path / ("out%d.fq" % k) for k in range(2)]
    fds = [os.open(str(p), os.O_WRONLY | os.O_CREAT | os.O_TRUNC) if w else -1 for p, w in zip(paths, which)]
    try:
        s, hist = scfq.norm_file(table, p1, p2, opts, *fds, recs=recs, bins=bins)
    finally:
        for fd in fds:
            if fd >= 0:
                os.close(fd)
    return s, hist, [p.read_bytes() if w else None for p, w in zip(paths, which)]


def every_entry_point(torch, scfq, tmp_path, dtable, ctable, r1, r2, kw, want, ctx, files):
    """device and host buffers and files, against the table given (dtable) and in the two-pass form (table = NULL)"""
    for table, extra in ((dtable, {}), (None, TWO_PASS)):
        where = (ctx, "a table" if table is not None else "two-pass")
        check_device(torch, scfq, table, ctable, K, True, r1, r2, want=want, ctx=(where, "device"), bins=BINS, two_pass=extra, **kw)
        opts = scfq.norm_opts(**dict(kw, **extra))
        s, hist, o1, o2 = scfq.norm_host(table, r1, r2, opts, bins=BINS)
        compare(scfq, s, hist, want, (where, "host"))
        assert o1 == want["out1"] and (o2 == want["out2"] if r2 is not None else o2 is None), (where, "host")
        recs = (scfq.NormRec * want["reads_in"])()
        s, hist, outs = file_call(scfq, tmp_path, table, files[0], files[1], opts, (True, r2 is not None), recs, BINS)
        compare(scfq, s, hist, want, (where, "file"))
        assert outs[0] == want["out1"] and (r2 is None or outs[1] == want["out2"]), (where, "file")
        assert recs_list(recs) == want["recs"], (where, "file, per-read table")
        assert int(s.passes) >= 1 and int(s.distinct) == len(ctable)


# ---- 1. entry points ------------------------------------------------------------------------------------------------------------
def test_fixtures_every_entry_point(gpu, scfq, tmp_path, fixture_table):
    torch = gpu
    ctable = fixture_table
    r1, r2, il = golden("r1.fq"), golden("r2.fq"), golden("interleaved.fq")
    two = normalize_of(ctable, K, True, r1, r2, bins=BINS, **FIXTURE)
    one = normalize_of(ctable, K, True, il, interleaved=True, bins=BINS, **FIXTURE)
    assert (two["out1"], two["out2"]) == (golden("out1.fq"), golden("out2.fq")) and one["recs"] == two["recs"] and one["classes"] == two["classes"]
    assert golden("report.tsv").decode() == ROW_HEADER + "\n" + report_row(two) + "\n"
    assert golden("hist.tsv").decode().splitlines() == [HIST_HEADER] + hist_rows(two["hist"])
    with device_table(scfq, [r1, r2], K, True) as dtable:
        every_entry_point(torch, scfq, tmp_path, dtable, ctable, r1, r2, FIXTURE, two, "two", (R1, R2))
        every_entry_point(torch, scfq, tmp_path, dtable, ctable, r1, r2, FIXTURE, two, "two, gz", (R1, R2GZ))
        every_entry_point(torch, scfq, tmp_path, dtable, ctable, il, None, dict(FIXTURE, interleaved=True), one, "interleaved", (IL, None))
        # single-end, against the pairs' table; its own two-pass form counts r1 alone
        single = normalize_of(ctable, K, True, r1, bins=BINS, **FIXTURE)
        check_device(torch, scfq, dtable, ctable, K, True, r1, want=single, ctx="single", bins=BINS, **FIXTURE)
        own = kcount_of(r1, K, True).table
        w1 = normalize_of(own, K, True, r1, bins=BINS, **FIXTURE)
        check_device(torch, scfq, None, own, K, True, r1, want=w1, ctx="single, two-pass", bins=BINS, two_pass=TWO_PASS, **FIXTURE)
        s, hist, outs = file_call(scfq, tmp_path, None, R1, None, scfq.norm_opts(**dict(FIXTURE, **TWO_PASS)), (True, False), None, BINS)
        compare(scfq, s, hist, w1, "single, two-pass, file")
        assert outs[0] == w1["out1"]
        # k given with a table: 0 or the table's; the report rows
        t1, p1 = to_dev(torch, as_array(r1))
        s, _ = scfq.norm_device(dtable, p1, len(r1), opts=scfq.norm_opts(k=K, **FIXTURE))
        assert_stats(s, single, "k = the table's")
        with pytest.raises(scfq.ScfqError) as e:
            scfq.norm_host(dtable, r1, r2, scfq.norm_opts(k=22))
        assert e.value.rc == scfq.SCFQ_EARG and "k = 22" in str(e.value) and "k = 21" in str(e.value)
        s, hist, o1, o2 = scfq.norm_host(dtable, r1, r2, scfq.norm_opts(**FIXTURE), bins=BINS)
        assert scfq.format_norm_row_tsv(s) == report_row(two)
        assert [scfq.format_norm_hist_tsv(d, int(a), int(b)) for d, (a, b) in enumerate(hist.tolist())] == hist_rows(two["hist"])
        assert len(scfq.norm_stages()) == 4
        # inputs at every offset from a 16-byte boundary
        for off in range(1, 4):
            check_device(torch, scfq, dtable, ctable, K, True, r1, r2, want=two, ctx=("offset", off), offs=(off, 3 - off), out_offs=(off, off + 1), bins=BINS, **FIXTURE)


def run(*args):
    return subprocess.run([SC] + list(args), capture_output=True, stdin=subprocess.DEVNULL)


def test_cli(gpu, tmp_path, fixture_table):
    """`sc fq-normalize` in a fresh process against the golden files"""
    o1, o2, per = (str(tmp_path / n) for n in ("o1.fq", "o2.fq", "per.tsv"))
    base = ["fq-normalize", "--k=21", "--target=20", "--min-depth=3"]
    r = run(*base, "-t", "--out1=" + o1, "--out2=" + o2, "--per-read=" + per, R1, R2GZ)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    assert r.stdout == golden("report.tsv") and open(o1, "rb").read() == golden("out1.fq") and open(o2, "rb").read() == golden("out2.fq")
    assert open(per, "rb").read() == golden("per_read.tsv")
    r = run(*base, "--header", "--hist", R1, R2)                                      # no output option: the report only
    assert r.returncode == 0 and r.stdout == golden("hist.tsv")
    two = normalize_of(fixture_table, K, True, golden("r1.fq"), golden("r2.fq"), bins=7, **FIXTURE)
    r = run(*base, "--hist=7", "-b", R1, R2)
    assert r.stdout.decode().splitlines() == [row + "\tr1.fq" for row in hist_rows(two["hist"])]
    # one interleaved input: the reads to stdout, the report to stderr with --stats; or to --out=PATH and the report to stdout
    r = run(*base, "--interleaved", "--stats", "-t", IL)
    il = b"".join(a + b for a, b in zip(split4(golden("out1.fq")), split4(golden("out2.fq"))))
    assert r.returncode == 0 and r.stdout == il and r.stderr == golden("report.tsv")
    r = run(*base, "--interleaved", IL)
    assert r.returncode == 0 and r.stdout == il and r.stderr == b""
    r = run(*base, "--interleaved", "--out=" + o1, IL)
    assert r.returncode == 0 and open(o1, "rb").read() == il and r.stdout == golden("report.tsv").split(b"\n", 1)[1]
    # single-end, plain mode, the other options
    r1 = golden("r1.fq")
    want = normalize_of(kcount_of(r1, 17, False).table, 17, False, r1, target=9, min_depth=2, weak_below=4, seed=77, keep_no_kmers=True)
    r = run("fq-normalize", "--k=17", "--plain", "--target=9", "--min-depth=2", "--weak-below=4", "--seed=77", "--keep-no-kmers", "--table-bits=16", "--stats", R1)
    assert r.returncode == 0 and r.stdout == want["out1"] and r.stderr.decode() == report_row(want) + "\n"
    # a failing call leaves no output file behind: a table that cannot hold the keys
    r = run(*base, "--table-bits=10", "--out1=" + o1, "--out2=" + o2, R1, R2)
    assert r.returncode == 1 and b"1024 slots" in r.stderr and not os.path.exists(o1) and not os.path.exists(o2)


def split4(data):
    lines = data.split(b"\n")[:-1]
    return [b"".join(x + b"\n" for x in lines[i:i + 4]) for i in range(0, len(lines), 4)]


# ---- 2. - 5., 8.: the case sets; those that depend on the windows a wave keeps in LDS also with SCFQ_NORM_LDS_WINDOWS=64 -------------
def child(*args, **env):
    clean = {k: v for k, v in os.environ.items() if not k.startswith(("SCFQ_NORM_", "SCFQ_KCOUNT_"))}
    r = subprocess.run([sys.executable, os.path.join(HERE, "_normalize_child.py")] + [str(a) for a in args], env=dict(clean, **env), capture_output=True, text=True)
    assert r.returncode == 0, (args, env, (r.stdout + r.stderr)[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_read_lengths(gpu, scfq):
    assert lengths(gpu, scfq, BUILT_IN_C) == 32


def test_read_lengths_counts_in_device_memory():
    """every read of more than 64 windows keeps its counts in device memory and selects from there: the same results"""
    assert child("cases", "lengths", 64, SCFQ_NORM_LDS_WINDOWS="64") == dict(rc=0, case="lengths", calls=32)


def test_select(gpu, scfq):
    assert select(gpu, scfq) == 2


def test_select_counts_in_device_memory():
    # (the least setting is 64: the reads of 65 and 130 windows take the other path)
    assert child("cases", "select", SCFQ_NORM_LDS_WINDOWS="1") == dict(rc=0, case="select", calls=2)


def test_special_keys(gpu, scfq):
    assert special_keys(gpu, scfq) == 4


def test_rule(gpu, scfq):
    assert rule(gpu, scfq) == 16


def test_partition(gpu, scfq):
    assert partition(gpu, scfq) == 17


# ---- 6. table states ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def child_default(fixture_table):
    """the fixture through a child process with no knob set, checked against the checker once"""
    got = child("fixture")
    want = normalize_of(fixture_table, K, True, golden("r1.fq"), golden("r2.fq"), bins=BINS, **FIXTURE)
    assert got["rc"] == 0 and got["stats"] == {k: want[k] for k in got["stats"]} and got["passes"] == 1
    assert got["out1"] == hashlib.sha256(want["out1"]).hexdigest() and got["out2"] == hashlib.sha256(want["out2"]).hexdigest()
    assert [tuple(r) for r in got["recs"]] == want["recs"] and got["hist"] == want["hist"]
    return got


def test_table_states(child_default, fixture_table):
    """growth through SCFQ_KCOUNT_START_BITS, long probe chains in a table one size above the keys, SCFQ_NORM_LDS_WINDOWS: the same
    results; a table that cannot hold the keys: SCFQ_EFULL through the two-pass form"""
    distinct = len(fixture_table)
    tight = distinct.bit_length()                     # the least power of two above the number of keys
    assert 1 << (tight - 1) <= distinct < 1 << tight and tight >= 11
    grown = child("fixture", SCFQ_KCOUNT_START_BITS="10")
    assert grown["passes"] > 1 and grown["slots"] > 1024
    chains = child("fixture", tight)
    assert chains["slots"] == 1 << tight and chains["passes"] == 1
    small = child("fixture", SCFQ_NORM_LDS_WINDOWS="64")
    for got in (grown, chains, small):
        for key in ("rc", "stats", "out1", "out2", "recs", "hist"):
            assert got[key] == child_default[key], key
    full = child("fixture", 10)
    assert full["rc"] == -10 and "1024 slots" in full["text"]


# ---- 7. outputs -----------------------------------------------------------------------------------------------------------------
def test_outputs(gpu, scfq, fixture_table):
    torch = gpu
    ctable = fixture_table
    r1, r2, il = golden("r1.fq"), golden("r2.fq"), golden("interleaved.fq")
    two = normalize_of(ctable, K, True, r1, r2, **FIXTURE)
    one = normalize_of(ctable, K, True, il, interleaved=True, **FIXTURE)
    opts = scfq.norm_opts(**FIXTURE)
    with device_table(scfq, [r1, r2], K, True) as dtable:
        # only one output asked for; none at all (the sizing call)
        s, _, o1, o2 = scfq.norm_host(dtable, r1, r2, opts, caps=(None, len(two["out2"]) + 9))
        assert_stats(s, two, "host, one output")
        assert (o1, o2) == (None, two["out2"])
        t1, p1 = to_dev(torch, as_array(r1), 1)
        t2, p2 = to_dev(torch, as_array(r2), 3)
        # an output that is one byte too small: SCFQ_EARG that names it, the statistics complete, no byte written anywhere
        for name in ("out1", "out2"):
            outs = [Out(torch, len(two[o]) - (1 if o == name else 0), 1 + 2 * j) for j, o in enumerate(("out1", "out2"))]
            with pytest.raises(scfq.ScfqError) as e:
                scfq.norm_device(dtable, p1, len(r1), p2, len(r2), opts, *[o.arg() for o in outs])
            assert e.value.rc == scfq.SCFQ_EARG and name in str(e.value), (name, str(e.value))
            assert str(len(two[name])) in str(e.value) and str(len(two[name]) - 1) in str(e.value), str(e.value)
            assert_stats(e.value.stats, two, ("too small", name))
            for o in outs:
                assert o.bytes(0) == b""
            with pytest.raises(scfq.ScfqError) as e:
                scfq.norm_host(dtable, r1, r2, opts, caps=tuple(len(two[o]) - (1 if o == name else 0) for o in ("out1", "out2")))
            assert e.value.rc == scfq.SCFQ_EARG and name in str(e.value)
            assert_stats(e.value.stats, two, ("too small, host", name))
        # a per-read table that is one entry too small: nothing is written to it or to the outputs
        outs = [Out(torch, len(two[o]), 1) for o in ("out1", "out2")]
        table = Out(torch, 16 * two["reads_in"], 0)
        for handle, extra in ((dtable, {}), (None, TWO_PASS)):
            with pytest.raises(scfq.ScfqError) as e:
                scfq.norm_device(handle, p1, len(r1), p2, len(r2), scfq.norm_opts(**dict(FIXTURE, **extra)), *[o.arg() for o in outs],
                                 recs=(table.ptr, two["reads_in"] - 1))
            assert e.value.rc == scfq.SCFQ_EARG and "per-read table holds %d entries" % (two["reads_in"] - 1) in str(e.value)
            assert table.bytes(0) == b"" and outs[0].bytes(0) == b"" and outs[1].bytes(0) == b""
        ti, pi = to_dev(torch, as_array(il), 2)
        out = Out(torch, len(one["out1"]) - 1, 5)
        with pytest.raises(scfq.ScfqError) as e:
            scfq.norm_device(dtable, pi, len(il), None, 0, scfq.norm_opts(interleaved=True, **FIXTURE), out.arg())
        assert e.value.rc == scfq.SCFQ_EARG and "out1" in str(e.value)
        assert_stats(e.value.stats, one, "too small, interleaved")
        assert out.bytes(0) == b""
        # the histogram at its least size, a small odd one, one around the depths that occur and the largest
        for bins in (2, 7, 21, 41, 2049, 4097, 1 << 20):
            want = normalize_of(ctable, K, True, r1, r2, bins=bins, **FIXTURE)
            s, hist = scfq.norm_device(dtable, p1, len(r1), p2, len(r2), opts, bins=bins)
            compare(scfq, s, hist, want, ("bins", bins))
            assert int(hist[:, 0].sum()) == want["units_in"] - 1 and int(hist[:, 1].sum()) == want["units_out"]
        # empty inputs
        for data in (b"", b"\n"):
            want = normalize_of(ctable, K, True, data, bins=3, **FIXTURE)
            s, hist, o1, o2 = scfq.norm_host(dtable, data, None, opts, bins=3)
            compare(scfq, s, hist, want, ("empty", data))
            assert o1 == want["out1"]


def test_deep_counts_beyond_the_lds_bins(gpu, scfq):
    """depths above the 2048 bins that the decision kernel keeps in LDS go to the histogram by global atomics"""
    rng = np.random.default_rng(5)
    k = 13
    a, b = dna(rng, 40), dna(rng, 40)
    counted = fastq([a] * 3000 + [b] * 2500)
    reads = fastq([a, b, a[:20] + b[:20], b] * 40)
    ctable = table_of(counted, k, False, big=True)
    with device_table(scfq, counted, k, False) as dtable:
        want, _ = check_device(gpu, scfq, dtable, ctable, k, False, reads, ctx="deep", bins=3001, target=2600, seed=9)
        assert want["hist"][3000][0] == 40 and want["hist"][2500][0] == 120 and 0 < want["hist"][3000][1] < 40 and want["hist"][2500][1] == 120
        check_device(gpu, scfq, dtable, ctable, k, False, reads, ctx="deep, last bin", bins=2600, target=2600, seed=9)

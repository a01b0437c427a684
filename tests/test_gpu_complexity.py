"""fq-complexity on the device (csrc/scfq_complexity.hip) against the checker of tests/_complexity_check.py: the statistics (every field),
the per-read table, the score histogram and both outputs compared with ==, and the bytes around every output buffer."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG
from _complexity_check import (FIELDS, MAX_LEN, NO_FIRST, SCORE_BINS, STATS_HEADER, TOO_LONG_REC, assert_stats, check_identities, complexity_of,
                               lengths_of, per_read_text, read_def, read_rows, stats_text)
from test_gpu_parity import to_dev
from test_gpu_trim import Out, as_array, differ

pytestmark = pytest.mark.gpu

SC = os.path.join(PKG, "sc")
CPLX = os.path.join(GOLDEN, "complexity")
R1, R2, IL, R2GZ = (os.path.join(CPLX, f) for f in ("r1.fq", "r2.fq", "interleaved.fq", "r2.fq.gz"))
FIXTURE = dict(max_masked_pct=30)                 # tests/golden/complexity/make_complexity.py's
WAVES, MAX_BLOCKS = 4, 4096                       # kCxWaves, kCxMaxBlocks: beyond their product a block of D1 makes a second round
LENGTHS = (0, 1, 2, 3, 4, 8, 9, 62, 63, 64, 65, 66, 127, 128, 129, 191, 192, 193, 511, 512, 513)
CACHE = {}                                        # the checker's per-read results, shared by every test of this file


def dna(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def planted(rng, n, unit, run, at):
    """n random bases with `unit` repeated over `run` bases from `at` on (cut at the end of the read)"""
    s = bytearray(dna(rng, n))
    s[at:at + run] = (unit * (run // len(unit) + 1))[:max(0, min(run, n - at))]
    return bytes(s)


def rec(tag, i, s, eol=b"\n"):
    return b"@%s%d" % (tag, i) + eol + s + eol + b"+" + eol + b"I" * len(s) + eol


def fq(seqs, eol=b"\n", tag=b"r"):
    return b"".join(rec(tag, i, s, eol) for i, s in enumerate(seqs))


def want_of(d1, d2=None, **kw):
    w = complexity_of(bytes(d1), None if d2 is None else bytes(d2), cache=CACHE, **kw)
    check_identities(w)
    return w


def recs_of(raw):
    return [tuple(int(v) for v in r) for r in np.frombuffer(raw, np.dtype("<u2")).reshape(-1, 4)]


def check_device(torch, scfq, d1, d2=None, kw=None, ctx="", want=None, offs=(0, 0), out_offs=(1, 3), extra=7):
    """the device entry point: the sizing call, then outputs of the reported sizes + extra bytes and a table of reads + 3 entries between
    sentinels"""
    kw = kw or {}
    want = want or want_of(d1, d2, **kw)
    a1, a2 = as_array(d1), as_array(d2)
    opts = scfq.cplx_opts(**kw)
    t1, p1 = to_dev(torch, a1, offs[0])
    t2, p2 = to_dev(torch, a2, offs[1]) if a2 is not None else (None, None)
    n2 = a2.size if a2 is not None else 0
    s, h = scfq.cplx_resident(p1, a1.size, p2, n2, opts)
    assert_stats(s, want, (ctx, "sizing"))
    assert h.tolist() == want["hist"], (ctx, "sizing, hist")
    outs = [Out(torch, len(want["out1"]) + extra, out_offs[0]), Out(torch, len(want["out2"]) + extra, out_offs[1]) if a2 is not None else None]
    table = Out(torch, 8 * (want["reads_in"] + 3), 8)
    s, h = scfq.cplx_resident(p1, a1.size, p2, n2, opts, *[o.arg() if o else None for o in outs], recs=(table.ptr, want["reads_in"] + 3))
    assert_stats(s, want, (ctx, kw, offs, out_offs))
    assert h.tolist() == want["hist"], (ctx, "hist")
    got = recs_of(table.bytes(8 * want["reads_in"]))
    assert got == want["recs"], (ctx, "recs", [(i, g, w) for i, (g, w) in enumerate(zip(got, want["recs"])) if g != w][:5])
    for k, o in zip(("out1", "out2"), outs):
        if o:
            differ(ctx, k, o.bytes(len(want[k])), want[k])
    return want


def check_host(scfq, d1, d2, kw, want, ctx):
    s, h, recs, o1, o2 = scfq.cplx_host(d1, d2, scfq.cplx_opts(**kw))
    assert_stats(s, want, (ctx, "host"))
    assert h.tolist() == want["hist"] and ([] if recs is None else recs_of(recs.tobytes())) == want["recs"], (ctx, "host")
    assert o1 == want["out1"] and (o2 == want["out2"] if d2 is not None else o2 is None), (ctx, "host")


def file_call(scfq, tmp_path, p1, p2, opts, which=(True, True)):
    """scfq_cplx_files into two files and a per-read table; returns (stats, hist, the contents or None, the table)"""
    paths = [tmp_path / ("out%d.fq" % k) for k in range(2)] + [tmp_path / "per_read.tsv"]
    fds = [os.open(str(p), os.O_WRONLY | os.O_CREAT | os.O_TRUNC) if w else -1 for p, w in zip(paths, tuple(which) + (True,))]
    try:
        s, h = scfq.cplx_files(p1, p2, opts, *fds)
    finally:
        for fd in fds:
            if fd >= 0:
                os.close(fd)
    return s, h, [p.read_bytes() if w else None for p, w in zip(paths, which)], paths[2].read_bytes()


def every_entry_point(torch, scfq, tmp_path, d1, d2, kw, ctx, files=None):
    want = check_device(torch, scfq, d1, d2, kw, ctx=(ctx, "device"))
    check_host(scfq, d1, d2, kw, want, ctx)
    if files is None:
        files = [tmp_path / "in1.fq", tmp_path / "in2.fq" if d2 is not None else None]
        for p, d in zip(files, (d1, d2)):
            if p is not None:
                p.write_bytes(bytes(d))
    s, h, outs, table = file_call(scfq, tmp_path, str(files[0]), None if files[1] is None else str(files[1]), scfq.cplx_opts(**kw), (True, d2 is not None))
    assert_stats(s, want, (ctx, "file"))
    assert h.tolist() == want["hist"], (ctx, "file, hist")
    assert outs[0] == want["out1"] and (d2 is None or outs[1] == want["out2"]), (ctx, "file")
    assert table.decode() == per_read_text(want, lengths_of(bytes(d1), None if d2 is None else bytes(d2), bool(kw.get("interleaved")))), (ctx, "file, per read")
    return want


def run(*args):
    return subprocess.run([SC] + [str(a) for a in args], capture_output=True, stdin=subprocess.DEVNULL)


def test_fixtures_every_entry_point(gpu, scfq, tmp_path):
    torch = gpu
    r1, r2, il = (open(p, "rb").read() for p in (R1, R2, IL))
    gold = {k: open(os.path.join(CPLX, k), "rb").read() for k in ("out1.fq", "out2.fq", "report.tsv", "hist.tsv", "per_read.tsv")}
    two = every_entry_point(torch, scfq, tmp_path, r1, r2, FIXTURE, "two", (R1, R2))
    assert (two["out1"], two["out2"]) == (gold["out1.fq"], gold["out2.fq"])
    every_entry_point(torch, scfq, tmp_path, r1, r2, FIXTURE, "two, gz", (R1, R2GZ))
    one = every_entry_point(torch, scfq, tmp_path, il, None, dict(FIXTURE, interleaved=True), "interleaved", (IL, None))
    assert one["recs"] == two["recs"] and one["hist"] == two["hist"]
    single = every_entry_point(torch, scfq, tmp_path, r1, None, FIXTURE, "single", (R1, None))
    assert len(scfq.cplx_stages()) == 4
    # only one output asked for
    s, h, recs, o1, o2 = scfq.cplx_host(r1, r2, scfq.cplx_opts(**FIXTURE), caps=(None, len(two["out2"]) + 9))
    assert_stats(s, two, "host, one output")
    assert (o1, o2) == (None, two["out2"])
    # the command
    o1, o2, pr = tmp_path / "c1.fq", tmp_path / "c2.fq", tmp_path / "c.tsv"
    r = run("fq-complexity", "-t", "--max-masked-pct=30", "--out1=%s" % o1, "--out2=%s" % o2, "--per-read=%s" % pr, R1, R2GZ)
    assert (r.returncode, r.stderr) == (0, b"") and r.stdout == gold["report.tsv"], r
    assert (o1.read_bytes(), o2.read_bytes(), pr.read_bytes()) == (gold["out1.fq"], gold["out2.fq"], gold["per_read.tsv"].split(b"\n", 1)[1])
    r = run("fq-complexity", "-t", "--hist", "--max-masked-pct=30", R1, R2)
    assert (r.returncode, r.stderr, r.stdout) == (0, b"", gold["hist.tsv"]), r
    r = run("fq-complexity", "--max-masked-pct=30", "--stats", R1)
    assert r.returncode == 0 and r.stdout == single["out1"] and r.stderr.decode() == stats_text(single) + "\n", r
    r = run("fq-complexity", "--max-masked-pct=30", "--interleaved", "--mask=n", IL)
    assert (r.returncode, r.stderr) == (0, b"") and r.stdout == want_of(il, interleaved=True, mask="n", **FIXTURE)["out1"]
    r = run("fq-complexity", "--report", "-t", "--max-masked-pct=30", R1)
    assert (r.returncode, r.stderr) == (0, b"") and r.stdout.decode() == STATS_HEADER + "\n" + stats_text(single) + "\n"
    # a failing call leaves no output file behind
    gone = tmp_path / "gone.fq"
    r = run("fq-complexity", "--out=%s" % gone, str(tmp_path / "in_that_is_not_there.fq"))
    assert r.returncode != 0 and not gone.exists()


def test_read_lengths(gpu, scfq):
    """every length three ways: a homopolymer, (AC)n, random sequence with one planted run; 513 is too long and echoed"""
    rng = np.random.default_rng(1)
    seqs = []
    for n in LENGTHS:
        seqs += [b"A" * n, (b"AC" * (n // 2 + 1))[:n], planted(rng, n, b"T", 14, n // 2)]
    data = fq(seqs)
    want = check_device(gpu, scfq, data, ctx="lengths")
    check_host(scfq, data, None, {}, want, "lengths")
    assert want["too_long"] == 3 and want["recs"][-1] == TOO_LONG_REC and want["hist"][SCORE_BINS - 1] == 3
    by_len = dict(zip(LENGTHS, want["recs"][::3]))
    assert by_len[3][0] == 0 and by_len[4] == (10, 0, NO_FIRST, 0) and by_len[8][0] == 30 and by_len[512] == (310, 512, 0, by_len[512][3])
    assert all(want["recs"][3 * k] == (read_rows(b"A" * n)[1], n, 0, read_rows(b"A" * n)[2]) for k, n in enumerate(LENGTHS) if 9 <= n <= MAX_LEN)
    # the definition itself on the short ones
    for s in seqs:
        if len(s) <= 66:
            assert read_def(s) == read_rows(s), s


def test_round_boundary(gpu, scfq):
    """runs that start at each position around the first and the second round boundary of a 192-base read: the intervals whose
    best(i + 1, j) comes from the round above; and runs that end exactly at the read's last base"""
    rng = np.random.default_rng(2)
    seqs = []
    for at in list(range(52, 67)) + list(range(116, 131)):
        seqs += [planted(rng, 192, b"G", 12, at), planted(rng, 192, b"AT", 20, at)]
    for n in (64, 65, 66, 67, 128, 130, 192):
        seqs += [planted(rng, n, b"C", 12, n - 12), planted(rng, n, b"AT", 20, n - 20), planted(rng, n, b"ACG", 30, n - 30)]
    data = fq(seqs)
    want = check_device(gpu, scfq, data, ctx="round boundary")
    assert all(r[1] >= 12 for r in want["recs"]), "every planted run is masked"
    for s in seqs[:2] + seqs[-2:]:
        assert read_def(s) == read_rows(s), s


def planted_set(rng, reads=48):
    seqs = []
    for i in range(reads):
        n = int(rng.integers(20, 200))
        unit = dna(rng, 1 + i % 6)
        seqs.append(planted(rng, n, unit, int(rng.integers(5, 61)), int(rng.integers(0, n))))
    return seqs


@pytest.mark.parametrize("window", (8, 16, 33, 64))
def test_parameters(gpu, scfq, window):
    data = fq(planted_set(np.random.default_rng(3)))
    masked = []
    for threshold in (1, 20, 150, 309, 310):
        want = check_device(gpu, scfq, data, kw=dict(window=window, threshold=threshold), ctx=("parameters", window, threshold))
        masked.append(want["masked_bases"])
    assert masked[0] > masked[1] >= masked[2] >= masked[3] >= masked[4] == 0, masked


def test_bytes(gpu, scfq):
    """N and lower case inside and next to runs; a read of only N"""
    rng = np.random.default_rng(4)
    a, b = dna(rng, 30), dna(rng, 30)
    seqs = [a + b"A" * 20 + b, a + b"A" * 9 + b"N" + b"A" * 10 + b, a + b"N" + b"A" * 20 + b"N" + b, a + b"A" * 9 + b"a" + b"A" * 10 + b,
            a + b"a" * 20 + b, a.lower() + b"A" * 20 + b.lower(), a + b"AC" * 12 + b"n" + b"AC" * 12 + b, b"N" * 50, b"N" * 3, b"n" * 70,
            a + b"A" * 6 + b"N" + b"A" * 6 + b, b"ACGTRYKM" * 10, bytes(range(33, 127)), b"A" * 40 + b"N" * 3 + b"A" * 40]
    data = fq(seqs)
    for mask in ("lower", "n"):
        want = check_device(gpu, scfq, data, kw=dict(mask=mask), ctx=("bytes", mask))
    assert [r[1] for r in want["recs"][7:10]] == [0, 0, 0] and want["recs"][0][1] >= 20 and want["recs"][1][1] >= 19 and want["recs"][4][1] == 0
    for s in seqs:
        assert read_def(s) == read_rows(s), s


def test_lines(gpu, scfq, tmp_path):
    rng = np.random.default_rng(5)
    seqs = planted_set(rng, 20)
    recs = [[b"@q%d some text" % i, s, b"+" + (b"q%d" % i if i % 3 == 0 else b""), b"I" * len(s)] for i, s in enumerate(seqs)]
    recs[1][3] = recs[1][3][:5]                    # a quality line shorter than the sequence, and longer ones
    recs[2][3] += b"JJJJJJJ"
    recs[3][3] = b""
    recs[4][3] = b"K" * 700
    lf = b"".join(line + b"\n" for r in recs for line in r)
    crlf = b"".join(line + b"\r\n" for r in recs for line in r)
    cases = dict(lf=lf, crlf=crlf, no_final_newline=lf[:-1], crlf_no_final_newline=crlf[:-2], cut_in_the_quality=lf[:-len(seqs[-1]) // 2 - 1],
                 three_lines=lf[:-len(seqs[-1]) - 1], two_lines=lf[:-len(seqs[-1]) - 3], one_line=lf[:lf.rindex(b"@q19") + 5], only_newlines=b"\n\n\n\n\n", empty=b"")
    for name, data in cases.items():
        want = check_device(gpu, scfq, data, ctx=("lines", name))
        check_host(scfq, data, None, {}, want, ("lines", name))
    want = want_of(lf)
    assert want["out1"].split(b"\n")[7] == recs[1][3] and want["out1"].split(b"\n")[19] == b"K" * 700 and want["masked_reads"] >= 5
    assert want_of(crlf)["out1"] == want["out1"]
    every_entry_point(gpu, scfq, tmp_path, crlf, cases["cut_in_the_quality"], {}, "lines, two files")


def test_mask_modes_and_the_drop_rule(gpu, scfq, tmp_path):
    rng = np.random.default_rng(6)
    s1, s2 = planted_set(rng, 70), planted_set(rng, 66)
    for i in range(0, 60, 4):
        s1[i] = dna(rng, 80)                       # mates without a mask next to mates with one
        s2[i + 1] = dna(rng, 90)
    r1, r2 = fq(s1, tag=b"a"), fq(s2, tag=b"b")
    il = b"".join(rec(b"a", i, s1[i]) + rec(b"b", i, s2[i]) for i in range(66)) + rec(b"a", 66, s1[66])
    modes = [check_device(gpu, scfq, r1, r2, dict(mask=m, max_masked_pct=50), ctx=("modes", m)) for m in ("none", "lower", "n")]
    assert all({k: w[k] for k in FIELDS if k != "mask"} == {k: modes[0][k] for k in FIELDS if k != "mask"} and w["recs"] == modes[0]["recs"] for w in modes)
    assert len({w["out1"] for w in modes}) == 3 and modes[0]["out1"].upper() == modes[1]["out1"].upper() and modes[0]["unpaired"] == 4
    assert modes[2]["out1"].count(b"N") > modes[0]["out1"].count(b"N")
    dropped = []
    for pct in (0, 10, 50, 100):
        w = every_entry_point(gpu, scfq, tmp_path, r1, r2, dict(max_masked_pct=pct), ("drop rule", pct))
        one = check_device(gpu, scfq, il, None, dict(max_masked_pct=pct, interleaved=True), ctx=("drop rule, interleaved", pct))
        assert one["recs"] == w["recs"] and one["unpaired"] == 1 and one["dropped_reads"] == w["dropped_reads"] and one["out1_bytes"] == w["out1_bytes"] + w["out2_bytes"]
        assert w["dropped_reads"] % 2 == 0 and w["low_reads"] <= w["dropped_reads"] <= 2 * w["low_reads"]
        dropped.append((w["low_reads"], w["dropped_reads"]))
        check_device(gpu, scfq, r2, None, dict(max_masked_pct=pct), ctx=("drop rule, single", pct))
    assert dropped[0][0] > dropped[1][0] > dropped[2][0] > dropped[3][0] == 0 and dropped[1][1] > dropped[1][0], dropped


def test_random_set(gpu, scfq):
    rng = np.random.default_rng(7)
    seqs = []
    for i in range(2000):
        n = int(rng.integers(30, 301))
        seqs.append(planted(rng, n, dna(rng, int(rng.integers(1, 7))), int(rng.integers(5, 61)), int(rng.integers(0, n))) if i % 3 == 0 else dna(rng, n))
    data = fq(seqs)
    want = check_device(gpu, scfq, data, ctx="random set", offs=(17, 0))
    with_mask = sum(1 for r in want["recs"] if r[1] > 0)
    assert with_mask >= 400 and 2000 - with_mask >= 400, with_mask
    check_device(gpu, scfq, data, kw=dict(max_masked_pct=20, mask="n"), ctx="random set, filtered")


def test_second_grid_round(gpu, scfq):
    """more reads than one pass of D1's grid holds; every fifth one a homopolymer, the others from a pool of 300 sequences"""
    rng = np.random.default_rng(8)
    reads = 20_000 if WAVES * MAX_BLOCKS == 16_384 else WAVES * MAX_BLOCKS * 5 // 4
    pool = [dna(rng, 24) for _ in range(300)]
    seqs = [bytes([b"ACGT"[i % 4]]) * 24 if i % 5 == 0 else pool[int(rng.integers(300))] for i in range(reads)]
    data = fq(seqs)
    want = check_device(gpu, scfq, data, ctx="second grid round", kw=dict(max_masked_pct=90))
    assert want["low_reads"] == reads // 5 and want["reads_in"] == reads > WAVES * MAX_BLOCKS


def test_capacities(gpu, scfq):
    torch = gpu
    r1, r2 = open(R1, "rb").read(), open(R2, "rb").read()
    want = want_of(r1, r2, **FIXTURE)
    a1, a2 = as_array(r1), as_array(r2)
    (t1, p1), (t2, p2) = to_dev(torch, a1, 0), to_dev(torch, a2, 0)
    opts = scfq.cplx_opts(**FIXTURE)
    n1, n2, reads = len(want["out1"]), len(want["out2"]), want["reads_in"]
    for c1, c2, cr, text in ((n1 - 1, n2, reads, "the out1 output holds %d bytes, the result has %d" % (n1 - 1, n1)),
                             (n1, n2 - 1, reads, "the out2 output holds %d bytes, the result has %d" % (n2 - 1, n2)),
                             (n1, n2, reads - 1, "the per-read table holds %d entries, the input has %d reads" % (reads - 1, reads))):
        outs, table = [Out(torch, c1), Out(torch, c2)], Out(torch, 8 * reads, 8)
        with pytest.raises(scfq.ScfqError) as e:
            scfq.cplx_resident(p1, a1.size, p2, a2.size, opts, outs[0].arg(), outs[1].arg(), recs=(table.ptr, cr))
        assert e.value.rc == scfq.SCFQ_EARG and text in str(e.value), str(e.value)
        assert_stats(e.value.stats, want, text)
        assert outs[0].bytes(0) == b"" and outs[1].bytes(0) == b"" and (cr == reads or table.bytes(0) == b"")      # (a table that fits may be filled)
        # the same with host memory
        with pytest.raises(scfq.ScfqError) as e:
            scfq.cplx_host(r1, r2, opts, caps=(c1, c2), recs_cap=cr)
        assert e.value.rc == scfq.SCFQ_EARG and text in str(e.value), str(e.value)
        assert_stats(e.value.stats, want, (text, "host"))
    # exactly enough
    outs, table = [Out(torch, n1), Out(torch, n2)], Out(torch, 8 * reads, 8)
    s, h = scfq.cplx_resident(p1, a1.size, p2, a2.size, opts, outs[0].arg(), outs[1].arg(), recs=(table.ptr, reads))
    assert (outs[0].bytes(n1), outs[1].bytes(n2), recs_of(table.bytes(8 * reads))) == (want["out1"], want["out2"], want["recs"])


def test_argument_errors(gpu, scfq):
    data = open(R1, "rb").read()

    def fails(text, d1, d2=None, opts=None, **kw):
        with pytest.raises(scfq.ScfqError) as e:
            scfq.cplx_host(d1, d2, opts, **kw)
        assert e.value.rc == scfq.SCFQ_EARG and text in str(e.value), (text, str(e.value))

    o = scfq.cplx_opts()
    o.struct_size -= 8
    with pytest.raises(scfq.ScfqError) as e:
        scfq.cplx_host(data, None, o)
    assert e.value.rc == scfq.SCFQ_EARG
    fails("unknown flag bits 0x6", data, opts=scfq.cplx_opts(flags=7))
    fails("the reserved words are 0, 0 and 9, not 0", data, opts=scfq.cplx_opts(reserved=(0, 0, 9)))
    fails("window 7 is not in 8 .. 64", data, opts=scfq.cplx_opts(window=7))
    fails("window 65 is not in 8 .. 64", data, opts=scfq.cplx_opts(window=65))
    fails("threshold 0 is not in 1 .. 310", data, opts=scfq.cplx_opts(threshold=0))
    fails("threshold 311 is not in 1 .. 310", data, opts=scfq.cplx_opts(threshold=311))
    fails("mask 3 is not in 0 .. 2", data, opts=scfq.cplx_opts(mask=3))
    fails("max_masked_pct 101 is not in 0 .. 100", data, opts=scfq.cplx_opts(max_masked_pct=101))
    fails("one input has no second output (out2)", data, caps=(10, 10))
    fails("interleaved input takes no second buffer", data, data, opts=scfq.cplx_opts(interleaved=True))
    s = scfq.CplxStats()                            # struct_size not set
    assert scfq.lib().scfq_cplx_buffers(None, 0, None, 0, 0, None, None, 0, None, None, 0, None, 0, 0, ctypes.byref(s)) == scfq.SCFQ_EARG

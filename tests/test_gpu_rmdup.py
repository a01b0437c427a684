"""fq-rmdup on the device (csrc/scfq_rmdup.hip) against the checker of tests/_rmdup_check.py: the statistics (every field but the two that
depend on the hash), the per-unit table, the histogram and both outputs compared with ==, and the bytes around every output buffer."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG
from _rmdup_check import FIELDS, HIST_BINS, STATS_HEADER, assert_stats, check_identities, per_read_text, rmdup_of, stats_text
from test_gpu_parity import to_dev
from test_gpu_trim import Out, as_array, differ

pytestmark = pytest.mark.gpu

SC = os.path.join(PKG, "sc")
RMDUP = os.path.join(GOLDEN, "rmdup")
EDGE = os.path.join(GOLDEN, "edge")
R1, R2, IL, R2GZ = (os.path.join(RMDUP, f) for f in ("r1.fq", "r2.fq", "interleaved.fq", "r2.fq.gz"))
FIXTURE = dict(prefix=50, swapped=True)           # tests/golden/rmdup/make_rmdup.py's
# the word (8 bytes), lane-group (64 bytes a step) and loop boundaries of U1 and U3, and a text far beyond them
LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 150, 511, 512, 513, 50_000)
PREFIXES = (1, 7, 8, 9, 64, 65, 65535)
DEFAULT_HASH_BITS = 40


def dna(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def rec(tag, i, s, eol=b"\n"):
    return b"@%s%d" % (tag, i) + eol + s + eol + b"+" + eol + b"I" * len(s) + eol


def fq(seqs, eol=b"\n", tag=b"r"):
    return b"".join(rec(tag, i, s, eol) for i, s in enumerate(seqs))


def want_of(d1, d2=None, **kw):
    w = rmdup_of(bytes(d1), None if d2 is None else bytes(d2), **kw)
    check_identities(w, w["hist"], w["recs"])
    return w


def recs_of(raw):
    return [tuple(int(v) for v in r) for r in np.frombuffer(raw, np.dtype("<u4")).reshape(-1, 2)]


def first_difference(got, want):
    return [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:5]


def check_device(torch, scfq, d1, d2=None, kw=None, ctx="", want=None, offs=(0, 0), out_offs=(1, 3), extra=7, hash_bits=0, place=to_dev):
    """the device entry point: the sizing call, then outputs of the reported sizes + extra bytes and a table of units + 3 entries between
    sentinels.  Returns (the checker's dict, the stats of the call)"""
    kw = kw or {}
    want = want or want_of(d1, d2, **kw)
    a1, a2 = as_array(d1), as_array(d2)
    opts = scfq.rmdup_opts(hash_bits=hash_bits, **kw)
    t1, p1 = place(torch, a1, offs[0])
    t2, p2 = place(torch, a2, offs[1]) if a2 is not None else (None, None)
    n2 = a2.size if a2 is not None else 0
    s, h = scfq.rmdup_resident(p1, a1.size, p2, n2, opts)
    assert_stats(s, want, (ctx, "sizing"))
    assert h.tolist() == want["hist"], (ctx, "sizing, hist")
    units = want["units_in"]
    outs = [Out(torch, len(want["out1"]) + extra, out_offs[0]), Out(torch, len(want["out2"]) + extra, out_offs[1]) if a2 is not None else None]
    table = Out(torch, 8 * (units + 3), 8)
    s, h = scfq.rmdup_resident(p1, a1.size, p2, n2, opts, *[o.arg() if o else None for o in outs], recs=(table.ptr, units + 3))
    assert_stats(s, want, (ctx, kw, offs, out_offs))
    assert int(s.hash_bits) == (hash_bits or DEFAULT_HASH_BITS)
    assert h.tolist() == want["hist"], (ctx, "hist")
    got = recs_of(table.bytes(8 * units))
    assert got == want["recs"], (ctx, "recs", first_difference(got, want["recs"]))
    check_identities({k: int(getattr(s, k)) for k in FIELDS}, h.tolist(), got)
    for k, o in zip(("out1", "out2"), outs):
        if o:
            differ(ctx, k, o.bytes(len(want[k])), want[k])
    return want, s


def check_host(scfq, d1, d2, kw, want, ctx):
    s, h, recs, o1, o2 = scfq.rmdup_host(d1, d2, scfq.rmdup_opts(**kw))
    assert_stats(s, want, (ctx, "host"))
    assert h.tolist() == want["hist"] and ([] if recs is None else recs_of(recs.tobytes())) == want["recs"], (ctx, "host")
    assert o1 == want["out1"] and (o2 == want["out2"] if d2 is not None else o2 is None), (ctx, "host")


def file_call(scfq, tmp_path, p1, p2, opts, which=(True, True)):
    """scfq_rmdup_files into two files and a per-unit table; returns (stats, hist, the contents or None, the table)"""
    paths = [tmp_path / ("out%d.fq" % k) for k in range(2)] + [tmp_path / "per_read.tsv"]
    fds = [os.open(str(p), os.O_WRONLY | os.O_CREAT | os.O_TRUNC) if w else -1 for p, w in zip(paths, tuple(which) + (True,))]
    try:
        s, h = scfq.rmdup_files(p1, p2, opts, *fds)
    finally:
        for fd in fds:
            if fd >= 0:
                os.close(fd)
    return s, h, [p.read_bytes() if w else None for p, w in zip(paths, which)], paths[2].read_bytes()


def every_entry_point(torch, scfq, tmp_path, d1, d2, kw, ctx, files=None):
    want, _ = check_device(torch, scfq, d1, d2, kw, ctx=(ctx, "device"))
    check_host(scfq, d1, d2, kw, want, ctx)
    if files is None:
        files = [tmp_path / "in1.fq", tmp_path / "in2.fq" if d2 is not None else None]
        for p, d in zip(files, (d1, d2)):
            if p is not None:
                p.write_bytes(bytes(d))
    s, h, outs, table = file_call(scfq, tmp_path, str(files[0]), None if files[1] is None else str(files[1]), scfq.rmdup_opts(**kw), (True, d2 is not None))
    assert_stats(s, want, (ctx, "file"))
    assert h.tolist() == want["hist"], (ctx, "file, hist")
    assert outs[0] == want["out1"] and (d2 is None or outs[1] == want["out2"]), (ctx, "file")
    assert table.decode() == per_read_text(want), (ctx, "file, per read")
    return want


def run(*args):
    return subprocess.run([SC] + [str(a) for a in args], capture_output=True, stdin=subprocess.DEVNULL)


def test_fixtures_every_entry_point(gpu, scfq, tmp_path):
    torch = gpu
    r1, r2, il = (open(p, "rb").read() for p in (R1, R2, IL))
    gold = {k: open(os.path.join(RMDUP, k), "rb").read() for k in ("out1.fq", "out2.fq", "report.tsv", "hist.tsv", "per_read.tsv")}
    two = every_entry_point(torch, scfq, tmp_path, r1, r2, FIXTURE, "two", (R1, R2))
    assert (two["out1"], two["out2"]) == (gold["out1.fq"], gold["out2.fq"])
    every_entry_point(torch, scfq, tmp_path, r1, r2, FIXTURE, "two, gz", (R1, R2GZ))
    one = every_entry_point(torch, scfq, tmp_path, il, None, dict(FIXTURE, interleaved=True), "interleaved", (IL, None))
    assert one["recs"] == two["recs"] and one["hist"] == two["hist"]
    single = every_entry_point(torch, scfq, tmp_path, r1, None, dict(prefix=50), "single", (R1, None))
    every_entry_point(torch, scfq, tmp_path, r1, r2, {}, "two, the defaults", (R1, R2))
    assert len(scfq.rmdup_stages()) == 7
    # only one output asked for
    s, h, recs, o1, o2 = scfq.rmdup_host(r1, r2, scfq.rmdup_opts(**FIXTURE), caps=(None, len(two["out2"]) + 9))
    assert_stats(s, two, "host, one output")
    assert (o1, o2) == (None, two["out2"])
    # the command
    o1, o2, pr = tmp_path / "c1.fq", tmp_path / "c2.fq", tmp_path / "c.tsv"
    r = run("fq-rmdup", "-t", "--prefix=50", "--swapped", "--out1=%s" % o1, "--out2=%s" % o2, "--per-read=%s" % pr, R1, R2GZ)
    assert (r.returncode, r.stderr) == (0, b"") and r.stdout == gold["report.tsv"], r
    assert (o1.read_bytes(), o2.read_bytes(), pr.read_bytes()) == (gold["out1.fq"], gold["out2.fq"], gold["per_read.tsv"].split(b"\n", 1)[1])
    r = run("fq-rmdup", "-t", "--hist", "--prefix=50", "--swapped", R1, R2)
    assert (r.returncode, r.stderr, r.stdout) == (0, b"", gold["hist.tsv"]), r
    r = run("fq-rmdup", "--prefix=50", "--stats", R1)
    assert r.returncode == 0 and r.stdout == single["out1"] and r.stderr.decode() == stats_text(single) + "\n", r
    o = tmp_path / "il.fq"
    r = run("fq-rmdup", "--prefix=50", "--swapped", "--interleaved", "--out=%s" % o, IL)
    assert (r.returncode, r.stderr) == (0, b"") and o.read_bytes() == one["out1"] and r.stdout.decode() == stats_text(one) + "\n"
    r = run("fq-rmdup", "--interleaved", IL)
    assert (r.returncode, r.stderr) == (0, b"") and r.stdout == want_of(il, interleaved=True)["out1"]
    r = run("fq-rmdup", "--report", "-t", "--prefix=50", R1)
    assert (r.returncode, r.stderr) == (0, b"") and r.stdout.decode() == STATS_HEADER + "\n" + stats_text(single) + "\n"
    # a failing call leaves no output file behind
    gone = tmp_path / "gone.fq"
    r = run("fq-rmdup", "--out=%s" % gone, str(tmp_path / "in_that_is_not_there.fq"))
    assert r.returncode != 0 and not gone.exists()


def length_set(rng):
    """at every length: a text, the text with another last byte, with another first byte, with one byte more (the text is a prefix of it), and
    the text once more"""
    texts = []
    for n in LENGTHS:
        b = dna(rng, n)
        texts.append(b)
        if n:
            texts.append(b[:-1] + (b"N" if b[-1:] != b"N" else b"A"))
            texts.append((b"n" if b[:1] != b"n" else b"a") + b[1:])
        texts += [b + b"R", b]
    return texts


_LENGTH_SET = {}


def length_cases():
    """the set as single-end input, as mate 1 beside one fixed mate 2, and as mate 2 beside one fixed mate 1; built once"""
    if not _LENGTH_SET:
        rng = np.random.default_rng(11)
        texts = length_set(rng)
        fixed = [dna(rng, 70)] * len(texts)
        _LENGTH_SET.update(texts=texts, single=(fq(texts), None), mate1=(fq(texts, tag=b"a"), fq(fixed, tag=b"b")), mate2=(fq(fixed, tag=b"a"), fq(texts, tag=b"b")))
    return _LENGTH_SET


@pytest.mark.parametrize("form", ("single", "mate1", "mate2"))
def test_text_lengths(gpu, scfq, form):
    case = length_cases()
    d1, d2 = case[form]
    want, _ = check_device(gpu, scfq, d1, d2, ctx=("lengths", form))
    # of the four or five units of a length exactly the last is a duplicate, of the first
    assert want["duplicate_units"] == len(LENGTHS) and want["max_copies"] == 2 and want["duplicated_classes"] == len(LENGTHS)
    texts = case["texts"]
    assert all((c == 0) == (u > 0 and texts[u] == texts[r] and r < u) for u, (r, c) in enumerate(want["recs"]))
    if form == "single":
        check_host(scfq, d1, None, {}, want, "lengths")
    else:
        check_device(gpu, scfq, d1, d2, kw=dict(swapped=True), ctx=("lengths, swapped", form))


@pytest.mark.parametrize("prefix", PREFIXES)
def test_prefix(gpu, scfq, prefix):
    case = length_cases()
    dups = []
    for form in ("single", "mate2"):
        d1, d2 = case[form]
        want, _ = check_device(gpu, scfq, d1, d2, kw=dict(prefix=prefix), ctx=("prefix", prefix, form))
        dups.append(want["duplicate_units"])
    # texts of more than `prefix` bytes that differ in their last byte or in their length are one key now
    longer = sum(1 for n in LENGTHS if n > prefix)
    assert dups[0] == dups[1] >= len(LENGTHS) + 2 * longer, (prefix, dups)


def test_class_sizes(gpu, scfq):
    """classes of 1, 2, 63, 64, 65 and 5000 members between 3000 units that are alone"""
    rng = np.random.default_rng(12)
    sizes = (1, 2, 63, 64, 65, 5000)
    texts = [t for n in sizes for t in [dna(rng, 40)] * n] + [dna(rng, 40) for _ in range(3000)]
    texts = [texts[i] for i in rng.permutation(len(texts))]
    data = fq(texts)
    want, s = check_device(gpu, scfq, data, ctx="class sizes", offs=(5, 0))
    assert [want["hist"][n] for n in (1, 2, 63, 64, 65, 1024)] == [3001, 1, 1, 1, 1, 1] and want["max_copies"] == 5000 and sum(want["hist"]) == 3006
    # the same classes as pairs, every second pair with its mates exchanged
    m1 = [t if i % 2 else t[::-1] for i, t in enumerate(texts)]
    m2 = [t[::-1] if i % 2 else t for i, t in enumerate(texts)]
    both, _ = check_device(gpu, scfq, fq(m1, tag=b"a"), fq(m2, tag=b"b"), kw=dict(swapped=True), ctx="class sizes, swapped pairs")
    assert both["hist"] == want["hist"]
    plain, _ = check_device(gpu, scfq, fq(m1, tag=b"a"), fq(m2, tag=b"b"), ctx="class sizes, pairs")
    assert 2400 < plain["max_copies"] < 2600 and plain["units_out"] > want["units_out"]      # (the class of 5000 falls into its odd and its even members)


def numbered(texts):
    return b"".join(b"@%d\n%s\n+\n%s\n" % (i, t, b"#" * len(t)) for i, t in enumerate(texts))


def test_one_class_of_200000(gpu, scfq):
    """every unit is compared with ONE head; a compare with the earlier members of the run would not end in a test's time"""
    n = 200_000
    data = numbered([b"GGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGG"] * n)
    want, s = check_device(gpu, scfq, data, ctx="one class")
    assert (want["units_out"], want["max_copies"], want["hist"][HIST_BINS - 1], want["recs"][0], want["recs"][n - 1]) == (1, n, 1, (0, n), (0, 0))
    assert (int(s.collisions), int(s.rounds)) == (0, 1)


def test_200000_distinct_units(gpu, scfq):
    n = 200_000
    rng = np.random.default_rng(13)
    block = rng.integers(0, 4, (n, 40), dtype=np.uint8)
    texts = [r.tobytes() for r in np.frombuffer(b"ACGT", np.uint8)[block]]
    assert len(set(texts)) == n
    data = numbered(texts)
    want, s = check_device(gpu, scfq, data, ctx="distinct")
    assert (want["units_out"], want["duplicate_units"], want["max_copies"], want["hist"][1]) == (n, 0, 1, n)
    assert int(s.collisions) == 0 and int(s.rounds) <= 1, (int(s.collisions), int(s.rounds))


@pytest.mark.parametrize("form", ("single", "pairs", "swapped"))
def test_hash_bits(gpu, scfq, form):
    """few bits of the hash put many classes into one run: the rounds sort them out, and nothing but `collisions` and `rounds` shows it"""
    rng = np.random.default_rng(14)
    pool = [dna(rng, int(rng.integers(0, 90))) for _ in range(160)]
    pick = lambda: [pool[int(i)] for i in rng.integers(0, len(pool), 1200)]
    if form == "single":
        d1, d2, kw = fq(pick()), None, {}
    else:
        # mate 2 from a pool of six: pairs repeat, and with the mates exchanged in every third pair the flag finds more
        m1, m2 = pick(), [pool[int(i)] for i in rng.integers(0, 6, 1200)]
        for i in range(0, 1200, 3):
            m1[i], m2[i] = m2[i], m1[i]
        d1, d2, kw = fq(m1, tag=b"a"), fq(m2, tag=b"b"), dict(swapped=form == "swapped")
    want = want_of(d1, d2, **kw)
    assert 100 < want["units_out"] < 1200 and want["duplicated_classes"] > 50
    seen = {}
    for bits in (64, 1, 2, 4, 33):
        _, s = check_device(gpu, scfq, d1, d2, kw=kw, ctx=("hash bits", form, bits), want=want, hash_bits=bits)
        seen[bits] = (int(s.collisions), int(s.rounds))
        if bits <= 4:
            assert seen[bits][0] > 0 and seen[bits][1] >= 2, (bits, seen)
    assert seen[64] == (0, 1) and seen[33] == (0, 1), seen
    assert seen[1][1] >= seen[4][1], seen


def sentinel_room(fill):
    def place(torch, arr, offset=0, pad=4096):
        """arr at `offset` bytes past a 4 KiB boundary inside a room of `fill` bytes"""
        t = torch.full((2 * pad + 4096 + offset + arr.size,), fill, dtype=torch.uint8, device="cuda")
        base = t.data_ptr()
        start = ((base + pad + 4095) // 4096) * 4096 - base + offset
        t[start:start + arr.size] = torch.from_numpy(arr.copy())
        torch.cuda.synchronize()
        return t, base + start
    return place


@pytest.mark.parametrize("offset", range(16))
def test_input_edges(gpu, scfq, offset):
    """the input at base + offset inside a room of sentinel bytes, its last text ending at its last byte; the outputs at + offset and
    + 15 - offset.  A load past the input's end would read the sentinel"""
    rng = np.random.default_rng(15)
    for n in (1, 5, 8, 13, 64, 69):
        text = dna(rng, n)
        # 0xA5 behind the last text where "\n+\n" stands behind its twin: reading it would make the two equal units differ
        data = fq([dna(rng, 30), text, dna(rng, 20)]) + b"@last\n" + text
        want, _ = check_device(gpu, scfq, data, ctx=("edges, equal", offset, n), out_offs=(offset, 15 - offset), offs=(offset, 0), place=sentinel_room(0xA5))
        assert want["recs"][3] == (1, 0) and want["lines1"] == 14
        # 'G' behind the last text where its neighbour goes on with G: with prefix = n + 3 a key cut at the prefix instead of at the text's end,
        # or a tail that is not masked, would make the two different units equal
        data = fq([dna(rng, 30), text + b"GGGGGGGGGGGG", dna(rng, 20)]) + b"@last\n" + text
        want, _ = check_device(gpu, scfq, data, kw=dict(prefix=n + 3), ctx=("edges, different", offset, n), out_offs=(offset, 15 - offset), offs=(offset, 0),
                               place=sentinel_room(ord("G")))
        assert want["recs"][3] == (3, 1) and want["duplicate_units"] == 0
    # the same with the last text as mate 2 of the last pair
    text = dna(rng, 13)
    m1 = fq([text, dna(rng, 9), text], tag=b"a")
    m2 = fq([text, dna(rng, 9)], tag=b"b") + b"@last\n" + text
    want, _ = check_device(gpu, scfq, m1, m2, ctx=("edges, pairs", offset), out_offs=(15 - offset, offset), offs=(offset, 15 - offset), place=sentinel_room(0xA5))
    assert want["recs"] == [(0, 2), (1, 1), (0, 0)]


def test_lines(gpu, scfq, tmp_path):
    rng = np.random.default_rng(16)
    pool = [dna(rng, int(rng.integers(1, 120))) for _ in range(12)]
    seqs = [pool[int(i)] for i in rng.integers(0, 12, 40)]
    recs = [[b"@q%d some text" % i, s, b"+" + (b"q%d" % i if i % 3 == 0 else b""), b"I" * len(s)] for i, s in enumerate(seqs)]
    recs[1][3] = recs[1][3][:5]                    # quality lines that are not the sequence's length: they are echoed as they are
    recs[2][3] += b"JJJJJJJ"
    recs[3][3] = b""
    lf = b"".join(line + b"\n" for r in recs for line in r)
    crlf = b"".join(line + b"\r\n" for r in recs for line in r)
    head, (h, q_seq, p, q) = b"".join(line + b"\n" for r in recs[:-1] for line in r), recs[-1]
    cases = dict(lf=lf, crlf=crlf, no_final_newline=lf[:-1], crlf_no_final_newline=crlf[:-2], cut_in_the_quality=head + h + b"\n" + q_seq + b"\n" + p + b"\n" + q[:len(q) // 2],
                 three_lines=head + h + b"\n" + q_seq + b"\n" + p + b"\n", three_lines_no_newline=head + h + b"\n" + q_seq + b"\n" + p,
                 two_lines=head + h + b"\n" + q_seq + b"\n", sequence_at_the_end=head + h + b"\n" + q_seq, cut_in_the_sequence=head + h + b"\n" + q_seq[:len(q_seq) // 2],
                 one_line=head + h + b"\n", header_at_the_end=head + h, only_newlines=b"\n\n\n\n\n", empty=b"", mixed=crlf[:len(crlf) // 2] + lf)
    for name, data in cases.items():
        want, _ = check_device(gpu, scfq, data, ctx=("lines", name))
        check_host(scfq, data, None, {}, want, ("lines", name))
    want = want_of(lf)
    assert want["duplicate_units"] >= 20 and want_of(crlf)["out1"] == want["out1"] and want_of(crlf)["recs"] == want["recs"]
    # reads1 != reads2, and every line form as a second file
    every_entry_point(gpu, scfq, tmp_path, crlf, cases["cut_in_the_quality"], {}, "lines, two files")
    w = every_entry_point(gpu, scfq, tmp_path, lf, lf[:lf.index(b"@q30")], dict(swapped=True), "lines, fewer reads in the second file")
    assert (w["reads1"], w["reads2"], w["pairs"], w["unpaired"]) == (40, 30, 30, 10)
    w, _ = check_device(gpu, scfq, lf[:lf.index(b"@q7")], crlf, ctx="lines, fewer reads in the first file")
    assert (w["pairs"], w["unpaired"]) == (7, 33)
    w, _ = check_device(gpu, scfq, lf[:lf.index(b"@q7")], None, kw=dict(interleaved=True), ctx="lines, interleaved with an odd record")
    assert (w["pairs"], w["unpaired"]) == (3, 1)


def test_edge_files(gpu, scfq, tmp_path):
    """tests/golden/edge: CR LF, lone CR, blank lines, truncated records, a 50 000-byte line, bytes above 127"""
    for name in sorted(os.listdir(EDGE)):
        path = os.path.join(EDGE, name)
        if name.endswith(".gz"):
            continue
        data = open(path, "rb").read()
        want = every_entry_point(gpu, scfq, tmp_path, data, None, {}, ("edge", name), (path, None))
        if want["reads1"] >= 2:
            every_entry_point(gpu, scfq, tmp_path, data, None, dict(interleaved=True, swapped=True, prefix=9), ("edge, interleaved", name), (path, None))
            check_device(gpu, scfq, data, data[:len(data) // 2], ctx=("edge, beside its first half", name))
    long_line = open(os.path.join(EDGE, "long_line_50k.fq"), "rb").read()
    want, _ = check_device(gpu, scfq, long_line + long_line, ctx="the long line twice")
    assert want["duplicate_units"] == want["units_in"] // 2 and want["bases_in"] >= 100_000


def test_swapped(gpu, scfq):
    rng = np.random.default_rng(17)
    a, b, c = dna(rng, 100), dna(rng, 100), dna(rng, 37)
    m1 = [a, b, a, b, a, c, c, a, b"", a]
    m2 = [b, a, a, b, b, c, c, c, a, b""]
    r1, r2 = fq(m1, tag=b"a"), fq(m2, tag=b"b")
    plain, _ = check_device(gpu, scfq, r1, r2, ctx="swapped, without the flag")
    flag, _ = check_device(gpu, scfq, r1, r2, kw=dict(swapped=True), ctx="swapped, with the flag")
    assert plain["recs"] == [(0, 2), (1, 1), (2, 1), (3, 1), (0, 0), (5, 2), (5, 0), (7, 1), (8, 1), (9, 1)]
    assert flag["recs"] == [(0, 3), (0, 0), (2, 1), (3, 1), (0, 0), (5, 2), (5, 0), (7, 1), (8, 2), (8, 0)]
    il = b"".join(rec(b"a", i, x) + rec(b"b", i, y) for i, (x, y) in enumerate(zip(m1, m2)))
    one, _ = check_device(gpu, scfq, il, None, kw=dict(swapped=True, interleaved=True), ctx="swapped, interleaved")
    assert one["recs"] == flag["recs"]
    # mates that agree up to the prefix only
    m1 += [a[:50] + c, b[:50] + c]
    m2 += [b[:50] + a, a[:50] + b]
    cut, _ = check_device(gpu, scfq, fq(m1, tag=b"a"), fq(m2, tag=b"b"), kw=dict(swapped=True, prefix=50), ctx="swapped, prefix")
    assert cut["recs"][10:] == [(0, 0), (0, 0)] and cut["recs"][0] == (0, 5)
    # a random mixture
    pool = [dna(rng, int(rng.integers(0, 40))) for _ in range(9)]
    x, y = ([pool[int(i)] for i in rng.integers(0, 9, 700)] for _ in range(2))
    mix, _ = check_device(gpu, scfq, fq(x, tag=b"a"), fq(y, tag=b"b"), kw=dict(swapped=True), ctx="swapped, mixture")
    assert mix["units_out"] <= 45                      # unordered pairs of nine keys
    mix, _ = check_device(gpu, scfq, fq(x, tag=b"a"), fq(y, tag=b"b"), ctx="pairs, mixture")
    assert 45 < mix["units_out"] <= 81


def test_laws(gpu, scfq):
    rng = np.random.default_rng(18)
    pool = [dna(rng, int(rng.integers(20, 150))) for _ in range(300)]
    pool += [t[:60] + dna(rng, 30) for t in pool[:100] if len(t) >= 60]
    x, y = ([pool[int(i)] for i in rng.integers(0, len(pool), 2000)] for _ in range(2))
    for d1, d2, kw in ((fq(x), None, {}), (fq(x, tag=b"a"), fq(y[:1990], tag=b"b"), dict(swapped=True)), (fq(x, tag=b"a"), fq(x[::-1], tag=b"b"), {})):
        whole, _ = check_device(gpu, scfq, d1, d2, kw=kw, ctx=("laws", kw))
        cut, _ = check_device(gpu, scfq, d1, d2, kw=dict(kw, prefix=60), ctx=("laws, prefix", kw))
        assert cut["duplicate_units"] >= whole["duplicate_units"] > 0
        for w, k in ((whole, kw), (cut, dict(kw, prefix=60))):
            assert sum(w["hist"]) == w["units_out"] and sum(c for _, c in w["recs"]) == w["units_in"]
            # once more over the output: nothing is removed, every byte is echoed
            again, s = check_device(gpu, scfq, w["out1"], w["out2"] if d2 is not None else None, kw=k, ctx=("laws, once more", k))
            assert again["duplicate_units"] == 0 and again["units_in"] == w["units_out"] and (again["out1"], again["out2"]) == (w["out1"], w["out2"])
            assert again["hist"][1] == w["units_out"] and int(s.rounds) == 0 == int(s.collisions)


def test_capacities(gpu, scfq):
    torch = gpu
    r1, r2 = open(R1, "rb").read(), open(R2, "rb").read()
    want = want_of(r1, r2, **FIXTURE)
    a1, a2 = as_array(r1), as_array(r2)
    (t1, p1), (t2, p2) = to_dev(torch, a1, 0), to_dev(torch, a2, 0)
    opts = scfq.rmdup_opts(**FIXTURE)
    n1, n2, units = len(want["out1"]), len(want["out2"]), want["units_in"]
    # the sizing call
    s, h = scfq.rmdup_resident(p1, a1.size, p2, a2.size, opts)
    assert_stats(s, want, "sizing")
    assert (int(s.out1_bytes), int(s.out2_bytes), h.tolist()) == (n1, n2, want["hist"])
    for c1, c2, cr, text in ((n1 - 1, n2, units, "the out1 output holds %d bytes, the result has %d" % (n1 - 1, n1)),
                             (n1, n2 - 1, units, "the out2 output holds %d bytes, the result has %d" % (n2 - 1, n2)),
                             (n1, n2, units - 1, "the per-unit table holds %d entries, the input has %d units" % (units - 1, units))):
        outs, table = [Out(torch, c1), Out(torch, c2)], Out(torch, 8 * units, 8)
        with pytest.raises(scfq.ScfqError) as e:
            scfq.rmdup_resident(p1, a1.size, p2, a2.size, opts, outs[0].arg(), outs[1].arg(), recs=(table.ptr, cr))
        assert e.value.rc == scfq.SCFQ_EARG and text in str(e.value), str(e.value)
        assert_stats(e.value.stats, want, text)
        assert outs[0].bytes(0) == b"" and outs[1].bytes(0) == b"" and (cr == units or table.bytes(0) == b"")      # (a table that fits may be filled)
        # the same with host memory
        with pytest.raises(scfq.ScfqError) as e:
            scfq.rmdup_host(r1, r2, opts, caps=(c1, c2), recs_cap=cr)
        assert e.value.rc == scfq.SCFQ_EARG and text in str(e.value), str(e.value)
        assert_stats(e.value.stats, want, (text, "host"))
    # exactly enough
    outs, table = [Out(torch, n1), Out(torch, n2)], Out(torch, 8 * units, 8)
    s, h = scfq.rmdup_resident(p1, a1.size, p2, a2.size, opts, outs[0].arg(), outs[1].arg(), recs=(table.ptr, units))
    assert (outs[0].bytes(n1), outs[1].bytes(n2), recs_of(table.bytes(8 * units))) == (want["out1"], want["out2"], want["recs"])
    # no table, one output
    outs = [Out(torch, n1), None]
    s, h = scfq.rmdup_resident(p1, a1.size, p2, a2.size, opts, outs[0].arg(), None)
    assert outs[0].bytes(n1) == want["out1"]


def test_argument_errors(gpu, scfq):
    data = open(R1, "rb").read()

    def fails(text, d1, d2=None, opts=None, **kw):
        with pytest.raises(scfq.ScfqError) as e:
            scfq.rmdup_host(d1, d2, opts, **kw)
        assert e.value.rc == scfq.SCFQ_EARG and text in str(e.value), (text, str(e.value))

    o = scfq.rmdup_opts()
    o.struct_size -= 8
    with pytest.raises(scfq.ScfqError) as e:
        scfq.rmdup_host(data, None, o)
    assert e.value.rc == scfq.SCFQ_EARG
    fails("unknown flag bits 0x4", data, opts=scfq.rmdup_opts(flags=5))
    fails("the reserved words are 0, 0 and 9, not 0", data, opts=scfq.rmdup_opts(reserved=(0, 0, 9)))
    fails("prefix 65536 is not in 0 .. 65535", data, opts=scfq.rmdup_opts(prefix=65536))
    fails("hash_bits 65 is not in 0 .. 64", data, opts=scfq.rmdup_opts(hash_bits=65))
    fails("single-end input has none", data, opts=scfq.rmdup_opts(swapped=True))
    fails("one input has no second output (out2)", data, caps=(10, 10))
    fails("interleaved input takes no second buffer", data, data, opts=scfq.rmdup_opts(interleaved=True))
    s = scfq.RmdupStats()                           # struct_size not set
    assert scfq.lib().scfq_rmdup_buffers(None, 0, None, 0, 0, None, None, 0, None, None, 0, None, 0, 0, ctypes.byref(s)) == scfq.SCFQ_EARG

"""fq-repair on the device (csrc/scfq_repair.hip) against the checker of tests/_repair_check.py: the statistics (every field but the ones
that depend on the hash or on the fast path), the per-record table and all four outputs compared with ==, and the bytes around every
output buffer."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG
from _repair_check import FIELDS, OUTPUTS, SINGLE, STATS_HEADER, assert_stats, check_identities, per_read_text, repair_of, stats_text
from test_gpu_trim import GUARD, SENTINEL, Out, as_array, differ

pytestmark = pytest.mark.gpu

SC = os.path.join(PKG, "sc")
REPAIR = os.path.join(GOLDEN, "repair")
EDGE = os.path.join(GOLDEN, "edge")
R1, R2, R2GZ = (os.path.join(REPAIR, f) for f in ("r1.fq", "r2.fq", "r2.fq.gz"))
GOLD = ("out1.fq", "out2.fq", "singles1.fq", "singles2.fq")
# the word (8 bytes), lane-group (64 bytes a step) and loop boundaries of P1, P2 and the compares, and a name far beyond them
LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 50_000)
DEFAULT_HASH_BITS = 40
LETTERS = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789:_-", np.uint8)


def rec(header, seq=b"ACGT", eol=b"\n"):
    """a record whose header line is "@" + header"""
    return b"@" + header + eol + seq + eol + b"+" + eol + b"I" * len(seq) + eol


def fq(headers, eol=b"\n", seqs=None):
    return b"".join(rec(h, b"ACGT" if seqs is None else seqs[i], eol) for i, h in enumerate(headers))


def numbered(n, tag=b"r", comment=b""):
    return [b"%s%d%s" % (tag, i, comment) for i in range(n)]


def place(torch, arr, offset=0, pad=4096):
    """device copy of arr `offset` bytes past a 256-byte boundary; the LAST byte of arr is the last byte of the room, sentinel bytes in
    front.  Returns (tensor, address, the check that the sentinels are intact)"""
    front = pad + offset
    t = torch.full((front + arr.size,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 256 == 0
    if arr.size:
        t[front:] = torch.from_numpy(arr.copy())
    torch.cuda.synchronize()

    def intact():
        h = t.cpu().numpy()
        assert (h[:front] == SENTINEL).all() and (h[front:] == arr).all(), "the input's room was written"
    return t, t.data_ptr() + front, intact


def first_difference(got, want):
    return [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:5]


def table_of(raw):
    return np.frombuffer(raw, np.dtype("<u4")).tolist()


def check_device(torch, scfq, d1, d2, ctx="", want=None, offs=(0, 0), out_offs=(1, 3, 5, 2), extra=7, hash_bits=0, path=None, sizing=True):
    """the device entry point: the sizing call, then outputs of the reported sizes + extra bytes and a table of reads1 + reads2 + 3 words
    between sentinels.  Returns (the checker's dict, the stats of the call)"""
    want = want or repair_of(bytes(d1), bytes(d2))
    a1, a2 = as_array(d1), as_array(d2)
    opts = scfq.repair_opts(hash_bits=hash_bits)
    t1, p1, intact1 = place(torch, a1, offs[0])
    t2, p2, intact2 = place(torch, a2, offs[1])
    if sizing:
        assert_stats(scfq.repair_resident(p1, a1.size, p2, a2.size, opts), want, (ctx, "sizing"), path)
    units = want["reads1"] + want["reads2"]
    outs = [Out(torch, len(w) + extra, off) for w, off in zip(want["outs"], out_offs)]
    table = Out(torch, 4 * (units + 3), 4)
    s = scfq.repair_resident(p1, a1.size, p2, a2.size, opts, [o.arg() for o in outs], table=(table.ptr, units + 3))
    assert_stats(s, want, (ctx, offs, out_offs), path)
    assert int(s.hash_bits) == (hash_bits or DEFAULT_HASH_BITS)
    got = table_of(table.bytes(4 * units))
    assert got == want["table"], (ctx, "table", first_difference(got, want["table"]))
    check_identities({k: int(getattr(s, k)) for k in FIELDS}, got)
    for name, o, w in zip(OUTPUTS, outs, want["outs"]):
        differ(ctx, name, o.bytes(len(w)), w)
    intact1()
    intact2()
    return want, s


def check_host(scfq, d1, d2, want, ctx):
    s, table, outs = scfq.repair_host(bytes(d1), bytes(d2))
    assert_stats(s, want, (ctx, "host"))
    assert ([] if table is None else table.tolist()) == want["table"], (ctx, "host, table")
    assert outs == want["outs"], (ctx, "host")


def file_call(scfq, tmp_path, p1, p2, opts=None, which=(True, True, True, True)):
    """scfq_repair_files into four files and a per-record table; returns (stats, the contents or None, the table)"""
    paths = [tmp_path / ("%s.fq" % n) for n in OUTPUTS] + [tmp_path / "per_read.tsv"]
    fds = [os.open(str(p), os.O_WRONLY | os.O_CREAT | os.O_TRUNC) if w else -1 for p, w in zip(paths, tuple(which) + (True,))]
    try:
        s = scfq.repair_files(p1, p2, opts, *fds)
    finally:
        for fd in fds:
            if fd >= 0:
                os.close(fd)
    return s, [p.read_bytes() if w else None for p, w in zip(paths, which)], paths[4].read_bytes()


def every_entry_point(torch, scfq, tmp_path, d1, d2, ctx, files=None):
    want, _ = check_device(torch, scfq, d1, d2, ctx=(ctx, "device"))
    check_host(scfq, d1, d2, want, ctx)
    if files is None:
        files = [tmp_path / "in1.fq", tmp_path / "in2.fq"]
        for p, d in zip(files, (d1, d2)):
            p.write_bytes(bytes(d))
    s, outs, table = file_call(scfq, tmp_path, str(files[0]), str(files[1]))
    assert_stats(s, want, (ctx, "file"))
    assert outs == want["outs"], (ctx, "file")
    assert table.decode() == per_read_text(want), (ctx, "file, per read")
    return want


def run(*args, env=None):
    return subprocess.run([SC] + [str(a) for a in args], capture_output=True, stdin=subprocess.DEVNULL, env=env)


# ---- the fixture --------------------------------------------------------------------------------------------------------------
def test_fixture_every_entry_point(gpu, scfq, tmp_path):
    torch = gpu
    r1, r2 = (open(p, "rb").read() for p in (R1, R2))
    gold = {k: open(os.path.join(REPAIR, k), "rb").read() for k in GOLD + ("report.tsv", "per_read.tsv")}
    want = every_entry_point(torch, scfq, tmp_path, r1, r2, "fixture", (R1, R2))
    assert want["outs"] == [gold[k] for k in GOLD] and want["in_step"] == 0
    every_entry_point(torch, scfq, tmp_path, r1, r2, "fixture, gz", (R1, R2GZ))
    assert len(scfq.repair_stages()) == 9
    # the command
    paths = [tmp_path / ("c_" + k) for k in GOLD]
    pr = tmp_path / "c.tsv"
    r = run("fq-repair", "-t", "--out1=%s" % paths[0], "--out2=%s" % paths[1], "--singles1=%s" % paths[2], "--singles2=%s" % paths[3], "--per-read=%s" % pr, R1, R2GZ)
    assert (r.returncode, r.stderr, r.stdout) == (0, b"", gold["report.tsv"])
    assert [p.read_bytes() for p in paths] == [gold[k] for k in GOLD] and pr.read_bytes() == gold["per_read.tsv"].split(b"\n", 1)[1]
    # without outputs: the report only; --check says whether the inputs are in step
    r = run("fq-repair", R1, R2)
    assert (r.returncode, r.stderr, r.stdout) == (0, b"", gold["report.tsv"].split(b"\n", 1)[1])
    r = run("fq-repair", "--check", R1, R2)
    assert (r.returncode, r.stderr, r.stdout) == (1, b"", gold["report.tsv"].split(b"\n", 1)[1])
    r = run("fq-repair", "--check", "-t", R1, R1)
    same = repair_of(r1, r1)
    assert same["in_step"] == 1 and (r.returncode, r.stderr, r.stdout.decode()) == (0, b"", STATS_HEADER + "\n" + stats_text(same) + "\n")
    assert sorted(p.name for p in tmp_path.iterdir() if p.name.startswith("c")) == sorted(["c.tsv"] + ["c_" + k for k in GOLD])


# ---- name lengths -------------------------------------------------------------------------------------------------------------
def names_around(rng, n):
    """a name of n bytes and its neighbours: another last byte, another first byte, one byte more"""
    name = LETTERS[rng.integers(0, LETTERS.size, n)].tobytes()
    out = [name, name + b"x"]
    if n:
        out += [name[:-1] + (b"#" if name[-1:] != b"#" else b"%"), (b"#" if name[:1] != b"#" else b"%") + name[1:]]
    return out


@pytest.mark.parametrize("suffix,last", ((False, 50_000), (True, 7), (False, 0)))
def test_name_lengths(gpu, scfq, suffix, last):
    torch = gpu
    rng = np.random.default_rng([20261101, int(suffix), last])
    names = [n for length in LENGTHS for n in names_around(rng, length)]
    # the fourth record of a name differs from the first only behind the delimiter: the same name, in R1 twice
    h1 = [n + (b"/1" if suffix else b"") + b" 1:N:0:%d" % k for k, n in enumerate(names)] + [names[2] + (b"/1" if suffix else b"") + b"\tother"]
    order = rng.permutation(len(names))
    h2 = [names[k] + (b"/2" if suffix else b"") + (b" 2:N:0:%d" % k if k % 3 else b"") for k in order]
    tail = LETTERS[rng.integers(0, LETTERS.size, last)].tobytes()
    d1 = fq(h1 + [tail + b" x"])
    # the last header of R2 is the input's last line, without a newline, its record cut to that one line
    d2 = fq(h2) + b"@" + tail + (b"/2" if suffix else b"")
    want, s = check_device(torch, scfq, d1, d2, ctx=("name lengths", suffix, last), path=1)
    # (the neighbours of a one-byte name coincide, so some names repeat in both inputs alike)
    assert want["pairs"] == len(names) + 1 and want["singles1"] == 1 and want["repeated1"] == want["repeated2"] + 1 and want["lines2"] == 4 * len(names) + 1
    assert want["table"][len(h1)] == len(h2)                                                  # the cut record found its mate
    check_device(torch, scfq, d2, d1, ctx=("name lengths, swapped", suffix, last), path=1, sizing=False)


# ---- orders and overlaps ------------------------------------------------------------------------------------------------------
def order_cases():
    rng = np.random.default_rng(20261102)
    seqs = [b"ACGT"[:1 + k % 4] * (1 + k % 5) for k in range(5000)]
    n100 = numbered(100)
    big = numbered(5000)
    perm = rng.permutation(5000)
    return {
        "reversed": (fq(n100), fq(n100[::-1])),
        "rotated": (fq(n100), fq(n100[1:] + n100[:1])),
        "permutation": (fq(big, seqs=seqs), fq([big[k] for k in perm], seqs=[seqs[k][::-1] for k in perm])),
        "partial": (fq([h for k, h in enumerate(n100) if k % 3 != 0]), fq([h for k, h in enumerate(n100) if k % 3 != 1])),
        "disjoint": (fq(numbered(70, b"a")), fq(numbered(45, b"b"))),
        "first empty": (b"", fq(n100[:33])),
        "second empty": (fq(n100[:65]), b""),
        "both empty": (b"", b""),
        "more in R2": (fq(n100[:40]), fq(n100)),
        "more in R1": (fq(n100), fq(n100[10:97])),
    }


@pytest.mark.parametrize("case", sorted(order_cases()))
def test_orders_and_overlaps(gpu, scfq, case):
    d1, d2 = order_cases()[case]
    want, s = check_device(gpu, scfq, d1, d2, ctx=case)
    expect = {"reversed": dict(pairs=100, moved=100), "rotated": dict(pairs=100, moved=100), "permutation": dict(pairs=5000),
              "partial": dict(pairs=33, singles1=33, singles2=34), "disjoint": dict(pairs=0, singles1=70, singles2=45),
              "first empty": dict(pairs=0, singles2=33, in_step=0), "second empty": dict(pairs=0, singles1=65), "both empty": dict(pairs=0, in_step=1),
              "more in R2": dict(pairs=40, singles2=60, moved=0, in_step=0), "more in R1": dict(pairs=87, singles1=13, moved=87)}[case]
    assert {k: want[k] for k in expect} == expect
    if case == "partial":
        assert want["singles1_bytes"] > 0 and want["singles2_bytes"] > 0


# ---- repeated names -----------------------------------------------------------------------------------------------------------
def test_repeated_names_in_classes(gpu, scfq):
    torch = gpu
    rng = np.random.default_rng(20261103)
    classes = ((1, 1), (2, 1), (3, 5), (63, 64), (64, 64), (65, 1), (5000, 4999))
    h1 = [b"class%d 1:%d" % (c, k) for c, (a, b) in enumerate(classes) for k in range(a)]
    h2 = [b"class%d 2:%d" % (c, k) for c, (a, b) in enumerate(classes) for k in range(b)]
    h1 = [h1[k] for k in rng.permutation(len(h1))]
    h2 = [h2[k] for k in rng.permutation(len(h2))]
    seqs1 = [b"ACGT"[:1 + k % 4] * (1 + k % 7) for k in range(len(h1))]
    seqs2 = [b"TGCA"[:1 + k % 3] * (1 + k % 5) for k in range(len(h2))]
    want, s = check_device(torch, scfq, fq(h1, seqs=seqs1), fq(h2, seqs=seqs2), ctx="classes", path=1)
    assert want["pairs"] == sum(min(a, b) for a, b in classes) and want["singles1"] == 1 + 64 + 1 and want["singles2"] == 2 + 1
    assert want["repeated1"] == sum(a - 1 for a, b in classes) and want["repeated2"] == sum(b - 1 for a, b in classes)


@pytest.mark.parametrize("case", ("one name", "one name, full join", "distinct"))
def test_two_hundred_thousand_records(gpu, scfq, monkeypatch, case):
    """one name carried by 200 000 records of each input costs 200 000 compares a side: linear.  In step it takes path 0, where only R1's
    records form a class; with the positional check off the union's class of 400 000 goes through the rounds, the second sort and the mates"""
    n = 200_000
    if case.startswith("one name"):
        d1, d2 = b"@same 1\nAC\n+\nII\n" * n, b"@same 2\nGT\n+\nII\n" * n
    else:
        rng = np.random.default_rng(20261104)
        d1 = b"".join(b"@n%d\nAC\n+\nII\n" % k for k in range(n))
        d2 = b"".join(b"@n%d\nGT\n+\nII\n" % k for k in rng.permutation(n))
    if case == "one name, full join":
        monkeypatch.setenv("SCFQ_REPAIR_FAST", "0")
    want, s = check_device(gpu, scfq, d1, d2, ctx=case, sizing=False)
    assert want["pairs"] == n and want["repeated1"] == want["repeated2"] == (n - 1 if case.startswith("one name") else 0)
    if case.startswith("one name"):
        assert want["in_step"] == 1 and int(s.path) == (0 if case == "one name" else 1) and want["moved"] == 0
    else:
        assert int(s.path) == 1 and want["moved"] > n // 2


# ---- the hash -----------------------------------------------------------------------------------------------------------------
def test_hash_bits(gpu, scfq):
    torch = gpu
    r1, r2 = (open(p, "rb").read() for p in (R1, R2))
    want, base = check_device(torch, scfq, r1, r2, ctx="default bits", path=1)
    for bits in (1, 2, 4, 33, 64):
        _, s = check_device(torch, scfq, r1, r2, ctx=("hash_bits", bits), want=want, hash_bits=bits, path=1, sizing=False)
        if bits <= 4:
            assert int(s.collisions) > 0 and int(s.rounds) >= 2, (bits, int(s.collisions), int(s.rounds))
    assert int(base.rounds) >= 1                                                               # (every pair is a candidate once)


# ---- placement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", range(16))
def test_inputs_at_every_offset(gpu, scfq, off):
    """both inputs at base + off, the last text at the room's last byte (place); the outputs at other offsets between sentinels"""
    names = numbered(70, b"read_with_a_longer_name_")
    d1 = fq(names, seqs=[b"ACGTTGCA" * (1 + k % 9) for k in range(70)])[:-1]
    d2 = fq(names[35:] + names[:30]) + b"@" + names[33]                                        # ends in a header
    want = repair_of(d1, d2)
    assert want["pairs"] == 66 and want["singles1"] == 4 and want["in_step"] == 0
    check_device(gpu, scfq, d1, d2, ctx=("offsets", off), want=want, offs=(off, (off + 5) % 16), out_offs=(off, 15 - off, (off + 7) % 16, (3 * off) % 16),
                 sizing=False)


# ---- line forms ---------------------------------------------------------------------------------------------------------------
def line_form_cases():
    """the plain files of tests/golden/edge/; its two .gz files go through the file entry point below"""
    names = numbered(40, b"q", b" c")
    cases = {"crlf": fq(names, eol=b"\r\n"), "no final newline": fq(names)[:-1], "blank lines": fq(names[:9]) + b"\n\n\n" + fq(names[9:20]) + b"\n",
             "crlf, no final": fq(names, eol=b"\r\n")[:-2]}
    for f in sorted(os.listdir(EDGE)):
        if f.endswith(".fq"):
            cases["edge/" + f] = open(os.path.join(EDGE, f), "rb").read()
    return cases


@pytest.mark.parametrize("case", sorted(line_form_cases()))
def test_line_forms_are_in_step_with_themselves(gpu, scfq, case):
    from _readstats_check import lines_of
    d = line_form_cases()[case]
    want, s = check_device(gpu, scfq, d, d, ctx=case, path=0)
    reads = want["reads1"]
    assert want["in_step"] == 1 and want["table"] == list(range(reads)) * 2
    # out1 is fq-screen's echo of the input: each line it has, as text plus '\n'
    assert want["out1"] == want["out2"] == b"".join(t + b"\n" for t in lines_of(d)) and want["singles1_bytes"] == 0


def test_compressed_edge_files_against_themselves(gpu, scfq, tmp_path):
    """two_member.fq.gz inflates to both members' records and is in step with itself; not_gzip.fq.gz, plain text under a .gz name, is read
    as the text it is, as everywhere else"""
    import gzip
    gz = sorted(f for f in os.listdir(EDGE) if f.endswith(".gz"))
    assert gz == ["not_gzip.fq.gz", "two_member.fq.gz"]
    for f in gz:
        p = os.path.join(EDGE, f)
        raw = open(p, "rb").read()
        d = gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw
        want = repair_of(d, d)
        s, outs, table = file_call(scfq, tmp_path, p, p)
        assert_stats(s, want, f, path=0)
        assert outs == want["outs"] and table.decode() == per_read_text(want) and want["in_step"] == 1 and want["reads1"] > 0, f


# ---- laws ---------------------------------------------------------------------------------------------------------------------
def test_the_fast_path_changes_nothing_but_path(gpu, scfq, monkeypatch):
    torch = gpu
    names = numbered(300, b"frag") + [b"again", b"again", b"", b""]
    d1, d2 = fq([n + b"/1" for n in names]), fq([n + b"/2 c" for n in names], seqs=[b"GGCC"] * len(names))
    want, fast = check_device(torch, scfq, d1, d2, ctx="fast", path=0)
    assert want["in_step"] == 1 and want["repeated1"] == want["repeated2"] == 2
    monkeypatch.setenv("SCFQ_REPAIR_FAST", "0")
    _, slow = check_device(torch, scfq, d1, d2, ctx="fast path off", want=want, path=1)
    monkeypatch.setenv("SCFQ_REPAIR_FAST", "1")
    check_device(torch, scfq, d1, d2, ctx="fast path on", want=want, path=0, sizing=False)
    monkeypatch.delenv("SCFQ_REPAIR_FAST")
    assert [int(getattr(fast, k)) for k in FIELDS] == [int(getattr(slow, k)) for k in FIELDS]
    # one name differs in the last record: the positional check says so and the join runs
    d3 = fq([n + b"/2 c" for n in names[:-1]] + [b"other"])
    w3, s3 = check_device(torch, scfq, d1, d3, ctx="one name differs", path=1)
    assert w3["pairs"] == len(names) - 1 and w3["moved"] == 0 and w3["in_step"] == 0


def test_repairing_a_repair_is_in_step(gpu, scfq):
    torch = gpu
    r1, r2 = (open(p, "rb").read() for p in (R1, R2))
    first = repair_of(r1, r2)
    want, s = check_device(torch, scfq, first["out1"], first["out2"], ctx="again", path=0)
    assert want["in_step"] == 1 and want["outs"] == [first["out1"], first["out2"], b"", b""]


def test_swapping_the_inputs_swaps_the_result(gpu, scfq):
    torch = gpu
    r1, r2 = (open(p, "rb").read() for p in (R1, R2))
    ab, s_ab = check_device(torch, scfq, r1, r2, ctx="a b", sizing=False)
    ba, s_ba = check_device(torch, scfq, r2, r1, ctx="b a", sizing=False)
    n1 = ab["reads1"]
    assert ba["table"] == ab["table"][n1:] + ab["table"][:n1]
    for x, y in (("pairs", "pairs"), ("singles1", "singles2"), ("repeated1", "repeated2"), ("singles1_bytes", "singles2_bytes"), ("moved", "moved")):
        assert int(getattr(s_ab, x)) == int(getattr(s_ba, y)) and int(getattr(s_ab, y)) == int(getattr(s_ba, x)), (x, y)
    assert sorted(ab["out1"].split(b"@")) == sorted(ba["out2"].split(b"@"))                   # the same records, in the other input's order


# ---- capacities ---------------------------------------------------------------------------------------------------------------
def test_capacities_and_arguments(gpu, scfq):
    torch = gpu
    r1, r2 = (open(p, "rb").read() for p in (R1, R2))
    want = repair_of(r1, r2)
    a1, a2 = as_array(r1), as_array(r2)
    t1, p1, _ = place(torch, a1)
    t2, p2, _ = place(torch, a2)
    units = want["reads1"] + want["reads2"]
    sizes = [len(w) for w in want["outs"]]
    assert all(sizes)
    # each output too small by one byte in turn: SCFQ_EARG naming it, the stats complete, nothing written anywhere
    for k, name in enumerate(OUTPUTS):
        outs = [Out(torch, n - (1 if j == k else 0), 1 + j) for j, n in enumerate(sizes)]
        table = Out(torch, 4 * units, 4)
        with pytest.raises(scfq.ScfqError) as e:
            scfq.repair_resident(p1, a1.size, p2, a2.size, None, [o.arg() for o in outs], table=(table.ptr, units))
        assert e.value.rc == scfq.SCFQ_EARG and "the %s output holds %d bytes, the result has %d" % (name, sizes[k] - 1, sizes[k]) in str(e.value), str(e.value)
        assert_stats(e.value.stats, want, ("too small", name))
        assert all(o.bytes(0) == b"" for o in outs)
    # a table that is too small: nothing is written to it or to an output
    outs = [Out(torch, n, 2) for n in sizes]
    table = Out(torch, 4 * units, 4)
    with pytest.raises(scfq.ScfqError) as e:
        scfq.repair_resident(p1, a1.size, p2, a2.size, None, [o.arg() for o in outs], table=(table.ptr, units - 1))
    assert e.value.rc == scfq.SCFQ_EARG and "per-record table holds %d entries" % (units - 1) in str(e.value)
    assert_stats(e.value.stats, want, "small table")
    assert table.bytes(0) == b"" and all(o.bytes(0) == b"" for o in outs)
    # subsets of the outputs; the others' sizes are reported all the same
    for which in ((True, False, False, False), (False, True, False, False), (False, False, True, True), (True, True, False, False), (False, True, False, True)):
        outs = [Out(torch, n, 3) if w else None for n, w in zip(sizes, which)]
        s = scfq.repair_resident(p1, a1.size, p2, a2.size, None, [o.arg() if o else None for o in outs])
        assert_stats(s, want, ("subset", which))
        for name, o, w in zip(OUTPUTS, outs, want["outs"]):
            if o:
                differ(which, name, o.bytes(len(w)), w)
    s, table, outs = scfq.repair_host(r1, r2, want=(False, True, True, False), table_cap=0)
    assert table is None and outs == [None, want["out2"], want["singles1_out"], None]
    with pytest.raises(scfq.ScfqError) as e:
        scfq.repair_host(r1, r2, caps=[sizes[0], sizes[1], sizes[2] - 1, sizes[3]])
    assert e.value.rc == scfq.SCFQ_EARG and "singles1" in str(e.value)
    # argument errors
    for kw, text in ((dict(flags=1), "unknown flag bits 0x1"), (dict(hash_bits=65), "hash_bits 65"), (dict(reserved=(0, 0, 0, 9)), "reserved")):
        with pytest.raises(scfq.ScfqError) as e:
            scfq.repair_resident(p1, a1.size, p2, a2.size, scfq.repair_opts(**kw))
        assert e.value.rc == scfq.SCFQ_EARG and text in str(e.value), (kw, str(e.value))

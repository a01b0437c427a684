"""fq-demux on the device (csrc/scfq_demux.hip) against the checker of tests/_demux_check.py: the outputs compared with ==, byte for
byte, every field of the statistics, every row, the per-unit table, and the bytes around every output buffer."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG
from _demux_check import ASSIGNED, assert_stats, demux_of, recs_of, report_text
from test_demux_host import HAND
from test_gpu_parity import to_dev
from test_gpu_trim import Out, as_array, differ

pytestmark = pytest.mark.gpu

SC = os.path.join(PKG, "sc")
DEMUX = os.path.join(GOLDEN, "demux")
R1, R2, IL, R2GZ, SHEET = (os.path.join(DEMUX, f) for f in ("r1.fq", "r2.fq", "interleaved.fq", "r2.fq.gz", "sheet.tsv"))
LETTERS = np.frombuffer(b"ACGT", np.uint8)


def dna(rng, n):
    return bytes(rng.choice(LETTERS, n))


def sheet_file():
    rows = [line.split("\t") for line in open(SHEET).read().splitlines() if line and not line.startswith("#")]
    return [tuple(r) for r in rows]


def substituted(rng, bc, k):
    bc = bytearray(bc)
    for i in rng.choice(len(bc), min(k, len(bc)), replace=False):
        bc[i] = rng.choice([b for b in b"ACGTN" if b != bc[i]])
    return bytes(bc)


def record(header, seq, rng=None):
    qual = bytes(rng.integers(35, 74, len(seq), dtype=np.uint8)) if rng is not None else b"I" * len(seq)
    return b"@" + header + b"\n" + seq + b"\n+\n" + qual + b"\n"


def pooled(rng, samples, n, read=40, pick=None, p_sub=0.2, p_rand=0.1):
    """n units whose inline barcodes are drawn from `samples` (pick(u): the sample of unit u, default random): r1 and r2 (r2 for a sheet
    without second barcodes is plain reads)"""
    r1, r2 = [], []
    for u in range(n):
        s = samples[pick(u) if pick else int(rng.integers(len(samples)))]
        b1, b2 = s[1].encode(), (s[2].encode() if len(s) > 2 else b"")
        x = rng.random()
        if x < p_sub:
            b1, b2 = substituted(rng, b1, int(rng.integers(0, 3))), (substituted(rng, b2, int(rng.integers(0, 3))) if b2 else b2)
        elif x < p_sub + p_rand:
            b1, b2 = dna(rng, len(b1)), dna(rng, len(b2))
        r1.append(record(b"u%d/1" % u, b1 + dna(rng, read), rng))
        r2.append(record(b"u%d/2" % u, b2 + dna(rng, read), rng))
    return b"".join(r1), b"".join(r2)


def interleave(r1, r2):
    """whole four-line records of r1 and r2, alternating"""
    a, b, out = r1.split(b"\n")[:-1], r2.split(b"\n")[:-1], []
    for u in range(len(a) // 4):
        out += a[4 * u:4 * u + 4] + b[4 * u:4 * u + 4]
    return b"".join(x + b"\n" for x in out)


def distinct_barcodes(rng, n, length):
    seen = []
    while len(seen) < n:
        b = dna(rng, length).decode()
        if b not in seen:
            seen.append(b)
    return seen


def check_device(torch, scfq, samples, d1, d2=None, kw=None, ctx="", offs=(0, 0), out_offs=(1, 3), want=None, extra=7, sheet=None):
    """the device entry point on d1 / d2: the sizing call, then outputs of the reported sizes + extra bytes between sentinels, and the
    per-unit table in device memory"""
    kw = kw or {}
    a1, a2 = as_array(d1), as_array(d2)
    if want is None:
        want = demux_of(bytes(d1), None if d2 is None else bytes(d2), samples, **kw)
    own = sheet is None
    sheet = sheet or scfq.demux_sheet(samples)
    opts = scfq.demux_opts(**kw)
    t1, p1 = to_dev(torch, a1, offs[0])
    t2, p2 = to_dev(torch, a2, offs[1]) if a2 is not None else (None, None)
    n2 = a2.size if a2 is not None else 0
    s, rows = scfq.demux_device(sheet, p1, a1.size, p2, n2, opts)
    assert_stats(s, rows, want, (ctx, "sizing"))
    units = want["units_in"]
    table = torch.full((8 * units + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    outs = [Out(torch, len(want["out1"]) + extra, out_offs[0]), Out(torch, len(want["out2"]) + extra, out_offs[1]) if a2 is not None else None]
    s, rows = scfq.demux_device(sheet, p1, a1.size, p2, n2, opts, *[o.arg() if o else None for o in outs], recs=(table.data_ptr(), units))
    assert_stats(s, rows, want, (ctx, kw, offs, out_offs))
    for k, o in zip(("out1", "out2"), outs):
        if o:
            differ(ctx, k, o.bytes(len(want[k])), want[k])
    h = table.cpu().numpy()
    assert (h[8 * units:] == 0xEE).all(), (ctx, "the table was written past its entries")
    assert recs_of(h[:8 * units].reshape(-1, 8)) == want["recs"], ctx
    if own:
        sheet.close()
    return want


def check_host(scfq, samples, d1, d2, kw, want, ctx):
    with scfq.demux_sheet(samples) as sheet:
        s, rows, o1, o2 = scfq.demux_host(sheet, d1, d2, scfq.demux_opts(**kw))
    assert_stats(s, rows, want, (ctx, "host"))
    assert o1 == want["out1"] and (o2 == want["out2"] if d2 is not None else o2 is None), (ctx, "host")


def check_files(scfq, tmp_path, samples, p1, p2, kw, want, ctx, two):
    """scfq_demux_files into a fresh directory: a file per destination and mate, the rows, the per-unit table in host memory"""
    out = tmp_path / ("out_%d" % len(list(tmp_path.iterdir())))
    out.mkdir()
    recs = (scfq.DemuxRec * max(want["units_in"], 1))()
    with scfq.demux_sheet(samples) as sheet:
        s, rows = scfq.demux_file(sheet, p1, p2, scfq.demux_opts(**kw), out_dir=str(out), recs=recs)
        names = sheet.names
    assert_stats(s, rows, want, (ctx, "file"))
    assert recs_of(recs[:want["units_in"]]) == want["recs"], ctx
    expect = {}
    for d, name in enumerate(names):
        r = want["rows"][d]
        if two:
            expect[name + "_R1.fq"] = want["out1"][r["off1"]:r["off1"] + r["bytes1"]]
            expect[name + "_R2.fq"] = want["out2"][r["off2"]:r["off2"] + r["bytes2"]]
        else:
            expect[name + ".fq"] = want["out1"][r["off1"]:r["off1"] + r["bytes1"]]
    assert sorted(os.listdir(out)) == sorted(expect), ctx
    for name, data in expect.items():
        assert (out / name).read_bytes() == data, (ctx, name)
    return out


def test_fixtures_every_entry_point(gpu, scfq, tmp_path):
    torch = gpu
    samples = sheet_file()
    r1, r2, il = (open(p, "rb").read() for p in (R1, R2, IL))
    two, one = demux_of(r1, r2, samples), demux_of(il, None, samples, interleaved=True)
    names = [s[0] for s in samples] + ["undetermined"]
    for d, name in enumerate(names):
        r = two["rows"][d]
        assert open(os.path.join(DEMUX, name + "_R1.fq"), "rb").read() == two["out1"][r["off1"]:r["off1"] + r["bytes1"]]
        assert open(os.path.join(DEMUX, name + "_R2.fq"), "rb").read() == two["out2"][r["off2"]:r["off2"] + r["bytes2"]]
    check_device(torch, scfq, samples, r1, r2, want=two, ctx="two")
    check_device(torch, scfq, samples, il, None, dict(interleaved=True), want=one, ctx="interleaved")
    check_host(scfq, samples, r1, r2, {}, two, "two")
    check_host(scfq, samples, il, None, dict(interleaved=True), one, "interleaved")
    check_files(scfq, tmp_path, samples, R1, R2, {}, two, "two", True)
    check_files(scfq, tmp_path, samples, R1, R2GZ, {}, two, "two, gz", True)
    check_files(scfq, tmp_path, samples, IL, None, dict(interleaved=True), one, "interleaved", False)
    # interleaved equals paired, once interleaved: per destination, mate 1 and mate 2 of each unit alternate
    for d in range(len(names)):
        a, b, c = two["rows"][d], one["rows"][d], []
        m1 = two["out1"][a["off1"]:a["off1"] + a["bytes1"]].split(b"\n")
        m2 = two["out2"][a["off2"]:a["off2"] + a["bytes2"]].split(b"\n")
        for u in range(a["units"]):
            c += m1[4 * u:4 * u + 4] + m2[4 * u:4 * u + 4]
        assert b"".join(x + b"\n" for x in c) == one["out1"][b["off1"]:b["off1"] + b["bytes1"]] and b["bytes1"] == a["bytes1"] + a["bytes2"], d
    # report only: no directory
    with scfq.demux_sheet(samples) as sheet:
        s, rows = scfq.demux_file(sheet, R1, R2GZ)
        assert_stats(s, rows, two, "file, no output")
        assert [scfq.format_demux_row_tsv(s, sheet, d, rows[d]) for d in range(len(names))] == report_text(two, samples)
    assert len(scfq.demux_stages()) == 4
    # the barcodes kept; no mismatch allowed; three
    for kw in (dict(keep_barcode=True), dict(mismatches=0), dict(mismatches=3)):
        check_device(torch, scfq, samples, r1, r2, kw, ctx=str(kw))


def test_cli_on_the_fixtures(gpu, tmp_path):
    out = tmp_path / "out"
    out.mkdir()
    per_read = tmp_path / "per_read.tsv"
    r = subprocess.run([SC, "fq-demux", "-t", "--sheet=" + SHEET, "--out-dir=%s" % out, "--per-read=%s" % per_read, R1, R2GZ], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    assert r.stdout == open(os.path.join(DEMUX, "report.tsv")).read()
    names = [s[0] for s in sheet_file()] + ["undetermined"]
    assert sorted(os.listdir(out)) == sorted(n + m for n in names for m in ("_R1.fq", "_R2.fq"))
    for f in os.listdir(out):
        assert (out / f).read_bytes() == open(os.path.join(DEMUX, f), "rb").read(), f
    two = demux_of(open(R1, "rb").read(), open(R2, "rb").read(), sheet_file())
    rows = [line.split("\t") for line in per_read.read_text().splitlines()]
    state = ("assigned", "unmatched", "ambiguous", "no_barcode")
    assert rows == [[str(u), names[s], str(a), str(b), state[0]] if k == ASSIGNED else [str(u), "-", "-", "-", state[k]] for u, (s, a, b, k) in enumerate(two["recs"])]
    # the samples on the command line, one input, header mode: a report without a directory; -b adds the file's name
    r = subprocess.run([SC, "fq-demux", "--sample=x:ACGT", "--sample=y:ACGA+TT", "--barcodes=header", "--mismatches=0", "-b", R1], capture_output=True, text=True)
    assert r.returncode == 1 and "sample 1 has a second barcode, sample 0 has none" in r.stderr
    r = subprocess.run([SC, "fq-demux", "--sample=x:ACGT", "--sample=y:ACGA", "--barcodes=header", "--mismatches=0", "-b", R1], capture_output=True, text=True)
    want = demux_of(open(R1, "rb").read(), None, [("x", "ACGT"), ("y", "ACGA")], header=True, mismatches=0)
    assert r.returncode == 0 and r.stdout.splitlines() == [line + "\tr1.fq" for line in report_text(want, [("x", "ACGT"), ("y", "ACGA")])]


@pytest.mark.parametrize("c", HAND, ids=[c["name"] for c in HAND])
def test_hand_worked_cases(gpu, scfq, c):
    """the cases of test_demux_host.py, whose expected bytes stand there literally, through the device and the host entry point"""
    want = demux_of(c["d1"], c["d2"], c["samples"], **c["kw"])
    assert want["recs"] == c["recs"] and want["out1"] == c["out1"] and want["out2"] == c["out2"]
    check_device(gpu, scfq, c["samples"], c["d1"], c["d2"], c["kw"], want=want, ctx=c["name"])
    with scfq.demux_sheet(c["samples"]) as sheet:
        s, rows, o1, o2 = scfq.demux_host(sheet, c["d1"], c["d2"], scfq.demux_opts(**c["kw"]))
    assert o1 == c["out1"] and (o2 or b"") == c["out2"] and [int(r.units) for r in rows] == c["units"]
    for k, v in c["stats"].items():
        assert int(getattr(s, k)) == v, (k, int(getattr(s, k)), v)


def test_unit_counts(gpu, scfq):
    """around the group of 32, the wave of 64 and the block of 256 (no kernel strides: a thread, or a wave, per unit or group)"""
    rng = np.random.default_rng(101)
    samples = [("a", "ACGTAC", "TTGACA"), ("b", "GGATCC", "CATGGT"), ("c", "TCAGGA", "AGCTTG")]
    with scfq.demux_sheet(samples) as sheet:
        for n in (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257):
            r1, r2 = pooled(rng, samples, n, read=int(rng.integers(1, 60)))
            check_device(gpu, scfq, samples, r1, r2, ctx=("two", n), sheet=sheet, offs=(n % 16, (3 * n) % 16))
            check_device(gpu, scfq, samples, interleave(r1, r2), None, dict(interleaved=True), ctx=("interleaved", n), sheet=sheet)


@pytest.mark.parametrize("n_samples", (1, 2, 3, 63, 64, 65, 255, 256, 257, 1024))
def test_sample_counts(gpu, scfq, n_samples):
    """the sort's bit count steps through 1, 2, 6, 7, 8, 9 and 11; the last samples of the sheet receive units"""
    rng = np.random.default_rng(200 + n_samples)
    codes = distinct_barcodes(rng, n_samples, 7)
    samples = [("s%d" % i, c) for i, c in enumerate(codes)]
    units = 150
    r1, r2 = pooled(rng, samples, units, read=20, pick=lambda u: (n_samples - 1 - u // 2) % n_samples if u % 3 else int(rng.integers(n_samples)))
    want = check_device(gpu, scfq, samples, r1, None, dict(mismatches=1), ctx=("single", n_samples))
    assert want["rows"][n_samples - 1]["units"] > 0 and want["assigned"] > units // 2
    check_device(gpu, scfq, samples, r1, r2, dict(mismatches=2), ctx=("two", n_samples))


def test_barcode_lengths_and_prefixes(gpu, scfq):
    """1, 2, 15, 16, 17, 31 and 32 letters, every barcode a prefix of the next: the longest eligible one without a mismatch wins"""
    rng = np.random.default_rng(303)
    lengths = (1, 2, 15, 16, 17, 31, 32)
    p, q = dna(rng, 32).decode(), dna(rng, 32).decode()
    single = [("len%d" % n, p[:n]) for n in lengths]
    dual = [("len%d" % n, p[:n], q[:33 - n if n > 1 else 32]) for n in lengths]
    r1, r2 = [], []
    for u in range(120):
        n = lengths[u % 7] + int(rng.integers(-1, 2))
        cut = int(rng.integers(0, 33))
        a = p[:n].encode() + dna(rng, int(rng.integers(0, 3)))
        b = q[:cut].encode() + dna(rng, 40 - cut)
        if u % 5 == 0:
            a = substituted(rng, a, 1) if a else a
        r1.append(record(b"u%d" % u, a, rng))
        r2.append(record(b"u%d" % u, b, rng))
    r1, r2 = b"".join(r1), b"".join(r2)
    for m in (0, 1, 3):
        want = check_device(gpu, scfq, single, r1, None, dict(mismatches=m), ctx=("single", m))
        assert m > 0 or all(r["units"] for r in want["rows"])
        check_device(gpu, scfq, dual, r1, r2, dict(mismatches=m), ctx=("dual", m))
        check_device(gpu, scfq, dual, r1, r2, dict(mismatches=m, keep_barcode=True), ctx=("dual, kept", m))


def test_destination_patterns(gpu, scfq):
    rng = np.random.default_rng(404)
    codes = distinct_barcodes(rng, 300, 8)
    samples = [("s%d" % i, c) for i, c in enumerate(codes)]
    n = 200
    patterns = dict(one=lambda u: 7, different=lambda u: u, gaps=lambda u: (0, 5, 6, 299, 150)[u % 5], alternating=lambda u: 3 + 200 * (u % 2))
    for name, pick in patterns.items():
        r1, r2 = pooled(rng, samples, n, read=30, pick=pick, p_sub=0, p_rand=0)
        want = check_device(gpu, scfq, samples, r1, r2, dict(mismatches=0), ctx=name)
        filled = sorted(d for d, r in enumerate(want["rows"]) if r["units"])
        assert filled == sorted(set(pick(u) for u in range(n))), name
    # nothing matches: every unit is undetermined, in input order
    r1, r2 = pooled(rng, samples, n, read=30, p_sub=0, p_rand=1.0)
    want = check_device(gpu, scfq, samples[:40], r1, r2, dict(mismatches=0), ctx="undetermined")
    assert want["rows"][-1]["units"] > n - 5 and want["out1"].count(b"@u") == n


def test_read_and_header_lengths_and_offsets(gpu, scfq):
    """reads of 0, m - 1, m, m + 1 and 1000 bases, headers of 1 to 300 bytes, the inputs at every offset of a 16-byte step"""
    rng = np.random.default_rng(505)
    samples = [("a", "ACGTACGT", "TTGACCAG"), ("b", "GGATCCTA", "CATGGTCA")]
    m = 8
    r1, r2, hd = [], [], []
    for u, (length, header) in enumerate((L, H) for L in (0, m - 1, m, m + 1, 1000, 37) for H in (1, 15, 16, 17, 300)):
        s = samples[u % 2]
        name = (b"%d" % u).ljust(header - 1, b"x")[:header - 1]
        r1.append(record(name, (s[1].encode() + dna(rng, 1000))[:length], rng))
        r2.append(record(name, (s[2].encode() + dna(rng, 1000))[:max(length, m)], rng))
        hd.append(record(name[:max(header - 20, 0)] + b" 1:N:0:" + s[1].encode() + b"+" + s[2].encode(), dna(rng, length), rng))
    r1, r2, hd = b"".join(r1), b"".join(r2), b"".join(hd)
    with scfq.demux_sheet(samples) as sheet:
        want = demux_of(r1, r2, samples)
        assert want["no_barcode"] == 10 and want["assigned"] == 20
        hwant = demux_of(hd, None, samples, header=True)
        assert hwant["assigned"] == 30
        for off in range(16):
            check_device(gpu, scfq, samples, r1, r2, want=want, ctx=("inline", off), sheet=sheet, offs=(off, 15 - off), out_offs=(off, 17 - off))
            check_device(gpu, scfq, samples, hd, None, dict(header=True), want=hwant, ctx=("header", off), sheet=sheet, offs=(off, 0), out_offs=(off + 1, 0))
        # "\r\n" line ends and a last line without a newline: every record goes out as its four pieces
        crlf = r1.replace(b"\n", b"\r\n")
        check_device(gpu, scfq, samples, crlf, r2[:-1], ctx="crlf", sheet=sheet)
        check_device(gpu, scfq, samples, hd.replace(b"\n", b"\r\n")[:-2], None, dict(header=True), ctx="crlf, header", sheet=sheet)


def test_capacities(gpu, scfq):
    torch = gpu
    samples = sheet_file()
    r1, r2 = (open(p, "rb").read() for p in (R1, R2))
    two = demux_of(r1, r2, samples)
    t1, p1 = to_dev(torch, as_array(r1))
    t2, p2 = to_dev(torch, as_array(r2), 3)
    with scfq.demux_sheet(samples) as sheet:
        # exact capacities
        check_device(torch, scfq, samples, r1, r2, want=two, ctx="exact", extra=0, sheet=sheet)
        # an output that is one byte too small: SCFQ_EARG that names it, statistics and rows complete, no byte written anywhere
        for name in ("out1", "out2"):
            outs = [Out(torch, len(two[o]) - (1 if o == name else 0), 1 + 2 * j) for j, o in enumerate(("out1", "out2"))]
            with pytest.raises(scfq.ScfqError) as e:
                scfq.demux_device(sheet, p1, len(r1), p2, len(r2), None, *[o.arg() for o in outs])
            assert e.value.rc == scfq.SCFQ_EARG and name in str(e.value), (name, str(e.value))
            assert str(len(two[name])) in str(e.value) and str(len(two[name]) - 1) in str(e.value), str(e.value)
            assert_stats(e.value.stats, e.value.rows, two, ("too small", name))
            for o in outs:
                assert o.bytes(0) == b""
            with pytest.raises(scfq.ScfqError) as e:
                scfq.demux_host(sheet, r1, r2, None, caps=[len(two[o]) - (1 if o == name else 0) for o in ("out1", "out2")])
            assert e.value.rc == scfq.SCFQ_EARG and name in str(e.value)
            assert_stats(e.value.stats, e.value.rows, two, ("too small, host", name))
        # the per-unit table one entry short: nothing is written to it; the rows one entry short: before any launch
        table = torch.full((8 * two["units_in"],), 0xEE, dtype=torch.uint8, device="cuda")
        with pytest.raises(scfq.ScfqError) as e:
            scfq.demux_device(sheet, p1, len(r1), p2, len(r2), None, recs=(table.data_ptr(), two["units_in"] - 1))
        assert e.value.rc == scfq.SCFQ_EARG and "the per-unit table holds 119 entries, the input has 120 units" in str(e.value)
        assert (table.cpu().numpy() == 0xEE).all()
        with pytest.raises(scfq.ScfqError) as e:
            scfq.demux_device(sheet, p1, len(r1), p2, len(r2), None, row_cap=len(samples))
        assert e.value.rc == scfq.SCFQ_EARG and "the rows hold 4 entries, the sheet needs 5" in str(e.value)
        recs = (scfq.DemuxRec * 119)()
        with pytest.raises(scfq.ScfqError) as e:
            scfq.demux_file(sheet, R1, R2, recs=recs)
        assert e.value.rc == scfq.SCFQ_EARG and "119 entries" in str(e.value)
        # only one output asked for
        s, rows, o1, o2 = scfq.demux_host(sheet, r1, r2, None, caps=(None, len(two["out2"]) + 9))
        assert_stats(s, rows, two, "host, one output")
        assert (o1, o2) == (None, two["out2"])


def slices(w):
    return [(w["out1"][r["off1"]:r["off1"] + r["bytes1"]], w["out2"][r["off2"]:r["off2"] + r["bytes2"]]) for r in w["rows"]]


def host_result(scfq, sheet, d1, d2, **kw):
    s, rows, o1, o2 = scfq.demux_host(sheet, d1, d2, scfq.demux_opts(**kw))
    return dict(out1=o1, out2=o2 or b"", rows=[dict(off1=int(r.off1), bytes1=int(r.bytes1), off2=int(r.off2), bytes2=int(r.bytes2), units=int(r.units)) for r in rows])


def test_law_concatenation(gpu, scfq):
    """for whole-record inputs A and B: per destination, the slice of demux(A + B) is the slice of demux(A) followed by that of demux(B)"""
    rng = np.random.default_rng(606)
    codes = distinct_barcodes(rng, 20, 6)
    samples = [("s%d" % i, c, codes[(i + 7) % 20]) for i, c in enumerate(codes)]
    a1, a2 = pooled(rng, samples, 333, read=25)
    b1, b2 = pooled(rng, samples, 77, read=50)
    with scfq.demux_sheet(samples) as sheet:
        for kw in (dict(), dict(keep_barcode=True, mismatches=2)):
            a, b, ab = host_result(scfq, sheet, a1, a2, **kw), host_result(scfq, sheet, b1, b2, **kw), host_result(scfq, sheet, a1 + b1, a2 + b2, **kw)
            assert slices(ab) == [(x[0] + y[0], x[1] + y[1]) for x, y in zip(slices(a), slices(b))]
            assert [r["units"] for r in ab["rows"]] == [x["units"] + y["units"] for x, y in zip(a["rows"], b["rows"])]


def test_law_header_mode_permutes_the_records(gpu, scfq):
    """in header mode nothing is clipped: the destinations' slices are a permutation of the normalised input records"""
    rng = np.random.default_rng(707)
    codes = distinct_barcodes(rng, 12, 8)
    samples = [("s%d" % i, c) for i, c in enumerate(codes)]
    tails = [c.encode() for c in codes] + [b"", b"ACGT", b"+", codes[0].encode() + b"+" + codes[1].encode(), substituted(rng, codes[2].encode(), 1)]
    recs = [record(b"r%d 1:N:0:" % u + tails[int(rng.integers(len(tails)))], dna(rng, int(rng.integers(0, 90))), rng) for u in range(400)]
    data = b"".join(recs).replace(b"\n", b"\r\n", 40)[:-1]                       # some "\r\n", no final newline: normalised on the way
    with scfq.demux_sheet(samples) as sheet:
        w = host_result(scfq, sheet, data, None, header=True)
    assert sorted(w["out1"].split(b"@r")) == sorted(b"".join(recs).split(b"@r")) and len(w["out1"]) == len(b"".join(recs))
    assert sum(r["units"] for r in w["rows"]) == 400 and 0 < w["rows"][-1]["units"] < 400

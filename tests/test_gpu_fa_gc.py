"""fa-gc on the device against the checker of _fa_gc_check.py: every comparison is == on integers or text.  T = 4096 is the
tile of the kernels; tiles lie on the ADDRESS grid, so an input at pointer offset `off` has its tile edges at k T - off."""
import ctypes
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG
from _fa_gc_check import PINS, FaModel, cli_text, gc_interval, parse_positions, parse_window, warning_line
from test_gpu_parity import to_dev
from test_ingest_sources import bgzf_file

pytestmark = pytest.mark.gpu

T = 4096
SC = os.path.join(PKG, "sc")
FASTA = os.path.join(GOLDEN, "fasta", "test.fasta")
OFFSETS = (0, 1, 15, 16)
SIZES = (0, 1, T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T + 17)
ALPHABET = np.frombuffer(b"ACGTACGTACGTacgtacgtNNnRYKMSWBDHVryk", dtype=np.uint8)


def run(*args):
    return subprocess.run([SC] + [str(a) for a in args], capture_output=True, text=True, stdin=subprocess.DEVNULL)


def red(code, msg):
    return "\x1b[31mError %d: %s\x1b[0m\n" % (code, msg)


def seq_bytes(rng, n):
    """bases with lower case, N runs and IUPAC letters mixed in"""
    s = rng.choice(ALPHABET, n)
    for _ in range(n // 300 + (n > 20)):
        at = int(rng.integers(0, max(1, n - 10)))
        s[at:at + int(rng.integers(1, 40))] = ord("N")
    return s.tobytes()


def wrapped(rng, names_lengths, width, eol=b"\n", final_eol=True):
    out = []
    for name, length in names_lengths:
        out.append(b">" + name + eol)
        s = seq_bytes(rng, length)
        out += [s[i:i + width] + eol for i in range(0, length, width)]
    data = b"".join(out)
    return data if final_eol or not data.endswith(eol) else data[:-len(eol)]


def mixed_input(rng, n, off):
    """n bytes with every small feature, and the two tile-edge cases patched in at the edges k T - off"""
    parts = [b"acgtnACGT\nGG\n"]                                        # sequence lines before any header
    k = 0
    while sum(map(len, parts)) < n + 200:
        eol = b"\r\n" if k % 3 == 1 else b"\n"
        name = b"c%d" % k + (b" some text>x" if k % 2 else b"")          # a '>' in the middle of a header
        parts.append(b">" + name + eol)
        if k % 5 == 2:
            parts.append(b">twin%d" % k + eol)                          # two header lines in a row: the first has no bases
        for j in range(int(rng.integers(0, 9))):
            line = seq_bytes(rng, int(rng.integers(1, 130)))
            if j % 4 == 1:
                line = line[:len(line) // 2] + b">" + line[len(line) // 2:]      # a '>' in the middle of a sequence line
            parts.append(line + eol)
            if j % 5 == 3:
                parts.append(eol)                                       # a blank line
        k += 1
    a = np.frombuffer(b"".join(parts)[:n], dtype=np.uint8).copy()
    for j, edge in enumerate(range(T - off, n, T)):
        if edge >= 1 and edge < n:
            a[edge - 1] = 10
            a[edge] = ord(">") if j % 2 == 0 else ord("G")
            if j % 2 == 0 and edge + 8 < n:
                a[edge + 1:edge + 8] = np.frombuffer(b"edge%02d\n" % j, dtype=np.uint8)[:7]
    if n and a[-1] == 10 and n % 2:
        a[-1] = ord("C")                                                # the input ends without '\n'
    return a


def features(a, off):
    """which of the tile-edge cases an input at pointer offset off holds"""
    n = a.size
    got = set()
    is_nl = a == 10
    starts = np.concatenate(([0], np.flatnonzero(is_nl) + 1))
    starts = starts[starts < n]
    hdr = a[starts] == ord(">") if starts.size else np.zeros(0, dtype=bool)
    for edge in range(T - off, n, T):
        if edge >= 1 and is_nl[edge - 1]:
            got.add("nl_then_gt" if a[edge] == ord(">") else "nl_then_base" if a[edge] != 10 else "nl_then_nl")
    for lo in range(-off, n, T):                                        # whole tiles without '\n'
        if lo > 0 and lo + T <= n and not is_nl[lo:lo + T].any():
            line = int(np.searchsorted(starts, lo, side="right")) - 1
            got.add("tile_in_header" if hdr[line] else "tile_in_sequence")
    if n and a[-1] != 10:
        got.add("no_final_nl")
    if n and a[0] != ord(">"):
        got.add("orphans")
    if starts.size > 1 and (hdr[:-1] & hdr[1:]).any():
        got.add("twin_headers")
    if n > 1 and (is_nl[:-1] & is_nl[1:]).any():
        got.add("blank_line")
    if n > 1 and ((a[:-1] == 13) & is_nl[1:]).any():
        got.add("crlf")
    gt = np.flatnonzero(a == ord(">"))
    mid = gt[~np.isin(gt, starts)]
    if mid.size:
        lines = np.searchsorted(starts, mid, side="right") - 1
        got |= {"gt_in_header"} if hdr[lines].any() else set()
        got |= {"gt_in_sequence"} if (~hdr[lines]).any() else set()
    return got


def long_inputs():
    """(label, bytes): a header line that covers three whole tiles, and a one-line contig of 3 T + 5 bases"""
    rng = np.random.default_rng(77)
    yield "long_header", b">first\nACGTNN\n>long " + b"h" * (4 * T) + b" tail\nGGCCAT\nacgt\n>last\nTTGCA"
    yield "long_contig", b">x\nAC\n>one_line\n" + seq_bytes(rng, 3 * T + 5) + b"\n>after\nGGC\n"


def tile_cut_ranks(model, off):
    """global base ranks that fall exactly on a tile's prefix"""
    edges = np.arange(T - off, model.n, T)
    return np.unique(np.searchsorted(model.base_pos, edges)).tolist()


def interval_set(model, off, rng):
    """all intervals of a contig of up to 200 bases; else the edges, the tile cuts and one below, the last base, 200 random pairs"""
    q = []
    cuts = tile_cut_ranks(model, off)
    for c, (_, _, rank, length) in enumerate(model.contigs):
        if length <= 200:
            q += [(c, a, b) for a in range(length + 1) for b in range(a, length + 1)]
            continue
        pts = {0, length, 1, length - 1}
        for g in cuts:
            pts |= {p for p in (g - rank, g - rank - 1, g - rank + 1) if 0 <= p <= length}
        pts = sorted(pts)
        q += [(c, a, b) for a in pts for b in pts if a <= b]
        pairs = np.sort(rng.integers(0, length + 1, (200, 2)), axis=1)
        q += [(c, int(a), int(b)) for a, b in pairs]
    return q


def check(scfq, ix, model, q=None, ctx=None):
    s = ix.summary
    assert (s.input_bytes, s.contigs, s.bases, s.gc_bases, s.acgt_bases, s.orphan_bases) == \
        (model.n, len(model.contigs), model.bases, model.gc_bases, model.acgt_bases, model.orphan_bases), ctx
    assert s.struct_size == ctypes.sizeof(scfq.FaSummary) and s.abi_version == 1
    assert ix.contigs == [(c[0].decode("latin-1"), c[1], c[3]) for c in model.contigs], ctx
    if q is not None:
        got = scfq.fa_count_intervals(ix, q)
        want = model.count_many(q)
        assert got.shape == want.shape and (got.astype(np.int64) == want).all(), (ctx, np.flatnonzero((got.astype(np.int64) != want).any(axis=1))[:5])


def check_at_offset(scfq, torch, a, off, rng, ctx):
    model = FaModel(a.tobytes())
    keep, ptr = to_dev(torch, a, off)
    with scfq.fa_index_device(ptr, a.size) as ix:
        assert ix.summary.tiles == ((ptr % T + a.size + T - 1) // T if a.size else 0)
        check(scfq, ix, model, interval_set(model, off, rng), ctx)
    del keep


# ---- the fixture -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fixture_model():
    return FaModel(open(FASTA, "rb").read())


FIX_WINDOWS = (1, 7, 50, 999, 100000)


def fixture_cells(model):
    q = []
    for c in range(3):
        for pos in range(1, 1001, 37):
            q += [(c,) + gc_interval(pos, w, 1000) for w in FIX_WINDOWS]
    return q


@pytest.mark.parametrize("entry", ["device", "host", "file"])
def test_fixture_through_every_entry_point(gpu, scfq, fixture_model, entry):
    data = open(FASTA, "rb").read()
    keep = None
    if entry == "device":
        keep, ptr = to_dev(gpu, np.frombuffer(data, dtype=np.uint8), 0)
        ix = scfq.fa_index_device(ptr, len(data))
    else:
        ix = scfq.fa_index_host(data) if entry == "host" else scfq.fa_index_file(FASTA)
    with ix:
        assert [(c[0], c[2]) for c in ix.contigs] == [("chr1", 1000), ("chr2", 1000), ("chr3", 1000)]
        assert ix.find("chr2") == 1 and ix.find("chr4") is None and ix.find("chr") is None
        check(scfq, ix, fixture_model, fixture_cells(fixture_model), entry)
        for pos, wtext, cell, counts in PINS:
            (chrom, p), = parse_positions(pos)[0]
            w = parse_window(wtext)
            c = ix.find(chrom)
            got = scfq.fa_count_intervals(ix, [(c,) + scfq.fa_gc_interval(p, w, ix.contigs[c][2])])[0]
            assert (int(got[0]), int(got[1])) == counts and scfq.format_fa_gc_value(int(got[0]), int(got[1]), w) == cell


def test_fixture_through_the_cli_and_the_mirror(gpu, scfq, fixture_model, tmp_path):
    for pos, wtext, cell, _ in PINS:
        r = run("fa-gc", "--pos", pos, FASTA, wtext)
        chrom, p = pos.split(":")
        assert (r.returncode, r.stderr, r.stdout) == (0, "", "chrom\tpos\tgc_%d\n%s\t%s\t%s\n" % (2 * int(wtext), chrom, p, cell))
    positions = [("chr%d" % c, pos) for pos in range(1, 1001, 37) for c in (3, 1, 2)]
    path = tmp_path / "all.tsv"
    path.write_text("".join("%s\t%d\n" % p for p in positions))
    want_out, want_err = cli_text(fixture_model, positions, list(FIX_WINDOWS))
    r = run("fa-gc", "--pos", path, FASTA, *FIX_WINDOWS)
    assert (r.returncode, r.stdout, r.stderr) == (0, want_out, want_err) and want_err == ""
    assert scfq.fa_gc(FASTA, str(path), [str(w) for w in FIX_WINDOWS]) == want_out


# ---- tile edges, line widths, endpoints ------------------------------------------------------------------------------

@pytest.mark.parametrize("off", OFFSETS)
def test_tile_edges(gpu, scfq, off):
    rng = np.random.default_rng(100 + off)
    for n in SIZES:
        check_at_offset(scfq, gpu, mixed_input(rng, n, off), off, rng, ("mixed", n, off))
    for label, data in long_inputs():
        check_at_offset(scfq, gpu, np.frombuffer(data, dtype=np.uint8), off, rng, (label, off))


def test_the_edge_inputs_hold_every_case(gpu):
    got = set()
    for off in OFFSETS:
        rng = np.random.default_rng(100 + off)
        for n in SIZES:
            got |= features(mixed_input(rng, n, off), off)
        for label, data in long_inputs():
            got |= features(np.frombuffer(data, dtype=np.uint8), off)
    assert got >= {"nl_then_gt", "nl_then_base", "tile_in_header", "tile_in_sequence", "no_final_nl", "orphans", "twin_headers",
                   "blank_line", "crlf", "gt_in_header", "gt_in_sequence"}, got


@pytest.mark.parametrize("width", [1, 59, 60, 63, 64, 65, 127])
def test_line_widths(gpu, scfq, width):
    rng = np.random.default_rng(width)
    lengths = [(b"w%d_a" % width, 150 + width // 2), (b"w%d_b" % width, (3 * T if width > 1 else T // 2) + 7),
               (b"w%d_c" % width, 2 * width + 1)]
    for off, eol, final in ((0, b"\n", True), (15, b"\r\n", False)):
        data = wrapped(rng, lengths, width, eol, final)
        check_at_offset(scfq, gpu, np.frombuffer(data, dtype=np.uint8), off, rng, (width, off))


# ---- query counts and bad intervals ----------------------------------------------------------------------------------

def test_query_counts_and_bad_intervals(gpu, scfq):
    rng = np.random.default_rng(9)
    data = wrapped(rng, [(b"a", 5000), (b"b", 0), (b"c", 12345)], 70)
    model = FaModel(data)
    L = scfq.lib()
    with scfq.fa_index_host(data) as ix:
        for nq in (0, 1, 63, 64, 65, 4097):
            c = rng.choice([0, 2], nq)
            length = np.array([5000, 0, 12345])[c]
            ab = np.sort((rng.random((nq, 2)) * (length[:, None] + 1)).astype(np.int64), axis=1)
            q = np.column_stack([c, ab]).astype(np.uint64)
            check(scfq, ix, model, q, nq)
        assert scfq.fa_count_intervals(ix, [(1, 0, 0)]).tolist() == [[0, 0, 0]]
        good = [(0, 0, 5000), (2, 5, 9), (0, 7, 7)]
        for bad, word in (((0, 0, 5001), "end > length"), ((2, 9, 5), "begin > end"), ((3, 0, 0), "no such contig"), ((1, 0, 1), "end > length")):
            for at in (0, 2, 3):
                q = np.array((good + good)[:at] + [bad] + good + [(7, 1, 0)], dtype=np.uint64)
                out = np.full((q.shape[0], 3), 0xABCD, dtype=np.uint64)
                assert L.scfq_fa_count_intervals(ix._h, q.ctypes.data, q.shape[0], out.ctypes.data) == scfq.SCFQ_EARG
                detail = L.scfq_fa_error_detail().decode()
                assert detail.startswith("interval %d: %s" % (at, word)) and (out == 0xABCD).all(), detail
        with pytest.raises(scfq.ScfqError) as e:
            scfq.fa_count_intervals(ix, [(0, 0, 1), (0, 2, 1)])
        assert e.value.rc == scfq.SCFQ_EARG and "interval 1" in str(e.value)


# ---- many contigs ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("contigs", [1, 2, 3000])
def test_many_contigs(gpu, scfq, contigs):
    rng = np.random.default_rng(contigs)
    names = [b"n%d" % k for k in range(contigs)]
    names[0] = b"Z"                                                    # a name of one byte
    names[-1] = b"L" * 255 if contigs > 1 else names[-1]               # and of 255
    if contigs > 2:
        names[1700] = names[40]                                         # one name twice
    data = wrapped(rng, [(nm, int(rng.integers(0, 41))) for nm in names], 25, final_eol=contigs != 2)
    model = FaModel(data)
    a = np.frombuffer(data, dtype=np.uint8)
    keep, ptr = to_dev(gpu, a, 1)
    with scfq.fa_index_device(ptr, a.size) as ix:
        q = [(c, x, y) for c in range(0, contigs, max(1, contigs // 60)) for x in range(model.contigs[c][3] + 1)
             for y in range(x, model.contigs[c][3] + 1)]
        check(scfq, ix, model, q, contigs)
        assert ix.find("Z") == 0 and ix.find(names[-1].decode()) == contigs - 1 == model.find(names[-1])
        if contigs > 2:
            assert ix.find("n40") == 40 == model.find(b"n40") and ix.contigs[1700][0] == "n40"


def test_name_limit(gpu, scfq):
    ok = b">" + b"k" * 255 + b"\tdescription\nACGT\n"
    with scfq.fa_index_host(ok) as ix:
        assert ix.contigs == [("k" * 255, 0, 4)]
    with scfq.fa_index_host(b">" + b"k" * 255) as ix:                   # the input ends in the name
        assert ix.contigs == [("k" * 255, 0, 0)]
    for data in (b">a\nAC\n>" + b"k" * 256 + b"\nACGT\n", b">" + b"k" * 256, b">" + b"k" * 5000 + b" x\nAC\n"):
        with pytest.raises(scfq.ScfqError) as e:
            scfq.fa_index_host(data)
        assert e.value.rc == scfq.SCFQ_EARG and "255" in str(e.value) and "contig %d" % (data[1:2] == b"a") in str(e.value)


# ---- one larger input ------------------------------------------------------------------------------------------------

def test_eight_mebibytes(gpu, scfq):
    rng = np.random.default_rng(8)
    per = (8 << 20) // 5 * 60 // 61
    data = wrapped(rng, [(b"chr%d" % k, per - 1000 * k) for k in range(5)], 60)
    model = FaModel(data)
    a = np.frombuffer(data, dtype=np.uint8)
    keep, ptr = to_dev(gpu, a, 16)
    c = rng.integers(0, 5, 10000)
    length = np.array([m[3] for m in model.contigs])[c]
    ab = np.sort((rng.random((10000, 2)) * (length[:, None] + 1)).astype(np.int64), axis=1)
    ab[::7, 1] = np.minimum(length[::7], ab[::7, 0] + rng.integers(0, 200, ab[::7, 0].size))      # short windows too
    with scfq.fa_index_device(ptr, a.size) as ix:
        check(scfq, ix, model, np.column_stack([c, ab]), "8 MiB")


# ---- .gz and BGZF ----------------------------------------------------------------------------------------------------

def test_gz_and_bgzf(gpu, scfq, fixture_model, tmp_path):
    rng = np.random.default_rng(3)
    big = wrapped(rng, [(b"s1", 153000), (b"s2", 0), (b"s3", 153000)], 80)
    assert len(big) > 300 * 1024
    for label, data, positions, windows in (("fixture", open(FASTA, "rb").read(), [("chr3", 10), ("chr1", 1), ("chr2", 1000)], [1, 100000]),
                                            ("big", big, [("s3", 152999), ("s1", 77777), ("s2", 1), ("s1", 1)], [50, 3200])):
        model = FaModel(data)
        plain, gz, bg = tmp_path / (label + ".fa"), tmp_path / (label + ".gzip.fa.gz"), tmp_path / (label + ".bgzf.fa.gz")
        plain.write_bytes(data)
        with gzip.open(gz, "wb") as f:
            f.write(data)
        bg.write_bytes(bgzf_file(data))
        pos = tmp_path / (label + ".pos")
        pos.write_text("".join("%s:%d\n" % p for p in positions))
        want = cli_text(model, positions, windows)
        rows = []
        for path in (plain, gz, bg):
            with scfq.fa_index_file(str(path)) as ix:
                check(scfq, ix, model, interval_set(model, 0, rng) if label == "fixture" else [(0, 5, 149000), (2, 0, 153000)], path)
            r = run("fa-gc", "--pos", pos, path, *windows)
            assert (r.returncode, r.stdout, r.stderr) == (0,) + want, path
            rows.append(r.stdout)
        assert rows[0] == rows[1] == rows[2]


# ---- CLI -------------------------------------------------------------------------------------------------------------

def test_cli_rows_warnings_and_exit_codes(gpu, scfq, fixture_model, tmp_path):
    text = ("chrom\tpos\nchr3\t10\nchrX\t5\nchr1\t1001\nchr1\t1000\nnot a line\nchr2:0\nchr1\t1\n# note\nchr2 500 x\nchr1\t1\n")
    path = tmp_path / "unsorted.bed"
    path.write_text(text)
    positions, warnings = parse_positions(str(path))
    assert positions == [("chr3", 10), ("chrX", 5), ("chr1", 1001), ("chr1", 1000), ("chr2", 0), ("chr1", 1), ("chr2", 500), ("chr1", 1)]
    want_out, want_err = cli_text(fixture_model, positions, [1, 50, 312500000])
    assert want_out.split("\n")[0] == "chrom\tpos\tgc_2\tgc_100\tgc_625000000"
    assert [l.split("\t")[:2] for l in want_out.split("\n")[1:-1]] == [["chr1", "1"], ["chr1", "1"], ["chr1", "1000"], ["chr2", "500"], ["chr3", "10"]]
    assert want_err == warning_line("<chr1:1001> is out of range") + warning_line("<chr2:0> is out of range") + warning_line("<chrX:5> is out of range")
    r = run("fa-gc", "--pos", path, FASTA, "1", "50", "5e5")
    assert (r.returncode, r.stdout) == (0, want_out)
    assert r.stderr == "".join(warning_line(w) for w in warnings) + want_err and len(warnings) == 1
    r = run("fa-gc", "-p", "chr9:1", FASTA, "10")
    assert (r.returncode, r.stdout, r.stderr) == (0, "chrom\tpos\tgc_20\n", warning_line("<chr9:1> is out of range"))
    r = run("fa-gc", FASTA, "10")
    assert (r.returncode, r.stdout, r.stderr) == (1, "", red(1, "Must provide --pos: (chr:100 / bed / vcf )"))
    r = run("fa-gc", "--pos", "chr1:1", FASTA)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", red(1, "Must provide a list of windows: (e.g. 100 200 500)"))
    r = run("fa-gc", "--pos", "chr1:1", FASTA, "0")
    assert (r.returncode, r.stdout, r.stderr) == (1, "", red(1, "Window lengths must be >= 1"))
    r = run("fa-gc", "--pos", "chr1:1", tmp_path / "none.fa", "5")
    assert (r.returncode, r.stdout, r.stderr) == (2, "", red(2, "Unable to open file: %s" % (tmp_path / "none.fa")))
    long_name = tmp_path / "long.fa"
    long_name.write_bytes(b">" + b"k" * 300 + b"\nACGT\n")
    r = run("fa-gc", "--pos", "k:1", long_name, "5")
    assert r.returncode == 1 and r.stdout == "" and "255" in r.stderr


# ---- lifetime --------------------------------------------------------------------------------------------------------

def test_two_indexes_at_once(gpu, scfq, fixture_model):
    rng = np.random.default_rng(21)
    other = wrapped(rng, [(b"p", 9000), (b"q", 777)], 61)
    other_model = FaModel(other)
    a = np.frombuffer(other, dtype=np.uint8)
    keep, ptr = to_dev(gpu, a, 15)
    one = scfq.fa_index_file(FASTA)
    two = scfq.fa_index_device(ptr, a.size)
    q1, q2 = fixture_cells(fixture_model), interval_set(other_model, 15, rng)
    for _ in range(2):
        check(scfq, one, fixture_model, q1, "one")
        check(scfq, two, other_model, q2, "two")
    one.close()
    check(scfq, two, other_model, q2, "two after one is gone")
    three = scfq.fa_index_host(open(FASTA, "rb").read())
    check(scfq, three, fixture_model, q1, "three")
    check(scfq, two, other_model, q2, "two again")
    two.close()
    check(scfq, three, fixture_model, q1, "three after two is gone")
    three.close()

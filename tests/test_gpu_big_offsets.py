"""The record pipelines on device-resident inputs whose offsets pass 2^32, against their checkers: tests/_big_offset_cases.py has the
layout (block x R + tail, just above 2^32 + 2^22 bytes) and the composition of the checkers' results, which
tests/test_big_offset_cases_host.py proves without a GPU.  The repeated part is compared on the device, repetition by repetition, the tail
and everything that is no row on the host; every comparison is ==.  A narrowed offset shows as a repetition next to 2^31 or 2^32 that
differs."""
import os

import numpy as np
import pytest

import _big_offset_cases as C
from conftest import GOLDEN
from _adapters_check import assert_result as assert_adapters
from _cycles_check import assert_result as assert_cycles
from _fa_gc_check import FaModel
from _insert_size_check import assert_result as assert_insert
from _kmers_check import CANONICAL, assert_result as assert_kmers
from _merge_check import assert_stats as assert_merge_stats
from _readstats_check import assert_summary
from _screen_check import assert_stats as assert_screen_stats, assert_summary as assert_screen_index, contigs_of, index_of_np
from _trim_check import assert_stats as assert_trim_stats

pytestmark = pytest.mark.gpu

NAMES = ("spike", "vector", "rrna")
FA = [os.path.join(GOLDEN, "screen", n + ".fa") for n in NAMES]
SENTINEL, GUARD = 0xA5, 256
PAD, AT = 8192, 5                      # guard bytes around an input; its first byte sits AT bytes past a 4 KiB boundary
UNTOUCHED = 0x7777777777777777
OVERLAP_REC = np.dtype([("offset", "<i4"), ("overlap", "<u2"), ("mismatches", "<u2")])
SCREEN_REC = np.dtype([("kmers", "<u4"), ("hit_kmers", "<u4"), ("best_hits", "<u4"), ("mask", "<u2"), ("best", "u1"), ("reserved", "u1")])


class Big:
    """block x R + tail in device memory between guard bytes 'G'; the filler is the block, repeated on the device into the buffer.
    fields: where every header of the block holds FIELD hex digits, which get the repetition number.  at: its first byte sits that many
    bytes past a 4 KiB boundary."""

    def __init__(self, torch, block, tail, R=None, fields=None, at=AT):
        self.torch, self.block, self.tail = torch, block, tail
        self.L = C.layout(block.size, tail.size, R)
        self.R, self.B, self.n, self.fields = self.L["R"], block.size, self.L["n"], fields
        self.t = torch.full((PAD + at + self.n + PAD + 4096,), 0x47, dtype=torch.uint8, device="cuda")
        base = self.t.data_ptr()
        self.start = ((base + PAD + 4095) // 4096) * 4096 - base + at
        self.ptr = base + self.start
        assert self.ptr % 4096 == at and self.start + self.n + PAD <= self.t.numel()
        filler = self.filler().view(self.R, self.B)
        filler.copy_(torch.from_numpy(block.copy()).cuda().expand(self.R, self.B))
        if fields is not None:                                  # one digit of all repetitions' numbers at a time
            r = torch.arange(self.R, device="cuda")
            cols = torch.from_numpy(np.asarray(fields, np.int64)).cuda()
            for j in range(C.FIELD):
                d = (r >> (4 * (C.FIELD - 1 - j))) & 15
                filler[:, cols + j] = torch.where(d < 10, d + 48, d + 87).to(torch.uint8)[:, None]
        self.t[self.start + self.L["filler"]:self.start + self.n] = torch.from_numpy(tail.copy()).cuda()
        torch.cuda.synchronize()

    def filler(self):
        return self.t[self.start:self.start + self.L["filler"]]

    def close(self):
        lo, hi = self.t[:self.start], self.t[self.start + self.n:]
        assert bool((lo == 0x47).all()) and bool((hi == 0x47).all()), "the guard bytes around an input were written"
        self.t = None


class Room:
    """device memory for `size` items between GUARD sentinel items on either side"""

    def __init__(self, torch, size, dtype=None, fill=SENTINEL):
        dtype = dtype or torch.uint8
        self.size, self.fill = size, fill
        self.t = torch.full((2 * GUARD + size,), fill, dtype=dtype, device="cuda")
        self.ptr = self.t.data_ptr() + GUARD * self.t.element_size()
        self.body = self.t[GUARD:GUARD + size]

    def arg(self):
        return (self.ptr, self.size)

    def intact(self, used=None):
        """the guards, and what lies behind the first `used` items"""
        used = self.size if used is None else used
        return bool((self.t[:GUARD] == self.fill).all()) and bool((self.t[GUARD + used:] == self.fill).all())


def on_device(torch, rows):
    a = np.frombuffer(rows, np.uint8) if isinstance(rows, bytes) else np.ascontiguousarray(rows)
    return torch.from_numpy(a.copy()).cuda(), a


def where(r, B):
    """for the message: the input bytes that repetition r stands for, per input (B: a block length, or one per file)"""
    return "; ".join("block of %d bytes: repetition %d is input bytes [%d, %d), 2^31 lies in repetition %d, 2^32 in %d" %
                     (b, r, r * b, (r + 1) * b, 2 ** 31 // b, 2 ** 32 // b) for b in (B if isinstance(B, tuple) else (B,)))


def assert_tiled(torch, got, tiled, ctx, B, chunk=256):
    """got: a device tensor of len(tiled) rows.  Its first R * k rows against the block's k rows, `chunk` repetitions at a time by a broadcast
    == on the device; the rest against the tail's rows on the host.  B: the bytes of input a repetition stands for, for the message."""
    R, step = tiled.R, tiled.step
    blk, want = on_device(torch, tiled.block)
    k = want.shape[0]
    assert got.shape[0] == len(tiled), (ctx, "rows", got.shape[0], len(tiled))
    if k:
        g = got[:R * k].view((R,) + tuple(blk.shape))
        for r0 in range(0, R, chunk):
            part = g[r0:r0 + chunk]
            if step:
                part = part - (torch.arange(r0, r0 + part.shape[0], device="cuda") * step)[:, None]
            eq = (part == blk).flatten(1).all(dim=1)
            if not bool(eq.all()):
                r = r0 + int((~eq).nonzero()[0])
                have = g[r].cpu().numpy() - r * step
                bad = np.flatnonzero((have != want).reshape(k, -1).any(axis=1))
                raise AssertionError((ctx, "repetition %d of %d differs" % (r, R), where(r, B),
                                      "rows", bad[:6].tolist(), "have", have[bad[:3]].tolist(), "want", want[bad[:3]].tolist()))
    tail, want_tail = got[R * k:].cpu().numpy(), np.frombuffer(tiled.tail, np.uint8) if isinstance(tiled.tail, bytes) else tiled.tail
    if step:
        tail = tail - R * step
    if not np.array_equal(tail, want_tail):
        bad = np.flatnonzero((tail != want_tail).reshape(want_tail.shape[0], -1).any(axis=1))
        raise AssertionError((ctx, "the tail differs at rows", bad[:6].tolist(), tail[bad[:3]].tolist(), want_tail[bad[:3]].tolist()))


def packed(recs, dtype):
    """rows of a checker's int64 table as the bytes of the library's records"""
    out = np.zeros(recs.shape[0], dtype)
    for j, name in enumerate(n for n in dtype.names if n != "reserved"):
        out[name] = recs[:, j]
    return out.view(np.uint8).reshape(recs.shape[0], dtype.itemsize)


def packed_tiled(t, dtype):
    return C.Tiled(packed(t.block, dtype), t.R, packed(t.tail, dtype))


@pytest.fixture(autouse=True)
def pool_memory(scfq, gpu):
    before = scfq.lib().scfq_device_bytes_now()
    yield
    gpu.cuda.empty_cache()
    assert scfq.lib().scfq_device_bytes_now() == before
    assert gpu.cuda.max_memory_allocated() < 36e9, "inputs and outputs of the tests stay below 36 GB, which leaves 4 GB for the library's own"


@pytest.fixture(scope="module")
def probes(scfq):
    return [seq.encode() for _, seq in scfq.adapters_default()]


@pytest.fixture(scope="module")
def single(gpu, probes):
    rng = np.random.default_rng(20261011)
    block, fields = C.single_block(rng, probes)
    L = C.layout(block.size, 0)
    reps = (0, L["marks"][2 ** 31], L["marks"][2 ** 32], L["R"] - 1)
    tail = C.single_tail(rng, probes, block, fields, reps)
    big = Big(gpu, block, tail, fields=fields)
    yield big
    big.close()


@pytest.fixture(scope="module")
def ref_texts():
    return [c for p in FA for c in contigs_of(open(p, "rb").read()) if len(c) > 400]


@pytest.fixture(scope="module")
def paired_data(ref_texts):
    rng = np.random.default_rng(20261012)
    return C.paired_blocks(rng, ref_texts), C.paired_tails(rng, ref_texts)


@pytest.fixture(scope="module")
def pair(gpu, paired_data):
    """R1 and R2: blocks of different lengths, repeated equally often"""
    (b1, b2, _), (t1, t2, _) = paired_data
    assert b1.size != b2.size
    R = -(-C.LIMIT // min(b1.size, b2.size))
    bigs = Big(gpu, b1, t1, R), Big(gpu, b2, t2, R)
    yield bigs
    for b in bigs:
        b.close()


@pytest.fixture(scope="module")
def fasta(gpu):
    rng = np.random.default_rng(20261013)
    block, fields, names = C.fasta_block(rng)
    big = Big(gpu, block, C.fasta_tail(rng), fields=fields)
    big.names = names
    yield big
    big.close()


@pytest.fixture(scope="module")
def screen_index(gpu, scfq):
    """(the library's index of the three fixture references, the checker's): built once, before any test's own memory is counted"""
    cindex = index_of_np([(n, open(p, "rb").read()) for n, p in zip(NAMES, FA)], 31)
    with scfq.screen_index_files(FA) as dindex:
        assert_screen_index(dindex.summary, cindex)
        yield dindex, cindex


# ---- the single-end input -----------------------------------------------------------------------------------------------------

def check_index(torch, scfq, big, want, n, ctx):
    lines = want["lines"]
    assert scfq.index_lines_device(big.ptr, n) == lines, ctx
    buf = torch.full((lines + 1 + GUARD,), UNTOUCHED, dtype=torch.int64, device="cuda")
    assert scfq.index_lines_device(big.ptr, n, buf.data_ptr(), lines + 1) == lines, ctx
    assert_tiled(torch, buf[:lines + 1], want["off"], ctx, big.B)            # (the tail's rows end with the sentinel entry)
    assert bool((buf[lines + 1:] == UNTOUCHED).all()), (ctx, "entries behind the sentinel were written")


def check_readstats(torch, scfq, big, want, n, ctx):
    reads = len(want["rows"])
    tab = torch.full((reads + GUARD, 5), -1, dtype=torch.int64, device="cuda")
    s = scfq.read_stats_device(big.ptr, n, tab.data_ptr(), reads)
    assert_tiled(torch, tab[:reads], want["rows"], ctx, big.B)
    assert bool((tab[reads:] == -1).all()), ctx
    assert_summary(s, want["rows"].whole(), want["input_bytes"], want["lines"], ctx)
    assert bytes(scfq.read_stats_device(big.ptr, n)) == bytes(s), (ctx, "the summary without a table")


def check_kmers(scfq, big, want, n, k, flags, ctx):
    assert_kmers(scfq.kmers_device(big.ptr, n, k, flags, True), C.kmers_tuple(want), k, flags, want["input_bytes"], ctx)


def test_line_index(gpu, scfq, single):
    big = single
    want = C.compose_index(C.index_of(big.block), C.index_of(big.tail), big.R, big.B)
    assert want["lines"] % 4 == 0 and big.n > C.LIMIT
    check_index(gpu, scfq, big, want, big.n, "line index")


def test_readstats(gpu, scfq, single):
    big = single
    want = C.compose_readstats(C.readstats_of(big.block), C.readstats_of(big.tail), big.R)
    assert want["input_bytes"] == big.n
    check_readstats(gpu, scfq, big, want, big.n, "readstats")


def test_cycles(gpu, scfq, single):
    big = single
    w = C.compose_cycles(C.cycles_of(big.block), C.cycles_of(big.tail), big.R)
    top = max(w["max_seq_len"], w["max_qual_len"])
    for cap in (top + 3, 100):
        assert_cycles(scfq.cycles_device(big.ptr, big.n, cap), w["table"], w["lines"], w["max_seq_len"], w["max_qual_len"], w["input_bytes"], cap, "cycles")


@pytest.mark.parametrize("k,canonical", [(7, False), (7, True), (12, False), (12, True)])
def test_kmers(gpu, scfq, single, k, canonical):
    big = single
    want = C.compose_kmers(C.kmers_of(big.block, k, canonical), C.kmers_of(big.tail, k, canonical), big.R)
    check_kmers(scfq, big, want, big.n, k, CANONICAL if canonical else 0, ("kmers", k, canonical))


def test_adapters(gpu, scfq, single, probes):
    big = single
    w = C.compose_adapters(C.adapters_of(big.block, probes), C.adapters_of(big.tail, probes), big.R)
    assert sum(w["hits"]) > big.R
    for cap in (w["max_seq_len"] + 3, 64):
        assert_adapters(scfq.adapters_device(big.ptr, big.n, None, cap), C.adapters_tuple(w), probes, cap, w["input_bytes"], "adapters")


@pytest.mark.parametrize("n", C.CUTS)
@pytest.mark.parametrize("what", ["index", "readstats", "kmers"])
def test_length_at_the_edge(gpu, scfq, single, what, n):
    """the same buffer with a length next to 2^31 or 2^32: the input ends inside a record of some repetition"""
    big = single
    assert 0 < n % big.B and n < big.L["filler"]
    ctx = (what, "n = %d: %d repetitions and %d bytes" % (n, n // big.B, n % big.B))
    if what == "index":
        check_index(gpu, scfq, big, C.cut_of(C.index_of, C.compose_index, big.block, n, B=big.B), n, ctx)
    elif what == "readstats":
        check_readstats(gpu, scfq, big, C.cut_of(C.readstats_of, C.compose_readstats, big.block, n), n, ctx)
    else:
        check_kmers(scfq, big, C.cut_of(lambda a: C.kmers_of(a, 7, False), C.compose_kmers, big.block, n), n, 7, 0, ctx)


def test_dedup(gpu, scfq, single):
    """every header of the filler is its own (the repetition number is part of it): the filler comes out as it went in, then the
    tail's records whose headers are new — not those that copy a header of repetition 0, of the repetitions that hold 2^31 and 2^32
    or of the last one, nor the second of a pair within the tail"""
    torch, big = gpu, single
    kept, want = C.dedup_of(big.block, big.fields, big.R, big.tail)
    assert want["duplicates"] == 61
    size, st = scfq.dedup_device(big.ptr, big.n)
    assert (size, {k: int(getattr(st, k)) for k in want}) == (want["bytes_out"], want), "sizing"
    out = Room(torch, want["bytes_out"])
    size, st = scfq.dedup_device(big.ptr, big.n, *out.arg())
    assert (size, {k: int(getattr(st, k)) for k in want}) == (want["bytes_out"], want)
    assert out.intact(), "bytes around the output were written"
    filler, B = big.filler().view(big.R, big.B), big.B
    have = out.body[:big.L["filler"]].view(big.R, big.B)
    for r0 in range(0, big.R, 256):
        eq = (have[r0:r0 + 256] == filler[r0:r0 + 256]).all(dim=1)
        if not bool(eq.all()):
            r = r0 + int((~eq).nonzero()[0])
            at = int((have[r] != filler[r]).nonzero()[0])
            raise AssertionError("output differs from the input in repetition %d of %d, at byte %d of it" % (r, big.R, at), where(r, B),
                                 bytes(have[r, at:at + 60].cpu().numpy()))
    assert out.body[big.L["filler"]:].cpu().numpy().tobytes() == kept
    del out, have


# ---- the paired input ---------------------------------------------------------------------------------------------------------

def check_insert(torch, scfq, want, B, ctx, *bufs):
    pairs = want["pairs"]
    tab = Room(torch, pairs * 8)
    got = scfq.insert_size_device(*bufs, records_ptr=tab.ptr, cap=pairs)
    assert tab.intact(), ctx
    assert_tiled(torch, tab.body.view(pairs, 8), packed_tiled(want["recs"], OVERLAP_REC), ctx, B)
    assert_insert(got, want, ctx)
    s0, h0 = scfq.insert_size_device(*bufs)
    assert bytes(s0) == bytes(got[0]) and np.array_equal(h0, got[1]), (ctx, "without a table")


def test_insert_size_two_files(gpu, scfq, pair, paired_data):
    (b1, b2, _), (t1, t2, _) = paired_data
    p1, p2 = pair
    want = C.compose_insert(C.insert_of(b1, b2), C.insert_of(t1, t2), p1.R)
    assert want["input_bytes1"] == p1.n != p2.n == want["input_bytes2"] and min(p1.n, p2.n) > C.LIMIT
    check_insert(gpu, scfq, want, (p1.B, p2.B), "insert-size, two files", p1.ptr, p1.n, p2.ptr, p2.n)


def test_insert_size_interleaved(gpu, scfq, paired_data):
    (_, _, bi), (_, _, ti) = paired_data
    big = Big(gpu, bi, ti)
    try:
        want = C.compose_insert(C.insert_of(bi), C.insert_of(ti), big.R)
        assert want["input_bytes1"] == big.n and want["unpaired"] == 0
        check_insert(gpu, scfq, want, big.B, "insert-size, interleaved", big.ptr, big.n)
    finally:
        big.close()


def check_outputs(torch, call, sizes, want, names, B, ctx):
    """call(outs) -> stats, for a list of (address, capacity); sizes(stats): the sizes it reports, in the order of `names`"""
    lens = [len(want[k]) for k in names]
    assert sizes(call([None] * len(names))) == lens, (ctx, "sizing")
    outs = [Room(torch, ln) for ln in lens]
    s = call([o.arg() for o in outs])
    assert sizes(s) == lens, ctx
    for k, o in zip(names, outs):
        assert o.intact(), (ctx, k, "bytes around the output were written")
        assert_tiled(torch, o.body, want[k], (ctx, k), B)
    return s


def test_merge(gpu, scfq, pair, paired_data):
    (b1, b2, _), (t1, t2, _) = paired_data
    p1, p2 = pair
    want = C.compose_merge(C.merge_of(b1, b2), C.merge_of(t1, t2), p1.R)
    s = check_outputs(gpu, lambda outs: scfq.merge_device(p1.ptr, p1.n, p2.ptr, p2.n, None, 33, *outs),
                      lambda s: [int(s.merged_bytes), int(s.unmerged1_bytes), int(s.unmerged2_bytes)], want, C.MERGE_OUTPUTS, (p1.B, p2.B), "merge")
    assert_merge_stats(s, want, "merge")
    assert s.merged > p1.R and s.too_long > 20


def test_trim(gpu, scfq, pair, paired_data):
    (b1, b2, _), (t1, t2, _) = paired_data
    p1, p2 = pair
    want = C.compose_trim(C.trim_of(b1, b2, **C.TRIM_ALL), C.trim_of(t1, t2, **C.TRIM_ALL), p1.R)
    opts = scfq.trim_opts(**C.TRIM_ALL)
    s = check_outputs(gpu, lambda outs: scfq.trim_device(p1.ptr, p1.n, p2.ptr, p2.n, opts, *outs), lambda s: [int(s.out1_bytes), int(s.out2_bytes)],
                      want, ("out1", "out2"), (p1.B, p2.B), "trim")
    assert_trim_stats(s, want, "trim")
    assert min(s.cut_overlap, s.cut_adapter, s.cut_polyg, s.cut_quality, s.dropped_reads) > p1.R


def test_screen(gpu, scfq, pair, paired_data, screen_index):
    torch = gpu
    (b1, b2, _), (t1, t2, _) = paired_data
    p1, p2 = pair
    dindex, cindex = screen_index
    want = C.compose_screen(C.screen_of(cindex, b1, b2, **C.SCREEN_KW), C.screen_of(cindex, t1, t2, **C.SCREEN_KW), p1.R)
    reads = want["reads_in"]
    assert reads == len(want["recs"])
    opts = scfq.screen_opts(**C.SCREEN_KW)
    table = Room(torch, 16 * reads)
    s = check_outputs(torch, lambda outs: scfq.screen_device(dindex, p1.ptr, p1.n, p2.ptr, p2.n, opts, *outs, recs=(table.ptr, reads) if outs[0] else None),
                      lambda s: [int(s.out1_bytes), int(s.out2_bytes)], want, ("out1", "out2"), (p1.B, p2.B), "screen")
    assert_screen_stats(s, want, "screen")
    assert table.intact(), "bytes around the per-read table were written"
    assert_tiled(torch, table.body.view(reads, 16), packed_tiled(want["recs"], SCREEN_REC), "screen, per-read records", (p1.B, p2.B))
    assert s.matched_pairs > p1.R and 0 < s.reads_out < s.reads_in


# ---- the FASTA ----------------------------------------------------------------------------------------------------------------

def test_fa_gc(gpu, scfq, fasta):
    big = fasta
    rng = np.random.default_rng(20261014)
    mb, mt = FaModel(big.block), FaModel(big.tail)
    cb, R, B = len(mb.contigs), big.R, big.B
    with scfq.fa_index_device(big.ptr, big.n) as ix:
        s = ix.summary
        assert (s.input_bytes, s.contigs, s.bases, s.gc_bases, s.acgt_bases, s.orphan_bases) == \
            (big.n, R * cb + len(mt.contigs), R * mb.bases + mt.bases, R * mb.gc_bases + mt.gc_bases, R * mb.acgt_bases + mt.acgt_bases, 0)
        assert s.tiles == (big.ptr % 4096 + big.n + 4095) // 4096
        block_rows = [(name, off, ln) for name, (_, off, _, ln) in zip(big.names, mb.contigs)]
        for r in range(R):
            have = ix.contigs[r * cb:(r + 1) * cb]
            want = [((name + b"%08x" % r).decode(), off + r * B, ln) for name, off, ln in block_rows]
            assert have == want, ("contigs of repetition %d of %d" % (r, R), where(r, B), have, want)
        assert ix.contigs[R * cb:] == [(c[0].decode(), c[1] + R * B, c[3]) for c in mt.contigs]
        for r in (0, big.L["marks"][2 ** 31 - 1], big.L["marks"][2 ** 31], big.L["marks"][2 ** 32 - 1], big.L["marks"][2 ** 32], R - 1):
            assert ix.find((big.names[1] + b"%08x" % r)) == r * cb + 1
            q = C.fasta_intervals(rng, mb, r * cb)
            got = scfq.fa_count_intervals(ix, q).astype(np.int64)
            want = mb.count_many([(c - r * cb, lo, hi) for c, lo, hi in q])
            assert (got == want).all(), ("intervals of repetition %d" % r, [q[i] for i in np.flatnonzero((got != want).any(axis=1))[:4]])
        q = C.fasta_intervals(rng, mt, R * cb)
        got = scfq.fa_count_intervals(ix, q).astype(np.int64)
        assert (got == mt.count_many([(c - R * cb, lo, hi) for c, lo, hi in q])).all(), "intervals of the tail"

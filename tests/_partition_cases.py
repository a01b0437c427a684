"""Inputs for the edges of the partitions of fq-readstats, fq-cycles, fq-kmers and fa-gc (seq-collection_amd/csrc/scfq_readstats.hip,
scfq_cycles.hip, scfq_kmers.hip, fa_tile_device.hpp), built where their kernels change path: the LDS stretch of 2048 lines of a
readstats tile and its dense / sparse border protocol, the lanes per line, the position windows and the groups of fq-cycles, the
step of fq-kmers and the chunk behind the input, the tile and step grid of fa-gc.

Every generator is deterministic, needs numpy at most and yields (label, uint8 array, facts); facts says what the case promises
(tests/test_partition_cases_host.py asserts each from the bytes before a device sees them).  The thresholds are read from the
sources (kernel_constants) and handed to the generators: a changed constant moves the cases, or fails here.  A generator whose
layout depends on the pointer's offset takes it as a parameter: tiles, steps and chunks lie on the ADDRESS grid, so an input at
pointer offset `off` has its edges at k * size - off.
"""
import functools
import os
import re

import numpy as np

from conftest import PKG

LF, CRLF = b"\n", b"\r\n"

_SOURCES = (("kRsTile", "scfq_readstats.hip"), ("kRsLineCap", "scfq_readstats.hip"), ("kCyGroup", "scfq_cycles.hip"),
            ("kCyWin", "scfq_cycles.hip"), ("kKmThreads", "scfq_kmers.hip"), ("kFaTileBytes", "fa_tile_device.hpp"),
            ("kFaStepBytes", "fa_tile_device.hpp"))


def kernel_constants():
    """{name: value} of the thresholds the kernels are built with (a literal, or a product of literals)"""
    out = {}
    for name, src in _SOURCES:
        text = open(os.path.join(PKG, "csrc", src)).read()
        m = re.search(r"constexpr uint32_t %s = (\d+(?: \* \d+)*);" % name, text)
        assert m, "%s is no longer a literal in %s" % (name, src)
        out[name] = int(np.prod([int(f) for f in m.group(1).split("*")], dtype=np.int64))
    assert out["kRsTile"] % 16 == 0 and out["kRsLineCap"] % 4 == 0 and out["kCyGroup"] % 2 == 0 and out["kCyWin"] % 16 == 0
    assert out["kFaTileBytes"] % out["kFaStepBytes"] == 0
    return out


# ---- text -------------------------------------------------------------------------------------------------------------------
_POOL = 1 << 17
_MIX = ((np.arange(_POOL, dtype=np.int64) * 2654435761) >> 13)


def _pool(alphabet):
    return np.frombuffer(alphabet, dtype=np.uint8)[_MIX % len(alphabet)].tobytes()


_SEQ5 = _pool(b"ACGTN")                       # fq-readstats: G|C, N and the rest
_SEQX = _pool(b"ACGTNacgtX")                  # fq-cycles: the five letters and "other"
_SEQ4 = _pool(b"ACGT")
_SEQ4N = _pool(b"ACGTACGTACGTACGTN")          # fq-kmers: mostly k-mers, some skipped windows
_LOWER = _pool(b"abcdefghijklmnopqrstuvwxyz")
_QUAL = (33 + (_MIX >> 3) % 94).astype(np.uint8).tobytes()


def _take(pool, length, salt):
    """`length` bytes whose letters depend on the position and on salt"""
    at = (salt * 131 + 17) % (_POOL - length)
    return pool[at:at + length]


def _line(j, length, seq_pool=_SEQ5):
    """text of `length` bytes for line j of a FASTQ: '@...', bases, '+...', quality bytes"""
    if length == 0:
        return b""
    role = j & 3
    if role == 0:
        return b"@" + _take(_LOWER, length - 1, j)
    if role == 1:
        return _take(seq_pool, length, j)
    if role == 2:
        return b"+" + _take(_LOWER, length - 1, j)
    return _take(_QUAL, length, j)


class _Lines:
    """a FASTQ written line by line: pos is the offset of the next line, j its number"""

    def __init__(self, seq_pool=_SEQ5):
        self.parts, self.pos, self.j, self.seq_pool = [], 0, 0, seq_pool

    def add(self, length, eol=LF):
        text = _line(self.j, length, self.seq_pool)
        self.parts += [text, eol]
        self.pos += len(text) + len(eol)
        self.j += 1

    def record(self, header, seq, plus, qual, eol=LF):
        for length in (header, seq, plus, qual):
            self.add(length, eol)

    def array(self):
        return np.frombuffer(b"".join(self.parts), dtype=np.uint8)


def _sparse_record(b, k):
    """a record of 1 to 3 KB"""
    b.record(6 + k % 20, 400 + (k * 211) % 1000, 1 + k % 3, 400 + ((k + 1) * 211) % 1000)


_SPARSE_MAX = 3000       # no record of _sparse_record is longer


# ---- R1: fq-readstats, the LDS stretch ---------------------------------------------------------------------------------------
def r1_lds_cap(T, C, offset):
    """Three tiles.  The outer two hold records of 1 to 3 KB; the middle one, bytes [T - offset, 2 T - offset), has exactly
    C - 1, C, C + 1 or C + 2 lines with a byte (text or newline) in it, the first of them line 4 i + phase for every phase.
    The first of those lines starts in the tile before; with phase 0 or 1 the last one ends in the tile behind, with phase 2 or
    3 its '\\n' is the tile's last byte."""
    for count in (C - 1, C, C + 1, C + 2):
        for phase in range(4):
            yield _r1_case(T, C, offset, count, phase)


def _r1_case(T, C, offset, count, phase):
    lo, hi, end = T - offset, 2 * T - offset, 3 * T - offset
    exact = phase >= 2
    b, k = _Lines(), 0
    while b.pos + _SPARSE_MAX <= lo - 400:
        _sparse_record(b, k)
        k += 1
    for _ in range(phase):
        b.add(50)
    assert b.pos < lo and (b.j & 3) == phase
    first = b.j
    b.add(lo + 100 - b.pos - 1)                       # its '\n' is byte lo + 99 of the input
    fill, fill_end = (count - 1, hi) if exact else (count - 2, hi - 100)
    base, extra = divmod(fill_end - b.pos, fill)
    assert base >= 1, "a tile of %d bytes does not hold %d lines" % (T, count)
    for i in range(fill):
        b.add(base + (i < extra) - 1)
    assert b.pos == fill_end
    if not exact:
        b.add(1000)                                   # from hi - 100 across the border
    assert b.j == first + count
    while b.j & 3:
        b.add(500 + 37 * (b.j & 3))
    while b.pos + _SPARSE_MAX <= end:
        _sparse_record(b, k)
        k += 1
    assert 2 * T < b.pos + offset <= 3 * T
    facts = dict(family="R1", T=T, C=C, offset=offset, lines_in_middle=count, phase=phase, dense=count > C, ends_on_border=exact)
    return "R1/offset=%d/lines=%d/phase=%d" % (offset, count, phase), b.array(), facts


# ---- R2: fq-readstats, dense and sparse tiles side by side -------------------------------------------------------------------
R2_TILES = "SDSDDS"
R2_PADS = range(130)
R2_CUTS = ("header", "seq_first", "seq", "cr_lf", "lf", "plus", "qual", "record_start")
_R2_HEADER = 8           # text bytes of the first header before it is lengthened


@functools.lru_cache(maxsize=4)
def _r2_body(T, C):
    avg = T // (2 * C)                                # bytes per line of a dense tile
    assert avg >= 6, "tiles of %d bytes and %d lines leave no room for short records" % (T, C)
    seq = avg + 1
    header = 4 * avg - 7 - 2 * seq
    b, k, r = _Lines(), 0, 0

    def small():
        nonlocal r
        b.record(header, seq, 3, seq, CRLF if r % 3 == 0 else LF)
        r += 1

    b.record(_R2_HEADER, 700, 1, 700)
    while b.pos + _SPARSE_MAX <= T - 300:             # tile 0: sparse, short records only in its last 3 KB
        _sparse_record(b, k)
        k += 1
    while b.pos < 2 * T - 1000:                       # tile 1: dense
        small()
    b.add(10)
    b.add(3 * T + 1000 - b.pos)                       # tile 2 lies inside this sequence line for every pad
    b.add(1)
    b.add(30)
    while b.pos < 5 * T + 40:                         # tiles 3 and 4: dense
        small()
    while b.pos + _SPARSE_MAX <= 6 * T - 200:         # tile 5: sparse
        _sparse_record(b, k)
        k += 1
    assert 5 * T < b.pos and b.pos + max(R2_PADS) <= 6 * T
    return b"".join(b.parts)


def r2_borders(T, C, pads=R2_PADS):
    """Six tiles at pointer offset 0: sparse, dense, sparse (inside one long sequence line), dense, dense, sparse.  A dense tile
    holds about 2 C lines of short records, every third of them with "\\r\\n".  The first header grows by pad bytes: over pads
    0 .. 129 every kind of border (S>D, D>S, D>D) cuts a record at every place of R2_CUTS."""
    body = _r2_body(T, C)
    for pad in pads:
        data = body[:_R2_HEADER] + b"h" * pad + body[_R2_HEADER:]
        yield "R2/pad=%d" % pad, np.frombuffer(data, dtype=np.uint8), dict(family="R2", T=T, C=C, offset=0, pad=pad, tiles=R2_TILES)


# ---- C1: fq-cycles, lanes per line ------------------------------------------------------------------------------------------
C1_LONGEST = (1, 48, 49, 50, 112, 113, 114, 240, 241, 242, 496, 497, 498)      # (gm + 15) / 16 chunks: 4 | 5, 8 | 9, 16 | 17, 32 | 33
C1_RECORDS = 67


def c1_lane_tiers(longest):
    """67 records (no multiple of any lines-per-step) whose sequence and quality lengths run through 0 .. longest; the longest
    line of the one group is a sequence line in one case and a quality line in the other"""
    for where in ("seq", "qual"):
        parts = []
        for i in range(C1_RECORDS):
            sl, ql = (i * 29 + 3) % (longest + 1), (i * 53 + longest) % (longest + 1)
            sl, ql = (0 if i == 0 else sl), (0 if i == 1 else ql)
            if where == "seq":
                sl, ql = (longest if i == 40 else sl), min(ql, longest - 1)
            else:
                sl, ql = min(sl, longest - 1), (longest if i == 40 else ql)
            eol = CRLF if i % 3 == 1 else LF
            parts += [b"@" + _take(_LOWER, i % 23, i), eol, _take(_SEQX, sl, i), eol, b"+", eol, _take(_QUAL, ql, i + 1000), eol]
        facts = dict(family="C1", longest=longest, longest_in=where, records=C1_RECORDS)
        yield "C1/longest=%d/%s" % (longest, where), np.frombuffer(b"".join(parts), dtype=np.uint8), facts


# ---- C2: fq-cycles, the number of windows -----------------------------------------------------------------------------------
C2_RECORDS = 100


def c2_tops(win):
    """line lengths around the places where (longest + 15) / win changes: win = 1024 gives 1008 1009 1010 1023 1024 1025 2033 2034"""
    return (win - 16, win - 15, win - 14, win - 1, win, win + 1, 2 * win - 15, 2 * win - 14)


def c2_window_edge(win, top):
    """100 records, most lines shorter than 500.  Sixteen lines (sequence and quality in turn) have `top` bytes and start, at
    pointer offset 0, d = 0 .. 15 bytes into a 16-byte chunk: the header before them is as long as that takes.  Other lines take
    the lengths of c2_tops below top."""
    lower = [v for v in c2_tops(win) if v < top]
    parts, pos, d_seen, others = [], 0, [], 0
    for i in range(C2_RECORDS):
        eol = CRLF if i % 4 == 1 else LF
        e = len(eol)
        sl, ql, hl = (i * 37) % 500, (i * 61 + 11) % 500, 5 + i % 7
        if i % 6 == 3 and i // 6 < 16:
            d = i // 6
            if d % 2 == 0:
                sl = top
                hl = 5 + (d - (pos + 5 + e)) % 16
            else:
                ql = top
                hl = 5 + (d - (pos + 5 + e + sl + e + 1 + e)) % 16
            d_seen.append(d)
        elif i % 6 == 0 and lower:
            if others % 2:
                sl = lower[(others // 2) % len(lower)]
            else:
                ql = lower[(others // 2) % len(lower)]
            others += 1
        rec = [b"@" + _take(_LOWER, hl - 1, i), eol, _take(_SEQX, sl, i), eol, b"+", eol, _take(_QUAL, ql, i + 500), eol]
        parts += rec
        pos += sum(map(len, rec))
    assert d_seen == list(range(16))
    facts = dict(family="C2", win=win, top=top, records=C2_RECORDS, d_values=d_seen, long_lines=16)
    return "C2/top=%d" % top, np.frombuffer(b"".join(parts), dtype=np.uint8), facts


# ---- C3: fq-cycles, groups -----------------------------------------------------------------------------------------------
def c3_group_edge(group):
    """reads of at most 20 bases.  A group is `group` sequence and quality lines, group / 2 records: one record less than a
    group, a whole group, one more, two groups and a record, the same cut behind its last sequence line, and three groups of
    which one (each in turn) has empty sequence and quality lines only"""
    per = group // 2
    variants = [("one_less", per - 1, None, False), ("whole", per, None, False), ("one_more", per + 1, None, False),
                ("two_and_one", 2 * per + 1, None, False), ("two_and_a_sequence_line", 2 * per + 1, None, True)]
    variants += [("empty_group_%d" % g, 3 * per, g, False) for g in range(3)]
    for name, records, empty, cut in variants:
        parts = []
        for i in range(records):
            eol = CRLF if i % 5 == 2 else LF
            sl, ql = (i * 7 + 1) % 21, (i * 11 + 5) % 21
            if empty is not None and i // per == empty:
                sl = ql = 0
            rec = [b"@" + _take(_LOWER, i % 9, i), eol, _take(_SEQX, sl, i), eol, b"+", eol, _take(_QUAL, ql, i + 77), eol]
            if cut and i == records - 1:
                rec = rec[:2] + [_take(_SEQX, 20, i)]                    # no '\n' behind it
            parts += rec
        odd = 2 * records - (1 if cut else 0)
        populations = [min(group, odd - g * group) for g in range((odd + group - 1) // group)]
        facts = dict(family="C3", group=group, records=records, populations=populations, empty_group=empty, ends_in_sequence=cut)
        yield "C3/%s" % name, np.frombuffer(b"".join(parts), dtype=np.uint8), facts


# ---- fq-kmers ---------------------------------------------------------------------------------------------------------------
def _fq_fill(nbytes, salt=0):
    """exactly nbytes of whole records"""
    assert nbytes == 0 or nbytes >= 6, nbytes
    parts, left, i = [], nbytes, 0
    while left:
        length = 20 + (i * 37 + salt) % 90
        eol = CRLF if i % 4 == 2 else LF
        rec = b"".join([b"@r%d" % i, eol, _take(_SEQ4N, length, i + salt), eol, b"+", eol, _take(_QUAL, length, i + salt), eol])
        if left == len(rec) or left - len(rec) >= 6:
            parts.append(rec)
            left -= len(rec)
        else:
            s = (left - 6) // 2
            parts.append(b"@\n" + _take(_SEQ4N, s, salt) + b"\n+\n" + _take(_QUAL, left - 6 - s, salt) + b"\n")
            left = 0
        i += 1
    return b"".join(parts)


K1_ENDINGS = ("short", "long", "long_cr", "lf")
K1_LAST = {"short": b"ACGTA", "long": b"GATTACAGATTACACCGTAT", "long_cr": b"GATTACAGATTACACCGTAT\r", "lf": b"GATTACAGATTACACCGTAT\n"}


def k1_totals(step):
    """shift + n: around a wave's 64 chunks (every residue of 16 that matters, below a step), around a step, two steps"""
    return (1023, 1024, 1025, step - 1, step, step + 1, 2 * step)


def k1_behind_the_input(step, shift, endings=K1_ENDINGS):
    """inputs of n = total - shift bytes for a pointer at offset shift, so that the position behind the input is the last byte
    of a chunk, the first byte of a chunk of its own (of a step and a block of its own at total = step, 2 step) or the second;
    they end in a sequence line of 5 bases without '\\n', of 20, of 20 and a bare '\\r', or of 20 and '\\n'"""
    for total in k1_totals(step):
        for ending in endings:
            tail = b"@t\n" + K1_LAST[ending]
            n = total - shift
            data = _fq_fill(n - len(tail), total) + tail
            assert len(data) == n
            facts = dict(family="K1", step=step, shift=shift, total=total, residue=total % 16, ending=ending,
                         last_line=K1_LAST[ending].rstrip(b"\n"))
            yield "K1/total=%d/%s/shift=%d" % (total, ending, shift), np.frombuffer(data, dtype=np.uint8), facts


K2_DELTAS = range(-13, 3)


def k2_edges_inside(edge, shift, eols=(LF, CRLF), deltas=K2_DELTAS):
    """a sequence line whose "\\n" or "\\r\\n" begins at byte edge + delta of the address grid (edge: 1024, the chunks of a wave,
    or a step) for delta = -13 .. 2, an empty quality line and a second sequence line right behind it, and one N in a sequence
    line as near to the edge as the layout allows (12 bytes at most)"""
    for eol in eols:
        for delta in deltas:
            eol_at = edge + delta - shift
            a_start = eol_at - 40 - 3
            head = _fq_fill(a_start, edge + delta)
            a = b"@a\n" + _take(_SEQ4, 40, delta + 50) + eol + b"+" + eol + eol
            b_start = a_start + len(a)
            data = bytearray(head + a + b"@\n" + _take(_SEQ4, 60, delta + 90) + b"\n+\n" + _take(_QUAL, 60, delta) + b"\n" + _fq_fill(200, 3))
            text = set(range(a_start + 3, eol_at)) | set(range(b_start + 2, b_start + 62))
            near = sorted((x for x in text if abs(x + shift - edge) <= 12), key=lambda x: (abs(x + shift - edge), x))
            assert near, (edge, delta, shift)
            data[near[0]] = ord("N")
            facts = dict(family="K2", edge=edge, shift=shift, delta=delta, eol=eol, eol_at=eol_at, bad_at=near[0])
            yield "K2/edge=%d/delta=%d/%s/shift=%d" % (edge, delta, "crlf" if eol == CRLF else "lf", shift), np.frombuffer(bytes(data), dtype=np.uint8), facts


K3_RUNS = (15, 16, 17, 1024, 1025, 5000)


def k3_merge(m):
    """one sequence line of A x m, T x m, A x m (the canonical k-mers of the A run and the T run are equal: a lane of sixteen
    windows of one k-mer next to one of another WORD and the same index), and one of C x m, G x m.  run_starts: where the
    second (and third) run begins; a pointer offset of -run_start mod 16 puts it on a lane's first byte"""
    for name, seq in (("ATA", b"A" * m + b"T" * m + b"A" * m), ("CG", b"C" * m + b"G" * m)):
        data = b"@h\n" + seq + b"\n+\n" + b"I" * 7 + b"\n"
        facts = dict(family="K3", m=m, runs=name, seq_len=len(seq), run_starts=[3 + r * m for r in range(1, len(name))])
        yield "K3/%s/m=%d" % (name, m), np.frombuffer(data, dtype=np.uint8), facts


# ---- fa-gc ------------------------------------------------------------------------------------------------------------------
def fa_offsets(tile, step):
    """pointer offsets that put the input's first byte around a step edge and into the last bytes of a tile"""
    return (step - 16, step - 1, step, step + 1, 2 * step - 1, 2 * step, tile - 17, tile - 16, tile - 15, tile - 1)

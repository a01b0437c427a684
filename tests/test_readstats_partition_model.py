"""A Python model of how R1 (csrc/scfq_readstats.hip: rs_borders + rs_reduce) partitions its work: by BYTES, a block per tile.
A record that lies inside one tile is stored by it, a record that crosses a tile border is zeroed by the border pass and added to
by every tile it touches, its lengths by the tile its first byte lies in; a tile with more lines than the LDS stretch holds adds
everything.  The model walks the same tiles, 16-byte chunks and line segments with the same index arithmetic and checks that every
table entry is written exactly once (one store and nothing else, or zero + adds) and that the table equals per_read()."""
import os
import random
import re

from conftest import PKG
from _readstats_check import lines_of, per_read


def kernel_constants():
    """the tile and the LDS line capacity the kernels are built with"""
    src = open(os.path.join(PKG, "csrc", "scfq_readstats.hip")).read()
    return tuple(int(re.search(r"constexpr uint32_t %s = (\d+);" % name, src).group(1)) for name in ("kRsTile", "kRsLineCap", "kRsThreads"))


def line_index(data):
    """K5: line_off[0 .. lines] with the sentinel one past the (real or implied) final newline"""
    n = len(data)
    off = [0] + [k + 1 for k in range(n) if data[k] == 10]
    if off[-1] >= n:
        off.pop()                           # nothing follows a final '\n'; an empty input has no line
    lines = len(off)
    off.append((n if data.endswith(b"\n") else n + 1) if lines else 0)
    return off, lines


def first_line_at_or_after(off, lines, x):
    a, b = 0, lines
    while a < b:
        m = a + (b - a) // 2
        if off[m] >= x:
            b = m
        else:
            a = m + 1
    return a


def text_len(data, off, lines, k, has_cr):
    if k >= lines:
        return 0
    s, nl = off[k], off[k + 1] - 1
    e = nl
    if has_cr and nl < len(data) and e > s and data[e - 1] == 13:
        e -= 1
    return e - s


def run_model(data, T, shift, line_cap, has_cr=True):
    n = len(data)
    off, lines = line_index(data)
    reads = (lines + 3) // 4
    assert lines == len(lines_of(data))
    if reads == 0:
        return []
    table = [None] * reads                  # None: never written (device memory is not zero)
    stores = [0] * reads
    adds = [0] * reads
    zeroed = [0] * reads
    n_tiles = (n + shift + T - 1) // T

    def tile_lo(t):
        a = t * T
        return 0 if a <= shift else min(a - shift, n)

    def geometry(t):
        lo = tile_lo(t)
        hi = n if t + 1 == n_tiles else tile_lo(t + 1)
        ja, jb = first_line_at_or_after(off, lines, lo), first_line_at_or_after(off, lines, hi)
        j_first = ja if off[ja] == lo else ja - 1
        j_last = jb - 1 if (jb >= 1 and jb - 1 > j_first) else j_first
        assert 0 <= j_first <= j_last < lines and j_last + 1 <= lines
        assert off[j_first] <= lo < off[j_first + 1]
        return lo, hi, ja, jb, j_first, j_last, (j_last - j_first + 1) > line_cap

    # R0: the border pass
    for t in range(n_tiles):
        lo, hi, ja, jb, j_first, j_last, dense = geometry(t)
        assert lo < hi
        if dense:
            for r in range(j_first >> 2, (j_last >> 2) + 1):
                table[r] = [0] * 5
                zeroed[r] += 1
        elif off[4 * (j_first >> 2)] < lo:
            table[j_first >> 2] = [0] * 5
            zeroed[j_first >> 2] += 1

    def add(r, field, v):
        if v:
            assert table[r] is not None and stores[r] == 0, ("add to an entry nobody zeroed", r)
            table[r][field] += v
            adds[r] += 1

    # R1
    for t in range(n_tiles):
        lo, hi, ja, jb, j_first, j_last, dense = geometry(t)
        t0 = t * T - shift
        r_first = j_first >> 2
        slots = {}
        for c in range(T // 16):
            c0 = t0 + 16 * c
            v0, v1 = max(c0, lo), min(c0 + 16, hi)
            if v0 >= v1:
                continue
            a, b = j_first, j_last + 1
            while b - a > 1:
                m = a + (b - a) // 2
                if off[m] <= v0:
                    a = m
                else:
                    b = m
            j, p = a, v0
            while True:
                assert j <= j_last
                nl = off[j + 1] - 1
                te = min(nl, v1)
                if has_cr and nl < n and nl - 1 >= p and nl - 1 < v1 and data[nl - 1] == 13:
                    te = nl - 1
                if te > p and (j & 1):
                    seg = data[p:te]
                    acc = slots.setdefault(j >> 2, [0, 0, 0])
                    if (j & 3) == 1:
                        acc[0] += seg.count(b"G") + seg.count(b"C")
                        acc[1] += seg.count(b"N")
                    else:
                        acc[2] += sum(seg)
                if nl >= v1:
                    break
                p = nl + 1
                j += 1
                if p >= v1:
                    break
        if dense:
            for r, (gc, nb, qs) in slots.items():
                add(r, 1, gc), add(r, 2, nb), add(r, 4, qs)
            r = (ja + 3) // 4
            while 4 * r < jb:
                add(r, 0, text_len(data, off, lines, 4 * r + 1, has_cr))
                add(r, 3, text_len(data, off, lines, 4 * r + 3, has_cr))
                r += 1
            continue
        n_slots = (j_last >> 2) - r_first + 1
        assert n_slots <= line_cap // 4 + 2 and j_last - j_first + 2 <= line_cap + 2
        for s in range(n_slots):
            r = r_first + s
            gc, nb, qs = slots.get(r, [0, 0, 0])
            end_line = min(4 * r + 4, lines)
            owner = off[4 * r] >= lo
            inside = owner and (off[end_line] <= hi or t + 1 == n_tiles)
            sl = text_len(data, off, lines, 4 * r + 1, has_cr) if owner else 0
            ql = text_len(data, off, lines, 4 * r + 3, has_cr) if owner else 0
            if inside:
                assert zeroed[r] == 0 and adds[r] == 0 and stores[r] == 0, ("a stored entry is touched twice", r)
                table[r] = [sl, gc, nb, ql, qs]
                stores[r] += 1
            else:
                add(r, 0, sl), add(r, 1, gc), add(r, 2, nb), add(r, 3, ql), add(r, 4, qs)
    for r in range(reads):
        assert table[r] is not None, ("entry never written", r)
        assert (stores[r] == 1 and adds[r] == 0 and zeroed[r] == 0) or (stores[r] == 0 and zeroed[r] >= 1), r
    return [tuple(x) for x in table]


def check(data, T, shift=0, line_cap=8, has_cr=True):
    assert run_model(data, T, shift, line_cap, has_cr) == per_read(data), (data[:80], T, shift, line_cap)


def test_the_kernels_geometry():
    """one input at the tile size and LDS capacity of the build: Illumina-like records, a read of three tiles, a stretch of short lines"""
    T, line_cap, threads = kernel_constants()
    assert T % (16 * threads) == 0 and line_cap % 4 == 0
    rng = random.Random(5)
    rec = lambda L: b"@read\n" + bytes(rng.choice(b"ACGTN") for _ in range(L)) + b"\n+\n" + bytes(rng.choice(b"FI#5") for _ in range(L)) + b"\n"
    data = b"".join(rec(150) for _ in range(300)) + rec(3 * T + 1) + b"\n" * (line_cap + 700) + b"".join(rec(rng.randrange(0, 40)) for _ in range(200))
    for shift in (0, 9):
        check(data, T, shift, line_cap, has_cr=False)


def test_special_line_lengths():
    for T in (16, 32, 64):
        for L in (0, 1, T - 1, T, T + 1, 3 * T):
            for eol in (b"\n", b"\r\n"):
                rec = b"@h" + eol + b"GCN" * (L // 3) + b"A" * (L % 3) + eol + b"+" + eol + b"I" * L + eol
                for shift in (0, 5, 15):
                    check(rec * 3, T, shift)
                    check(rec * 3 + rec[:-len(eol)], T, shift)          # no final newline
                    check((rec * 2)[:-1], T, shift)                      # "\r" as the last byte of a CRLF file
    for T in (16, 64):
        check(b"", T)
        check(b"\n", T)
        check(b"x", T)
        check(b"@a\r", T)
        check(b"ACGTNGC" * 40, T)                                        # no newline at all
        check(b"\r\n" * 100, T)
        check(b"\n" * 300, T)
        check(b"\n" * 300, T, line_cap=2048)


def test_random_layouts():
    rng = random.Random(20260117)
    alphabets = (b"ACGTN\n", b"GCNI\r\n\n", b"ACGTNacgtn@+FI#:,\r\n\n\n", bytes(range(256)), b"\n\n\n\nG\r")
    for trial in range(400):
        T = rng.choice((16, 32, 48, 64, 128))
        line_cap = rng.choice((4, 8, 16, 2048))
        kind = rng.randrange(3)
        if kind == 0:                       # random bytes
            alpha = rng.choice(alphabets)
            data = bytes(rng.choice(alpha) for _ in range(rng.randrange(0, 600)))
        elif kind == 1:                     # lines of chosen lengths, some of them empty, some around a tile
            eol = rng.choice((b"\n", b"\r\n"))
            parts = []
            for _ in range(rng.randrange(1, 40)):
                L = rng.choice((0, 0, 1, 2, 15, 16, 17, T - 1, T, T + 1, 3 * T, rng.randrange(0, 200)))
                parts.append(bytes(rng.choice(b"ACGTN\rI") for _ in range(L)) + eol)
            data = b"".join(parts)
            if rng.random() < 0.5:
                data = data[:len(data) - rng.randrange(0, 3)]
        else:                               # one long line among short ones
            data = b"@r\n" + bytes(rng.choice(b"ACGTN") for _ in range(rng.randrange(200, 900))) + b"\n+\n" + b"I" * rng.randrange(0, 300)
        has_cr = True if rng.random() < 0.5 else (b"\r\n" in data)
        check(data, T, rng.randrange(0, 16), line_cap, has_cr)

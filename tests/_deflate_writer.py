"""A seeded DEFLATE writer (RFC 1951) for the inflater tests: the stream shapes that zlib's compressor never emits but that the
format allows and zlib's inflate accepts (distances 32 507 - 32 768, length 258 as code 284 + 31, one or no distance codes, precode
runs across the literal/length | distance border, HLIT 257 / 286, HDIST 1 / 30, HCLEN 19, 15-bit codes on used symbols, codes whose
two-level tables are near the decoders' LDS reserve, empty stored blocks between dynamic ones), and streams that every decoder has to
reject.  Pure Python; a helper module for the tests, not a conftest.

A stream is built by `Builder`: bytes go in as literals, greedy LZ77 matches or explicit copies (distance, length, optionally a forced
length code and extra value), and `Builder.cut(...)` closes a block with the code shape chosen for it.  `Builder.data` is what the
stream inflates to; `Builder.deflate()` the raw DEFLATE bytes."""
import heapq
import random
import struct
import zlib


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
LIT_ROOT, DIST_ROOT = 10, 8                   # the device tables' first-level bits (bgzf_inflate_kernel.hpp: kLitRoot, kDistRoot)
LIT_ENTRIES, DIST_ENTRIES = 1344, 416         # and their LDS reserve (kLitEntries, kDistEntries)


def _len_sym(n):
    if n == 258:
        return 285, 0, 0
    k = 0
    while k + 1 < 28 and LEN_BASE[k + 1] <= n:
        k += 1
    return 257 + k, LEN_EXTRA[k], n - LEN_BASE[k]


_LEN_TAB = [None] * 3 + [_len_sym(n) for n in range(3, 259)]


def _dist_sym(d):
    k = 0
    while k + 1 < 30 and DIST_BASE[k + 1] <= d:
        k += 1
    return k, DIST_EXTRA[k], d - DIST_BASE[k]


_DIST_TAB = [None] + [_dist_sym(d) for d in range(1, 32769)]


# ---- bit writer ----------------------------------------------------------------------------------------------------------------
class BitWriter:
    """LSB-first fields into an integer accumulator, flushed in 4 KiB pieces; Huffman codes go in pre-reversed."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, v, n):
        self.acc |= v << self.n
        self.n += n
        if self.n >= 4096:
            self.out += (self.acc & ((1 << 4096) - 1)).to_bytes(512, "little")
            self.acc >>= 4096
            self.n -= 4096

    def align(self):
        self.put(0, -self.n & 7)

    @property
    def bitpos(self):
        return 8 * len(self.out) + self.n

    def getvalue(self):
        return bytes(self.out) + self.acc.to_bytes((self.n + 7) >> 3, "little")


def _rev(v, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (v & 1)
        v >>= 1
    return r


def canonical(lens):
    """RFC 1951 3.2.2: code lengths -> [(bit-reversed code, length)] per symbol (length 0: no code).  Over-subscribed lengths still
    give codes (truncated), so that invalid streams can be written."""
    mx = max(lens) if lens else 0
    bl = [0] * 16
    for n in lens:
        bl[n] += 1
    bl[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, mx + 1):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    out = []
    for n in lens:
        if n:
            out.append((_rev(nxt[n] & ((1 << n) - 1), n), n))
            nxt[n] += 1
        else:
            out.append((0, 0))
    return out


def kraft(lens, bits=15):
    return sum(1 << (bits - n) for n in lens if n)


def huffman_lengths(freq, limit):
    """length-limited Huffman code lengths (frequencies halved until the limit holds); at least two codes, so the code is complete"""
    freq = list(freq)
    used = [i for i, f in enumerate(freq) if f]
    if len(used) < 2:
        for i in range(len(freq) - 1, -1, -1):
            if i not in used:
                used.append(i)
                freq[i] = 1
                if len(used) == 2:
                    break
    while True:
        heap = [(freq[i], i, (i,)) for i in used]
        heapq.heapify(heap)
        depth = [0] * len(freq)
        tie = len(freq)
        while len(heap) > 1:
            fa, _, a = heapq.heappop(heap)
            fb, _, b = heapq.heappop(heap)
            for s in a + b:
                depth[s] += 1
            heapq.heappush(heap, (fa + fb, tie, a + b))
            tie += 1
        if max(depth) <= limit:
            return depth
        freq = [(f + 1) >> 1 if f else 0 for f in freq]


def complete_code(n, fixed, pool):
    """lengths for n symbols: `fixed` {symbol: length} as given, the rest of the Kraft sum filled with symbols from `pool` (the
    binary digits of what is left, shortest first): a complete code in which the fixed symbols have exactly their lengths"""
    lens = [0] * n
    for s, ln in fixed.items():
        lens[s] = ln
    rem = (1 << 15) - kraft(lens)
    assert rem >= 0, "over-subscribed"
    free = [s for s in pool if s not in fixed]
    for ln in range(1, 16):
        if rem & (1 << (15 - ln)):
            lens[free.pop(0)] = ln
    return lens


# ---- what build_table (bgzf_inflate_kernel.hpp) allocates -----------------------------------------------------------------------
def table_alloc(count, root):
    """entries of the two-level table build_table makes for a code with count[l] codes of length l (first level + every
    second-level table, sized the way the kernel sizes them)"""
    mx = 15
    while mx >= 1 and not count[mx]:
        mx -= 1
    first = 1 << root
    nf, code, cur = first, 0, None
    for ln in range(1, mx + 1):
        cnt = count[ln]
        for c in range(cnt):
            if ln > root:
                pre = _rev(code, ln) & (first - 1)
                if pre != cur:
                    curr, left, ll = ln - root, (1 << (ln - root)) - (cnt - c), ln
                    while left > 0 and ll < mx:
                        ll += 1
                        curr += 1
                        left = (left << 1) - count[ll]
                    nf += 1 << curr
                    cur = pre
            code += 1
        code <<= 1
    return nf


def lens_alloc(lens, root):
    count = [0] * 16
    for n in lens:
        count[n] += 1
    count[0] = 0
    return table_alloc(count, root)


def max_table_counts(kind, seed=1, iters=2500):
    """hill climb over complete count vectors (at most 286 lit/len or 30 distance codes): codes whose tables need as many entries
    as the decoders reserve for them (`enough 286 10 15` = 1332, `enough 30 8 15` = 400)"""
    nsym, root = (286, LIT_ROOT) if kind == "lit" else (30, DIST_ROOT)
    rng = random.Random(seed)
    c, n = [0] * 16, 2
    c[1] = 2
    while n < nsym:
        ln = max(k for k in range(1, 15) if c[k])
        c[ln] -= 1
        c[ln + 1] += 2
        n += 1
    best, cur = table_alloc(c, root), c
    for _ in range(iters):
        x = cur[:]
        for _ in range(rng.randint(1, 3)):
            ln = rng.randint(1, 14)
            if rng.random() < 0.5:
                if x[ln] and sum(x) < nsym:
                    x[ln] -= 1
                    x[ln + 1] += 2
            elif x[ln + 1] >= 2:
                x[ln + 1] -= 2
                x[ln] += 1
        if sum(x) >= 2:
            v = table_alloc(x, root)
            if v >= best:
                best, cur = v, x
    return cur, best


_MAX_COUNTS = {}


def max_table_code(kind, used, nsym):
    """lengths (nsym symbols) with the hill climb's count vector; the longest codes go to the symbols in `used` (in order), so
    that decoding runs through the second-level tables"""
    if kind not in _MAX_COUNTS:
        _MAX_COUNTS[kind] = max_table_counts(kind)
    count = _MAX_COUNTS[kind][0]
    by_len = [ln for ln in range(15, 0, -1) for _ in range(count[ln])]
    assert len(by_len) <= nsym
    order = list(used) + [s for s in range(nsym) if s not in set(used)]
    lens = [0] * nsym
    for s, ln in zip(order, by_len):
        lens[s] = ln
    assert kraft(lens) == 1 << 15
    return lens


def long_codes_on_used_symbols(used, nsym, lo=13, hi=15, longest=(284, 29)):
    """used symbols get codes of lo..hi bits (the symbols in `longest`: hi), the unused ones take the rest of the Kraft sum with
    short codes"""
    fixed = {s: hi if s in longest else lo + (i % (hi - lo + 1)) for i, s in enumerate(sorted(used))}
    return complete_code(nsym, fixed, [s for s in range(nsym) if s not in fixed])


def single_distance_code(dsym):
    lens = [0] * (dsym + 1)
    lens[dsym] = 1
    return lens


def no_distance_codes():
    return [0]


# ---- code-length (precode) encoding ---------------------------------------------------------------------------------------------
def rle_lengths(lens, hlit, use16=True, use17=True, use18=True, cross=True):
    """RFC 1951 3.2.7 run-length items [(symbol, extra)]; cross=False: no run spans the literal/length | distance border"""
    parts = [lens] if cross else [lens[:hlit], lens[hlit:]]
    items = []
    for part in parts:
        i = 0
        while i < len(part):
            v, j = part[i], i
            while j < len(part) and part[j] == v:
                j += 1
            run = j - i
            if v == 0 and (use17 or use18):
                while run >= 3:
                    if use18 and run >= 11:
                        k = min(run, 138)
                        items.append((18, k - 11))
                    elif use17:
                        k = min(run, 10)
                        items.append((17, k - 3))
                    else:
                        break
                    run -= k
                items += [(0, None)] * run
            else:
                items.append((v, None))
                run -= 1
                while use16 and run >= 3:
                    k = min(run, 6)
                    items.append((16, k - 3))
                    run -= k
                items += [(v, None)] * run
            i = j
    return items


_CL_EXTRA = {16: 2, 17: 3, 18: 7}


def write_dynamic_header(w, last, litlens, distlens, hlit=None, hdist=None, hclen=None, items=None, cross=True, use16=True, use17=True,
                         use18=True, cl_lens=None):
    hlit = len(litlens) if hlit is None else hlit
    hdist = len(distlens) if hdist is None else hdist
    if items is None:
        items = rle_lengths(list(litlens) + list(distlens), hlit, use16, use17, use18, cross)
    if cl_lens is None:
        f = [0] * 19
        for s, _ in items:
            f[s] += 1
        cl_lens = huffman_lengths(f, 7)
    if hclen is None:
        hclen = 19
        while hclen > 4 and cl_lens[CL_ORDER[hclen - 1]] == 0:
            hclen -= 1
    w.put(last, 1)
    w.put(2, 2)
    w.put(hlit - 257, 5)
    w.put(hdist - 1, 5)
    w.put(hclen - 4, 4)
    for k in range(hclen):
        w.put(cl_lens[CL_ORDER[k]], 3)
    cc = canonical(cl_lens)
    for s, x in items:
        w.put(*cc[s])
        if s >= 16:
            w.put(x, _CL_EXTRA[s])


def write_tokens(w, tokens, litlens, distlens):
    lc, dc = canonical(litlens), canonical(distlens)
    lit_word = [lc[b] for b in range(256)]
    for t in tokens:
        if t.__class__ is int:
            w.put(*lit_word[t])
            continue
        ln, d = t[0], t[1]
        if len(t) > 2:
            ls, lx = t[2], t[3]
            le = LEN_EXTRA[ls - 257]
        else:
            ls, le, lx = _LEN_TAB[ln]
        ds, de, dx = _DIST_TAB[d]
        c1, n1 = lc[ls]
        c2, n2 = dc[ds]
        w.put(c1 | (lx << n1) | (c2 << (n1 + le)) | (dx << (n1 + le + n2)), n1 + le + n2 + de)
    w.put(*lc[256])


def used_symbols(tokens):
    fl, fd = [0] * 286, [0] * 30
    for t in tokens:
        if t.__class__ is int:
            fl[t] += 1
        else:
            fl[t[2] if len(t) > 2 else _LEN_TAB[t[0]][0]] += 1
            fd[_DIST_TAB[t[1]][0]] += 1
    fl[256] += 1
    return fl, fd


# ---- streams --------------------------------------------------------------------------------------------------------------------
class Builder:
    """data + tokens; `cut()` closes a block.  A block: ("dyn", tokens, shape), ("fixed", tokens), ("stored", bytes) or ("raw", fn)
    for hand-written bits.  shape: a dict of code choices (see `_dyn_codes`)."""

    def __init__(self, seed=0, window=32768):
        self.data = bytearray()
        self.tokens = []
        self.blocks = []
        self.record_starts = []
        self.window = window
        self.rng = random.Random(seed)
        self._hash = {}

    # -- bytes in --
    def literals(self, b):
        self.tokens += list(b)
        self.data += b

    def copy(self, d, n, force=None):
        """a match <n, d>; force = (length symbol, extra value) writes it with that code (e.g. 258 as (284, 31))"""
        assert 1 <= d <= min(len(self.data), 32768) and 3 <= n <= 258, (d, n, len(self.data))
        if force is not None:
            ls, lx = force
            assert LEN_BASE[ls - 257] + lx == n and lx < (1 << LEN_EXTRA[ls - 257]) or (ls, lx) == (284, 31) and n == 258
            self.tokens.append((n, d, ls, lx))
        else:
            self.tokens.append((n, d))
        src = len(self.data) - d
        if d >= n:
            self.data += self.data[src:src + n]
        else:
            for k in range(n):
                self.data.append(self.data[src + k])

    def text(self, b, max_dist=32768):
        """greedy LZ77 (3-byte hash, the latest position only)"""
        h, data, base = self._hash, self.data, len(self.data)
        data += b
        i, end = base, len(data)
        toks = self.tokens
        while i < end:
            if i + 3 <= end:
                key = bytes(data[i:i + 3])
                p = h.get(key)
                h[key] = i
                if p is not None and i - p <= max_dist:
                    n = 3
                    lim = min(258, end - i)
                    while n < lim and data[p + n] == data[i + n]:
                        n += 1
                    toks.append((n, i - p))
                    i += n
                    continue
            toks.append(data[i])
            i += 1

    def record(self, n_seq, literal=False):
        """one FASTQ record (sequence and quality of n_seq bytes)"""
        r = self.rng
        name = b"@c%d" % len(self.record_starts)
        seq = bytes(r.choice(b"ACGTN") if r.random() < 0.97 else 78 for _ in range(n_seq))
        qual = bytes(r.choice(b"FFFF:,#") for _ in range(n_seq))
        self.record_starts.append(len(self.data))
        rec = name + b"\n" + seq + b"\n+\n" + qual + b"\n"
        (self.literals if literal else self.text)(rec)

    def records(self, nbytes, literal=False, lo=20, hi=300):
        stop = len(self.data) + nbytes
        while len(self.data) < stop:
            self.record(self.rng.randint(lo, hi), literal)

    def far_record_copy(self, d, pieces=None, force258=False):
        """a filler record so that a record starts exactly d bytes back, then that record again as matches of distance d (pieces of
        the given lengths; the rest literals).  force258: pieces of 258 written as 284 + 31."""
        pos = len(self.data)
        cands = [s for s in self.record_starts[:-1] if pos + 14 <= s + d <= pos + 4000]
        assert cands, (d, pos)
        s = cands[0]
        fill = s + d - pos                      # bytes of filler record: "@f" + digits + "\n" + seq + "\n+\n" + qual + "\n"
        head = b"@f"
        while (fill - len(head) - 5) % 2:
            head += b"x"
        n = (fill - len(head) - 5) // 2
        self.record_starts.append(pos)
        self.literals(head + b"\n" + b"A" * n + b"\n+\n" + b"F" * n + b"\n")
        assert len(self.data) - s == d
        end = self.record_starts[self.record_starts.index(s) + 1]
        rec_len = end - s
        self.record_starts.append(len(self.data))
        k = 0
        pieces = list(pieces or [])
        while k < rec_len:
            n = pieces.pop(0) if pieces else self.rng.choice([3, 4, 10, 57, 130, 227, 255, 257, 258])
            n = min(n, rec_len - k)
            if n < 3:
                self.literals(bytes(self.data[len(self.data) - d:len(self.data) - d + n]))
            elif n == 258 and force258:
                self.copy(d, 258, (284, 31))
            else:
                self.copy(d, n)
            k += n

    def runs(self, n):
        """a record made of overlapping copies: distance 1, 2 and 3 in the sequence (n bytes each), distance 1 in the quality"""
        self.record_starts.append(len(self.data))
        self.literals(b"@runs\n")
        for d in (1, 2, 3):
            self.literals(b"TAC"[:d])
            self.copy(d, n)
        self.literals(b"\n+\nF")
        left = 3 * n + 5
        while left:
            k = min(left, 258) if left - min(left, 258) != 1 and left - min(left, 258) != 2 else left - 3
            self.copy(1, k)
            left -= k
        self.literals(b"\n")

    # -- blocks --
    def cut(self, kind="dyn", **shape):
        if kind == "stored":
            raise ValueError("use stored()")
        self.blocks.append((kind, self.tokens, shape))
        self.tokens = []

    def stored(self, b):
        assert not self.tokens, "cut() the open block first"
        self.blocks.append(("stored", bytes(b), None))
        self.data += b

    def raw_block(self, fn):
        """a block written by fn(bitwriter, last) (no bytes of output of its own)"""
        assert not self.tokens
        self.blocks.append(("raw", fn, None))

    def deflate(self, final=True):
        """the raw stream; final=False: no block has BFINAL set (a stream that goes on behind these bytes)"""
        if self.tokens:
            self.cut()
        if not self.blocks:
            self.blocks.append(("fixed", [], {}))
        w = BitWriter()
        self.block_bits, self.block_out, out = [], [], 0      # where every block starts: bit of the stream, byte of the output
        for i, (kind, body, shape) in enumerate(self.blocks):
            last = int(final and i == len(self.blocks) - 1)
            self.block_bits.append(w.bitpos)
            self.block_out.append(out)
            if kind == "stored":
                out += len(body)
            elif kind != "raw":
                out += sum(1 if t.__class__ is int else t[0] for t in body)
            if kind == "stored":
                write_stored(w, last, body)
            elif kind == "fixed":
                w.put(last, 1)
                w.put(1, 2)
                write_tokens(w, body, FIXED_LIT, FIXED_DIST)
            elif kind == "raw":
                body(w, last)
            else:
                litlens, distlens, hdr = _dyn_codes(body, shape)
                write_dynamic_header(w, last, litlens, distlens, **hdr)
                write_tokens(w, body, litlens, distlens)
        w.align()
        return w.getvalue()


def write_stored(w, last, b, nlen=None):
    assert len(b) <= 65535
    w.put(last, 1)
    w.put(0, 2)
    w.align()
    w.put(len(b), 16)
    w.put((~len(b) & 0xFFFF) if nlen is None else nlen, 16)
    for x in b:
        w.put(x, 8)


def _dyn_codes(tokens, shape):
    """shape keys: lit = "huffman" | "long" | "max" | list of lengths; dist = "huffman" | "long" | "max" | "single" | "none" | list;
    hlit / hdist = "min" | "full" (286 / 30) | number; and the precode's hclen / cross / use16 / use17 / use18"""
    fl, fd = used_symbols(tokens)
    ul = [s for s in range(286) if fl[s]]
    ud = [s for s in range(30) if fd[s]]
    lit = shape.get("lit", "huffman")
    if lit == "huffman":
        litlens = huffman_lengths(fl, 15)
    elif lit == "long":
        litlens = long_codes_on_used_symbols(ul, 286)
    elif lit == "max":
        litlens = max_table_code("lit", sorted(ul, key=lambda s: -fl[s]), 286)
    else:
        litlens = list(lit)
    dist = shape.get("dist", "huffman")
    if dist == "huffman":
        distlens = huffman_lengths(fd, 15)
    elif dist == "long":
        distlens = long_codes_on_used_symbols(ud, 30)
    elif dist == "max":
        distlens = max_table_code("dist", sorted(ud, key=lambda s: -fd[s]), 30)
    elif dist == "single":
        assert len(ud) == 1, ud
        distlens = single_distance_code(ud[0])
    elif dist == "none":
        assert not ud
        distlens = no_distance_codes()
    else:
        distlens = list(dist)
    litlens, distlens = _trim(litlens, shape.get("hlit", "min"), 257, 286), _trim(distlens, shape.get("hdist", "min"), 1, 30)
    hdr = {k: shape[k] for k in ("hclen", "cross", "use16", "use17", "use18") if k in shape}
    return litlens, distlens, hdr


def _trim(lens, how, lo, hi):
    lens = list(lens) + [0] * (hi - len(lens))
    if how == "full":
        n = hi
    elif how == "min":
        n = max(lo, max([i + 1 for i, v in enumerate(lens) if v], default=lo))
    else:
        n = how
    assert all(v == 0 for v in lens[n:])
    return lens[:n]


# ---- wrappers -------------------------------------------------------------------------------------------------------------------
def gzip_member(raw, data, crc=None, isize=None):
    return (b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + raw +
            struct.pack("<II", (zlib.crc32(data) if crc is None else crc) & 0xFFFFFFFF, (len(data) if isize is None else isize) & 0xFFFFFFFF))


def bgzf_member(raw, data, crc=None, isize=None):
    bsize = 18 + len(raw) + 8
    assert bsize <= 65536, bsize
    hdr = b"\x1f\x8b\x08\x04" + b"\x00\x00\x00\x00" + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize - 1)
    return hdr + raw + struct.pack("<II", (zlib.crc32(data) if crc is None else crc) & 0xFFFFFFFF,
                                   (len(data) if isize is None else isize) & 0xFFFFFFFF)


def lenient_inflate(raw, history=b"", zeros=False):
    """inflate `raw` (a valid stream apart from distances too far back) the way a decoder without the distance check would:
    references before the start read `history` (the previous member's bytes) or zeros (zlib's INFLATE_ALLOW_INVALID_DISTANCE_TOOFAR_ARRR)"""
    pre = bytes(32768) if zeros else bytes(max(0, 32768 - len(history))) + history[-32768:]
    d = zlib.decompressobj(-15, zdict=pre)
    return d.decompress(raw) + d.flush()


# ---- the corpus -----------------------------------------------------------------------------------------------------------------
def _fastq_filler(b, nbytes, literal=False):
    b.records(nbytes, literal=literal)


def valid_case(name, size, seed, head=b""):
    """a Builder for one valid shape, about `size` bytes of FASTQ content (behind `head`, as literals), blocks of 16 - 40 KiB of output"""
    b = Builder(seed)
    if head:
        b.record_starts.append(0)
        b.literals(head)
    r = b.rng
    lead = min(34_000, size * 2 // 3)                                             # history in front of the far copies
    blk = lambda: min(r.randint(16_000, 40_000), max(3_000, size - len(b.data)))   # noqa: E731
    far = lambda lo=24577: r.randint(min(lo, len(b.data) - 1000), min(32768, len(b.data) - 1000))        # noqa: E731
    cl = lambda d: min(d, len(b.data) - 1000)                                        # noqa: E731  (small cases: what history allows)
    if name == "far_distances":
        b.records(lead)
        while len(b.data) < size:
            for d in (32768, 32767, 32507, 32600, r.randint(32507, 32768)):
                b.far_record_copy(cl(d))
                b.records(r.randint(200, 2000))
                if len(b.data) >= size:
                    break
            if len(b.data) % 3 == 0:
                b.runs(r.randint(3, 258))
            b.cut()
    elif name == "len284_31":
        b.records(lead)
        while len(b.data) < size:
            for d in (32768, 24577, r.randint(1_000, 32_768)):
                b.far_record_copy(cl(d), pieces=[258, 258, 258], force258=r.random() < 0.8)
                b.records(r.randint(100, 1500))
                if len(b.data) >= size:
                    break
            b.cut()
    elif name == "long_codes":
        # 15-bit codes on the symbols in use, length code 284 (5 extra) with distance code 29 (13 extra): 48 bits per pair
        b.records(lead, literal=True)
        b.cut(lit="long", dist="none")
        while len(b.data) < size:
            b.far_record_copy(far(), pieces=[r.randint(227, 257)] * 3)
            b.records(r.randint(200, 3000), literal=True)
            if len(b.data) % 4 == 0:
                b.cut(lit="long", dist="long", hlit="full", hdist="full")
            elif len(b.data) % 4 == 1:
                b.cut(lit="long", dist="long")
    elif name == "single_distance":
        b.records(lead, literal=True)
        b.cut(dist="none")
        while len(b.data) < size:
            b.records(r.randint(2_000, 9_000), literal=True)
            b.far_record_copy(cl(32768))
            b.far_record_copy(far())
            b.cut(dist="single")
            b.literals(b"@run\n")
            b.copy(1, r.randint(3, 258))
            b.literals(b"\n+\n")
            b.copy(1, 100)
            b.literals(b"\n")
            b.records(r.randint(500, 3_000), literal=True)
            b.cut(dist="single", hdist=1)
    elif name == "no_distance":
        while len(b.data) < size:
            b.records(blk(), literal=True)
            b.cut(dist="none", hdist=r.choice([1, 30]))
    elif name == "crossing_runs":
        b.records(lead)
        b.cut(hlit="full", hdist="full", cross=True)
        k = 0
        while len(b.data) < size:
            if k % 2 == 0:
                b.records(blk() // 2)
            else:
                b.records(blk() // 2, literal=True)
                b.far_record_copy(far(), pieces=[100] * 8)
            fl, fd = used_symbols(b.tokens)
            ul = [s for s in range(286) if fl[s]]
            ud = [s for s in range(30) if fd[s]]
            # a 16 run from the literal/length lengths into the distance ones, or a run of zeros (17 / 18) across the border
            if k % 2 == 0:
                distlens = huffman_lengths(fd, 15)
                v = distlens[0]
                fixed_l = {s: 10 for s in ul if s < 281}
                fixed_l.update({s: v for s in range(281, 286) if v})
                litlens = complete_code(286, fixed_l, [s for s in range(256) if s not in fixed_l])
                b.cut(lit=litlens, dist=distlens, hlit="full", hdist="full", cross=True, hclen=19)
            else:
                b.cut(hlit="full", hdist="full", cross=True, use16=False)
            k += 1
    elif name == "max_tables":
        b.records(lead)
        while len(b.data) < size:
            b.records(blk())
            if r.random() < 0.5:
                b.far_record_copy(far())
            b.cut(lit="max", dist="max", hlit="full", hdist="full")
    elif name == "sync_flush":
        # pigz-style: an empty stored block every few KiB, and stored blocks at odd bit positions between dynamic / fixed ones
        while len(b.data) < size:
            b.records(r.randint(2_000, 9_000))
            b.cut(kind=r.choice(["dyn", "dyn", "fixed"]))
            b.stored(b"")
            if r.random() < 0.3:
                b.records(r.randint(50, 400), literal=True)
                piece = bytes(b.data[-r.randint(1, 300):])
                b.cut()
                b.stored(piece)
    elif name == "header_edges":
        # HCLEN 19 with trailing zero lengths, HLIT 257 (no matches) / 286, HDIST 1 / 30
        while len(b.data) < size:
            b.records(r.randint(3_000, 9_000), literal=True)
            b.cut(dist="none", hlit=257, hdist=1, hclen=19)
            b.records(r.randint(3_000, 9_000))
            b.cut(hlit="full", hdist="full", hclen=19)
            b.records(r.randint(3_000, 9_000), literal=True)
            b.cut(kind="fixed")
    elif name == "eob_only":
        # blocks of nothing but end-of-block: an incomplete lit/len code of one 1-bit code, between ordinary dynamic blocks
        while len(b.data) < size:
            b.records(r.randint(3_000, 9_000))
            b.cut()
            b.cut(lit=[0] * 256 + [1], dist="none")
    else:
        raise KeyError(name)
    if b.tokens or not b.blocks:
        b.cut()
    return b


def far_model_case(seed):
    """small enough for the Python loop models: 34 KB of history in one stored block, then dynamic blocks with copies of distance
    32 768 / 32 767 / 32 507, 258 as 284 + 31, and 48-bit pairs (15-bit codes for length code 284 and distance code 29)"""
    h = Builder(seed)
    h.records(34_000, literal=True)
    b = Builder(seed)
    b.record_starts = list(h.record_starts)
    b.stored(bytes(h.data))
    for d in (32768, 32767, 32507):
        b.far_record_copy(d, pieces=[258, 258], force258=True)
    b.cut(dist="single")
    b.far_record_copy(b.rng.randint(24577, 32768), pieces=[240] * 3)
    b.records(1_500, literal=True)
    b.cut(lit="long", dist="long", hlit="full", hdist="full")
    return b


def member_case(name, seed, limit=65536):
    """a valid shape that fits one BGZF member: at most 64 KiB of output, BSIZE <= 65536"""
    size = 60_000
    while True:
        b = valid_case(name, size, seed)
        b.raw = b.deflate()
        if len(b.data) <= limit and 26 + len(b.raw) <= 65536:
            return b
        size -= 4_000


VALID = ["far_distances", "len284_31", "long_codes", "single_distance", "no_distance", "crossing_runs", "max_tables", "sync_flush",
         "header_edges", "eob_only"]
# shapes that the device search accepts as block starts (gz_inflate_kernels.hpp: sync_deep_tab): all but the one-code lit/len block
SEARCH_REJECTS = {"eob_only"}


def crossing_runs(items, hlit):
    """run-length items (16 / 17 / 18) that cover lengths on both sides of the literal/length | distance border"""
    k, out = 0, []
    for s, x in items:
        rep = 1 if s < 16 else {16: 3, 17: 3, 18: 11}[s] + x
        if s >= 16 and k < hlit < k + rep:
            out.append(s)
        k += rep
    return out


def _junk_tokens(rng, n):
    return [rng.randrange(256) for _ in range(n)]


def invalid_cases(seed=5):
    """{name: raw deflate} of streams that zlib rejects; each starts with a few KiB of valid data"""
    rng = random.Random(seed)
    out = {}

    def with_prefix(fn):
        b = Builder(seed)
        b.records(3_000)
        b.cut()
        b.raw_block(fn)
        return b.deflate()

    toks = _junk_tokens(rng, 300) + [(10, 5), (258, 100), (30, 2)]
    fl, fd = used_symbols(toks)
    good_l, good_d = huffman_lengths(fl, 15), huffman_lengths(fd, 15)

    def dyn(litlens, distlens, tokens=toks, **hdr):
        def fn(w, last):
            write_dynamic_header(w, last, litlens, distlens, **hdr)
            write_tokens(w, tokens, litlens, distlens)
            w.put(0, 64)
        return fn

    over_l = list(good_l)
    over_l[next(s for s in range(286) if not fl[s])] = 1
    out["oversubscribed_litlen"] = with_prefix(dyn(over_l, good_d))
    over_d = list(good_d) + [0] * (30 - len(good_d))
    for s in range(30):
        if not fd[s]:
            over_d[s] = 1
            break
    out["oversubscribed_dist"] = with_prefix(dyn(good_l, over_d))
    inc_l = long_codes_on_used_symbols([s for s in range(286) if fl[s]], 286)
    inc_l[next(s for s in range(256) if inc_l[s] and not fl[s])] = 0
    out["incomplete_litlen"] = with_prefix(dyn(inc_l, good_d))
    no_eob = complete_code(286, {s: 12 for s in range(286) if fl[s] and s != 256}, [s for s in range(286) if not fl[s] and s != 256])
    out["no_end_of_block_code"] = with_prefix(dyn(no_eob, good_d, tokens=[]))
    items = rle_lengths(good_l + good_d, len(good_l))
    out["repeat16_first"] = with_prefix(dyn(good_l, good_d, items=[(16, 1)] + items))
    out["repeats_overrun"] = with_prefix(dyn(good_l, good_d, items=items[:-1] + [(18, 127)]))
    out["hlit_287"] = with_prefix(dyn(good_l + [0], good_d, hlit=287))
    out["hdist_31"] = with_prefix(dyn(good_l, list(good_d) + [0] * (31 - len(good_d)), hdist=31))

    def fixed_sym(lsym, dsym=None):
        def fn(w, last):
            w.put(last, 1)
            w.put(1, 2)
            c = canonical(FIXED_LIT)
            for t in _junk_tokens(rng, 50):
                w.put(*c[t])
            w.put(*c[lsym])
            if dsym is not None:
                w.put(*canonical(FIXED_DIST)[dsym])
            w.put(0, 64)
        return fn

    out["litlen_286_in_data"] = with_prefix(fixed_sym(286))
    out["litlen_287_in_data"] = with_prefix(fixed_sym(287))
    out["dist_30_in_data"] = with_prefix(fixed_sym(257, 30))
    out["dist_31_in_data"] = with_prefix(fixed_sym(257, 31))

    def missing_single(w, last):
        one = single_distance_code(4)            # code '0' for distance code 4; the other 1-bit code ('1') is missing
        write_dynamic_header(w, last, good_l, one)
        lc = canonical(good_l)
        for t in [t for t in toks if t.__class__ is int][:40]:
            w.put(*lc[t])
        w.put(*lc[_LEN_TAB[10][0]])
        w.put(1, 1)
        w.put(0, 64)
    out["missing_single_distance_code"] = with_prefix(missing_single)

    def type3(w, last):
        w.put(last, 1)
        w.put(3, 2)
        w.put(0, 64)
    out["block_type_3"] = with_prefix(type3)
    out["stored_bad_nlen"] = with_prefix(lambda w, last: (write_stored(w, last, b"hello, world", nlen=0x1234), w.put(0, 64)))
    return out


def zlib_inflate(raw):
    d = zlib.decompressobj(-15)
    out = d.decompress(raw) + d.flush()
    if not d.eof:
        raise zlib.error("incomplete stream")
    return out

"""Plain-Python / numpy checker of `sc fa-gc`, written from the definitions of the command (include/sc_fqcount.h):

  a header line is a line whose first byte is '>'; a base is a byte 0x21 .. 0x7E on any other line; a contig starts at a header
  line, its name is the text after '>' up to the first byte <= 0x20, its bases are those up to the next header line; gc is
  G C g c, acgt is A C G T a c g t.

It shares no code with the product.  FaModel holds the per-base class arrays of one input and their prefix sums."""
import gzip
import math
import re

import numpy as np

GC = np.zeros(256, dtype=bool)
GC[list(b"GCgc")] = True
ACGT = np.zeros(256, dtype=bool)
ACGT[list(b"ACGTacgt")] = True
BASE = np.zeros(256, dtype=bool)
BASE[0x21:0x7F] = True

# scripts/functional-tests.sh:73-80 of the reference: (position, window text, cell text), and the counts behind them
PINS = (("chr1:1", "1", "0.5", (1, 2)), ("chr1:10", "100000", "0.495", (495, 1000)), ("chr3:10", "100000", "0.513", (513, 1000)))


class FaModel:
    def __init__(self, data):
        a = np.frombuffer(bytes(data), dtype=np.uint8)
        self.n = a.size
        # line starts: byte 0 and every byte behind a '\n'
        nl = np.flatnonzero(a == 10)
        starts = np.concatenate(([0], nl + 1)) if a.size else np.zeros(0, dtype=np.int64)
        starts = starts[starts < a.size]
        is_hdr_line = a[starts] == ord(">") if starts.size else np.zeros(0, dtype=bool)
        # per byte: is its line a header line
        line_of = np.searchsorted(starts, np.arange(a.size), side="right") - 1 if a.size else np.zeros(0, dtype=np.int64)
        in_hdr = is_hdr_line[line_of] if a.size else np.zeros(0, dtype=bool)
        base = BASE[a] & ~in_hdr
        self.base_pos = np.flatnonzero(base)                       # byte offset of every base, in rank order
        seq = a[self.base_pos]
        self.seq = seq.tobytes()
        self.gc_pre = np.concatenate(([0], np.cumsum(GC[seq], dtype=np.int64)))
        self.acgt_pre = np.concatenate(([0], np.cumsum(ACGT[seq], dtype=np.int64)))
        self.bases = int(seq.size)
        self.gc_bases = int(self.gc_pre[-1])
        self.acgt_bases = int(self.acgt_pre[-1])
        self.contigs = []                                          # (name bytes, header offset, rank, length)
        hdr_offsets = starts[is_hdr_line] if starts.size else []
        ranks = np.searchsorted(self.base_pos, hdr_offsets)
        raw = a.tobytes()
        for k, off in enumerate(hdr_offsets):
            m = re.match(rb"[\x21-\xff]*", raw[off + 1:off + 1 + 4096])
            rank = int(ranks[k])
            end = int(ranks[k + 1]) if k + 1 < len(hdr_offsets) else self.bases
            self.contigs.append((m.group(0), int(off), rank, end - rank))
        self.orphan_bases = self.contigs[0][2] if self.contigs else self.bases

    def find(self, name):
        raw = name if isinstance(name, bytes) else name.encode("latin-1")
        for i, c in enumerate(self.contigs):
            if c[0] == raw:
                return i
        return None

    def count(self, contig, begin, end):
        """(gc, acgt, bases) of the bases [begin, end) of a contig"""
        rank, length = self.contigs[contig][2], self.contigs[contig][3]
        assert 0 <= begin <= end <= length
        lo, hi = rank + begin, rank + end
        return int(self.gc_pre[hi] - self.gc_pre[lo]), int(self.acgt_pre[hi] - self.acgt_pre[lo]), end - begin

    def count_many(self, q):
        """q: int array (nq, 3) of contig, begin, end -> int array (nq, 3)"""
        q = np.asarray(q, dtype=np.int64).reshape(-1, 3)
        rank = np.array([c[2] for c in self.contigs], dtype=np.int64)[q[:, 0]] if q.size else np.zeros(0, dtype=np.int64)
        lo, hi = rank + q[:, 1], rank + q[:, 2]
        return np.stack([self.gc_pre[hi] - self.gc_pre[lo], self.acgt_pre[hi] - self.acgt_pre[lo], hi - lo], axis=1)

    def count_slow(self, contig, begin, end):
        """the same by walking the bases one by one: what the reference does per cell"""
        rank = self.contigs[contig][2]
        seq = self.seq[rank + begin:rank + end]
        return sum(c in b"GCgc" for c in seq), sum(c in b"ACGTacgt" for c in seq), len(seq)


def parse_window(text):
    """sci_parse_int and the '>= 1' rule; ValueError for what is no window"""
    if "e" in text:
        co, ex = text.split("e", 1)
        if not re.fullmatch(r"[+-]?[0-9]+", ex):
            raise ValueError(text)
        value = math.pow(float(co) * 10.0, float(int(ex)))
        if not value < 9e18:
            raise ValueError(text)
        value = int(value)
    else:
        digits = text.replace(",", "")
        if not re.fullmatch(r"[+-]?[0-9]+", digits):
            raise ValueError(text)
        value = int(digits)
    if value < 1:
        raise ValueError("Window lengths must be >= 1")
    return value


def gc_interval(pos, window, length):
    """(begin, end), or None when the 1-based pos is out of range"""
    pos0 = pos - 1
    if pos < 1 or pos0 >= length:
        return None
    return max(0, pos0 - window), min(length, pos0 + window + 1)


def c_round(x):
    """C round(): halves away from zero"""
    return math.copysign(math.floor(abs(x) + 0.5), x) if abs(x) < 2 ** 52 else x


def value_text(gc, acgt, window):
    if acgt == 0:
        return "nan"
    digits = len(str(window)) + 2
    scale = math.pow(10.0, digits)
    return repr(c_round(gc / acgt * scale) / scale)


def parse_positions(pos_in):
    """([(chrom, pos)], [warning text]) of one 'chr:pos' string or a positions file"""
    if ":" in pos_in and "/" not in pos_in:
        chrom, pos = pos_in.split(":", 1)
        return [(chrom, int(pos))], []
    opener = gzip.open if pos_in.endswith(".gz") else open
    with opener(pos_in, "rb") as f:
        lines = f.read().decode("latin-1").split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    out, warnings = [], []
    for n, line in enumerate(lines, 1):
        if line.endswith("\r"):
            line = line[:-1]
        fields = re.split(r"[\t: ]+", line.strip("\t: "))
        if len(fields) >= 2 and re.fullmatch(r"[+-]?[0-9]+", fields[1]):
            out.append((fields[0], int(fields[1])))
        elif n != 1 and not line.startswith("#"):
            warnings.append('Invalid line: %d in "%s" > %s' % (n, pos_in, line))
    return out, warnings


def order(positions):
    """stable: all-digit names by value then position; x, y, m by that rank then position; the others by name"""
    def key(p):
        s = p[0].lower()
        if len(s) > 3 and s.startswith("chr"):
            s = s[3:]
        if re.fullmatch("[0-9]*", s):
            return (0, int(s or "0"), b"", p[1])
        if s in ("x", "y", "m"):
            return (1, {"x": 1, "y": 2, "m": 3}[s], b"", p[1])
        return (2, 0, s.encode("latin-1"), 0)
    return sorted(positions, key=key)


def warning_line(msg):
    return "\x1b[33mWarning: %s\x1b[0m\n" % msg


def cli_text(model, positions, windows):
    """(stdout, stderr) of `sc fa-gc` for parsed positions (in input order) and parsed windows"""
    out = ["\t".join(["chrom", "pos"] + ["gc_%d" % (2 * w) for w in windows])]
    err = []
    for chrom, pos in order(positions):
        c = model.find(chrom)
        span = None if c is None else gc_interval(pos, windows[0], model.contigs[c][3])
        if span is None:
            err.append(warning_line("<%s:%d> is out of range" % (chrom, pos)))
            continue
        cells = []
        for w in windows:
            b, e = gc_interval(pos, w, model.contigs[c][3])
            gc, acgt, _ = model.count(c, b, e)
            cells.append(value_text(gc, acgt, w))
        out.append("\t".join([chrom, str(pos)] + cells))
    return "\n".join(out) + "\n", "".join(err)

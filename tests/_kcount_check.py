"""The checker of fq-kcount: the definitions of include/sc_fqcount.h restated in plain Python on top of _kmers_check.kmers_of (a
slice and a dict, any k), summed over one or two inputs, with what the table's readers return (unique, the histogram with its
overflow bin, the dump filters, the top-N order) and the texts of `sc fq-kcount`; and a numpy form (64-bit keys, np.unique) for
inputs too large for a Python loop.  Every comparison is ==."""
import numpy as np

from _kmers_check import CODE, kmers_of, revcomp_index, word_of
from _readstats_check import line_spans_np

SUMMARY_FIELDS = ("struct_size", "abi_version", "reads", "lines", "input_bytes", "k", "flags", "windows", "kmers", "skipped",
                  "short_lines", "distinct", "unique", "max_count", "slots", "passes")
CANONICAL = 1
EARG, EHIP, EFULL = -5, -3, -10
HIST_HEADER = "count\tkmers"
DUMP_HEADER = "kmer\tcount"
TOTALS_HEADER = "k\twindows\tkmers\tskipped\tshort_lines\tdistinct\tunique\tmax_count"


class Want:
    """what one call has to return: the table {key: count} and the sums over the inputs"""

    def __init__(self, table, windows, kmers, skipped, short_lines, lines, reads, input_bytes):
        self.table, self.windows, self.kmers, self.skipped, self.short_lines = table, windows, kmers, skipped, short_lines
        self.lines, self.reads, self.input_bytes = lines, reads, input_bytes

    @property
    def distinct(self):
        return len(self.table)

    @property
    def unique(self):
        return sum(1 for c in self.table.values() if c == 1)

    @property
    def max_count(self):
        return max(self.table.values(), default=0)

    def __eq__(self, other):
        return self.__dict__ == other.__dict__

    def __repr__(self):
        return "Want(%r)" % ({k: v for k, v in self.__dict__.items() if k != "table"},)


def _sum(parts):
    table = {}
    tot = [0] * 7
    for t, windows, kmers, skipped, short, lines, nbytes in parts:
        for key, c in t.items():
            table[key] = table.get(key, 0) + c
        for i, v in enumerate((windows, kmers, skipped, short, lines, (lines + 3) // 4, nbytes)):
            tot[i] += v
    return Want(table, *tot)


def kcount_of(inputs, k, canonical=False):
    """inputs: one bytes object or a list of one or two; the plain form"""
    if isinstance(inputs, (bytes, bytearray)):
        inputs = [inputs]
    return _sum([kmers_of(bytes(d), k, canonical) + (len(d),) for d in inputs])


def _one_np(a, k, canonical):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    starts, tends = line_spans_np(a)
    lines = starts.size
    s, e = starts[1::4], tends[1::4]
    short = int(((e - s) < k).sum())
    per_line = np.maximum(e - s - k + 1, 0)
    windows = int(per_line.sum())
    if windows == 0:
        return {}, 0, 0, 0, short, lines, a.size
    first = np.cumsum(per_line) - per_line
    pos = np.arange(windows, dtype=np.int64) - np.repeat(first, per_line) + np.repeat(s, per_line)      # where each window starts
    lut = np.full(256, 4, np.uint64)
    for byte, code in CODE.items():
        lut[byte] = code
    code = lut[a]
    fw, rc, bad = np.zeros(windows, np.uint64), np.zeros(windows, np.uint64), np.zeros(windows, bool)
    three = np.uint64(3)
    for i in range(k):
        c = code[pos + i]
        isbad = c == 4
        bad |= isbad
        c = np.where(isbad, np.uint64(0), c)
        fw = (fw << np.uint64(2)) | c                  # (k = 32: the first shifts move zeros out)
        rc |= (three - c) << np.uint64(2 * i)
    idx = (np.minimum(fw, rc) if canonical else fw)[~bad]
    skipped = int(bad.sum())
    vals, counts = np.unique(idx, return_counts=True)
    table = {int(v): int(c) for v, c in zip(vals, counts)}
    return table, windows, windows - skipped, skipped, short, lines, a.size


def kcount_of_np(inputs, k, canonical=False):
    """the numpy form; inputs: one uint8 array or a list of one or two"""
    if isinstance(inputs, np.ndarray):
        inputs = [inputs]
    return _sum([_one_np(a, k, canonical) for a in inputs])


def hist_of(table, bins):
    """hist[0] = 0, hist[c] keys with count c for c <= bins - 2, hist[bins - 1] keys with count >= bins - 1"""
    h = [0] * bins
    for c in table.values():
        h[min(c, bins - 1)] += 1
    return h


def dump_of(table, min_count=1, max_count=0):
    """[(key, count)] in ascending key order; max_count = 0: no upper bound"""
    return [(key, c) for key, c in sorted(table.items()) if c >= min_count and (max_count == 0 or c <= max_count)]


def top_of(table, n):
    """the n most frequent: count descending, then key ascending"""
    return sorted(table.items(), key=lambda t: (-t[1], t[0]))[:n]


def canonical_key(key, k):
    return min(key, revcomp_index(key, k))


def rows_text(rows, k, suffix=""):
    return "".join("%s\t%d%s\n" % (word_of(key, k), c, suffix) for key, c in rows)


def hist_text(table, high=10000, suffix=""):
    """stdout of `sc fq-kcount [--high=N]`: jellyfish-histo shaped"""
    mx = max(table.values(), default=0)
    h = hist_of(table, high + 2)
    out = ["%d\t%d%s\n" % (c, h[c], suffix) for c in range(1, min(mx, high) + 1)]
    if h[high + 1]:
        out.append("%d\t%d%s\n" % (high + 1, h[high + 1], suffix))
    return "".join(out)


def totals_text(want, k, suffix=""):
    return "%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d%s\n" % (k, want.windows, want.kmers, want.skipped, want.short_lines, want.distinct, want.unique,
                                                  want.max_count, suffix)


def assert_summary(s, want, k, flags, ctx=""):
    """s: scfq.KcountSummary; every field but the two diagnostics compared with =="""
    head = dict(reads=want.reads, lines=want.lines, input_bytes=want.input_bytes, k=k, flags=flags, windows=want.windows, kmers=want.kmers,
                skipped=want.skipped, short_lines=want.short_lines, distinct=want.distinct, unique=want.unique, max_count=want.max_count)
    for name, v in head.items():
        assert int(getattr(s, name)) == v, (ctx, k, flags, name, int(getattr(s, name)), v)
    assert want.windows == want.kmers + want.skipped and sum(want.table.values()) == want.kmers, ctx
    assert int(s.passes) >= 1 and int(s.slots) >= 1024 and int(s.slots) & (int(s.slots) - 1) == 0, (ctx, int(s.passes), int(s.slots))


def assert_table(t, want, k, flags, ctx="", bins=None):
    """t: scfq.KcountTable; hist at the four sizes, the whole dump, every present key and absent ones through query"""
    table = want.table
    mx = want.max_count
    for b in (bins if bins is not None else sorted({2, max(mx + 1, 2), mx + 2, 10002})):
        got = t.hist(b).tolist()
        assert got == hist_of(table, b), (ctx, k, flags, "hist", b)
        assert got[0] == 0 and sum(got) == len(table), (ctx, b)
    got = [tuple(r) for r in t.dump(1, 0).tolist()]
    if got != dump_of(table):
        diff = sorted(set(got) ^ set(dump_of(table)))[:6]
        raise AssertionError((ctx, k, flags, "dump differs", len(got), len(table), diff))
    keys = sorted(table)
    if flags & CANONICAL:                      # the plain index of either strand finds the canonical entry
        ask = [revcomp_index(v, k) if i % 2 else v for i, v in enumerate(keys)]
    else:
        ask = keys
    full = 4 ** k - 1
    absent = [v for v in (0, 1, full, full - 1, 0x123456789ABCDEF & full, (0x0F1E2D3C4B5A6978 & full)) if
              (canonical_key(v, k) if flags & CANONICAL else v) not in table]
    counts = t.query(np.array(ask + absent, dtype=np.uint64)).tolist()
    assert counts == [table[v] for v in keys] + [0] * len(absent), (ctx, k, flags, "query")

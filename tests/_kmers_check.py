"""The checker of fq-kmers, twice: a plain restatement of the definitions in include/sc_fqcount.h (lines as _readstats_check.py
has them; a window is k consecutive text bytes of one sequence line, a k-mer when all of them are A C G T) with a slice and a
dict, and a numpy form (2-bit codes, one shifted add per base, bincount) for inputs too large for a Python loop.  Both return
(table, windows, kmers, skipped, short_lines, lines); the table is a dict {index: count} of the non-zero entries, or with
dense=True the numpy form's uint64 array of 4^k entries."""
import numpy as np

from _readstats_check import line_spans_np, lines_of

SUMMARY_FIELDS = ("struct_size", "abi_version", "reads", "lines", "input_bytes", "k", "flags", "windows", "kmers", "skipped",
                  "short_lines", "distinct", "max_count", "table_entries")
CANONICAL = 1
CODE = {65: 0, 67: 1, 71: 2, 84: 3}


def index_of(word):
    """index of k letters of ACGT (bytes), first base most significant"""
    v = 0
    for b in word:
        v = 4 * v + CODE[b]
    return v


def revcomp_index(index, k):
    out = 0
    for _ in range(k):
        out = 4 * out + (3 - (index & 3))
        index >>= 2
    return out


def kmers_of(data, k, canonical=False):
    ls = lines_of(bytes(data))
    table = {}
    windows = kmers = skipped = short = 0
    for j in range(1, len(ls), 4):
        s = ls[j]
        if len(s) < k:
            short += 1
        for i in range(len(s) - k + 1):
            w = s[i:i + k]
            windows += 1
            if all(b in CODE for b in w):
                v = index_of(w)
                if canonical:
                    v = min(v, revcomp_index(v, k))
                table[v] = table.get(v, 0) + 1
                kmers += 1
            else:
                skipped += 1
    return table, windows, kmers, skipped, short, len(ls)


def kmers_of_np(a, k, canonical=False, dense=False):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    starts, tends = line_spans_np(a)
    lines = starts.size
    s, e = starts[1::4], tends[1::4]
    short = int(((e - s) < k).sum())
    per_line = np.maximum(e - s - k + 1, 0)
    windows = int(per_line.sum())
    entries = 4 ** k
    if windows == 0:
        return (np.zeros(entries, np.uint64) if dense else {}), 0, 0, 0, short, lines
    first = np.cumsum(per_line) - per_line
    pos = np.arange(windows, dtype=np.int64) - np.repeat(first, per_line) + np.repeat(s, per_line)      # where each window starts
    lut = np.full(256, 4, np.int64)
    for byte, code in CODE.items():
        lut[byte] = code
    code = lut[a]
    fw, rc, bad = np.zeros(windows, np.int64), np.zeros(windows, np.int64), np.zeros(windows, bool)
    for i in range(k):
        c = code[pos + i]
        bad |= c == 4
        fw = 4 * fw + c
        rc += (3 - c) << (2 * i)
    idx = (np.minimum(fw, rc) if canonical else fw)[~bad]
    skipped = int(bad.sum())
    if dense:
        table = np.bincount(idx, minlength=entries).astype(np.uint64)
    elif entries <= 1 << 16:
        full = np.bincount(idx, minlength=entries)
        table = {int(v): int(full[v]) for v in np.flatnonzero(full)}
    else:                                      # (bincount without its 4^k array)
        vals, counts = np.unique(idx, return_counts=True)
        table = {int(v): int(c) for v, c in zip(vals, counts)}
    return table, windows, windows - skipped, skipped, short, lines


def as_dict(table):
    if isinstance(table, dict):
        return table
    nz = np.flatnonzero(table)
    return {int(v): int(table[v]) for v in nz}


def assert_result(got, want, k, flags, input_bytes, ctx=""):
    """got: (scfq.KmerSummary, table or None) of a call; want: a checker's tuple; every field compared with =="""
    s, table = got
    wt, windows, kmers, skipped, short, lines = want
    wd = as_dict(wt)
    head = dict(reads=(lines + 3) // 4, lines=lines, input_bytes=input_bytes, k=k, flags=flags, windows=windows, kmers=kmers, skipped=skipped,
                short_lines=short, distinct=len(wd), max_count=max(wd.values(), default=0), table_entries=4 ** k)
    for name, v in head.items():
        assert int(getattr(s, name)) == v, (ctx, k, flags, name, int(getattr(s, name)), v)
    if table is not None:
        assert table.shape == (4 ** k,), (ctx, table.shape)
        if isinstance(wt, dict):
            gd = as_dict(table)
            if gd != wd:
                diff = sorted(set(gd.items()) ^ set(wd.items()))[:8]
                raise AssertionError((ctx, k, flags, "tables differ", diff))
        elif not np.array_equal(table, wt):
            bad = np.flatnonzero(table != wt)
            raise AssertionError((ctx, k, flags, "tables differ", bad[:8].tolist(), table[bad[:8]].tolist(), wt[bad[:8]].tolist()))


def word_of(index, k):
    return "".join("ACGT"[(index >> (2 * (k - 1 - i))) & 3] for i in range(k))


def cli_text(table, k, suffix="", top=None):
    """stdout of `sc fq-kmers --k=K [--top=N]` for one file"""
    items = sorted(as_dict(table).items())
    if top is not None:
        items = sorted(items, key=lambda t: (-t[1], t[0]))[:top]
    return "".join("%s\t%d%s\n" % (word_of(v, k), c, suffix) for v, c in items)


def totals_text(want, k, suffix=""):
    """stdout of `sc fq-kmers --totals` for one file"""
    wt, windows, kmers, skipped, short, _ = want
    wd = as_dict(wt)
    return "%d\t%d\t%d\t%d\t%d\t%d\t%d%s\n" % (k, windows, kmers, skipped, short, len(wd), max(wd.values(), default=0), suffix)

"""The checker of fq-cycles: a plain restatement of the definitions in include/sc_fqcount.h (lines and records as
_readstats_check.py has them; every text byte of a sequence or quality line counts at its 0-based position in the line), a
numpy form of it for inputs too large for a Python loop, and rows / tail / total for a given cap."""
import numpy as np

from _readstats_check import line_spans_np, lines_of

ROW_FIELDS = ("bases", "a", "c", "g", "t", "n", "quals", "qual_sum")
LETTERS = b"ACGTN"


def table_of(data):
    """(table as an int64 array of shape (longest line, 8), lines, max_seq_len, max_qual_len), byte by byte"""
    ls = lines_of(bytes(data))
    seq = [ls[j] for j in range(1, len(ls), 4)]
    qual = [ls[j] for j in range(3, len(ls), 4)]
    ms, mq = max([len(s) for s in seq] or [0]), max([len(q) for q in qual] or [0])
    rows = [[0] * 8 for _ in range(max(ms, mq))]
    for s in seq:
        for p, b in enumerate(s):
            rows[p][0] += 1
            k = LETTERS.find(bytes([b]))
            if k >= 0:
                rows[p][1 + k] += 1
    for q in qual:
        for p, b in enumerate(q):
            rows[p][6] += 1
            rows[p][7] += b
    return np.array(rows, dtype=np.int64).reshape(-1, 8), len(ls), ms, mq


def table_of_np(a):
    """table_of for a uint8 array: position = byte index - start of its line, counted with bincount"""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    starts, tends = line_spans_np(a)
    lines = starts.size

    def positions(phase):
        s, e = starts[phase::4], tends[phase::4]
        lens = e - s
        total = int(lens.sum())
        longest = int(lens.max()) if lens.size else 0
        if total == 0:
            return np.zeros(0, np.int64), np.zeros(0, np.int64), longest
        first = np.cumsum(lens) - lens                        # where each line's bytes begin in the concatenation
        pos = np.arange(total, dtype=np.int64) - np.repeat(first, lens)
        return pos, np.repeat(s, lens) + pos, longest

    sp, si, ms = positions(1)
    qp, qi, mq = positions(3)
    top = max(ms, mq)
    out = np.zeros((top, 8), np.int64)
    if sp.size:
        sb = a[si]
        out[:, 0] = np.bincount(sp, minlength=top)
        for k, letter in enumerate(LETTERS):
            out[:, 1 + k] = np.bincount(sp[sb == letter], minlength=top)
    if qp.size:
        out[:, 6] = np.bincount(qp, minlength=top)
        out[:, 7] = np.bincount(qp, weights=a[qi].astype(np.float64), minlength=top).astype(np.int64)      # sums < 2^53: exact
    return out, lines, ms, mq


def split(table, cap):
    """(rows, tail, total) the library owes for `cap`"""
    rows = table[:cap]
    return rows, [int(v) for v in table[cap:].sum(axis=0)], [int(v) for v in table.sum(axis=0)]


def row_ints(r):
    return [int(getattr(r, f)) for f in ROW_FIELDS]


def assert_result(got, table, lines, ms, mq, input_bytes, cap, ctx=""):
    """got: (scfq.CycleSummary, rows) of a call with `cap`; every field compared with =="""
    s, rows = got
    want_rows, tail, total = split(table, cap)
    head = dict(reads=(lines + 3) // 4, lines=lines, input_bytes=input_bytes, max_seq_len=ms, max_qual_len=mq, cycles=min(cap, max(ms, mq)))
    for name, v in head.items():
        assert int(getattr(s, name)) == v, (ctx, cap, name, int(getattr(s, name)), v)
    assert row_ints(s.tail) == tail, (ctx, cap, "tail", row_ints(s.tail), tail)
    assert row_ints(s.total) == total, (ctx, cap, "total", row_ints(s.total), total)
    assert rows.shape == want_rows.shape, (ctx, cap, rows.shape, want_rows.shape)
    if not np.array_equal(rows, want_rows):
        bad = np.flatnonzero((rows != want_rows).any(axis=1))
        raise AssertionError((ctx, cap, "rows differ", bad[:8].tolist(), rows[bad[:4]].tolist(), want_rows[bad[:4]].tolist()))


def mean_text(num, den):
    """the `$float` rule of scfq_format_tsv: "%.16g", ".0" when bare, nan"""
    if den == 0:
        return "nan" if num == 0 else "inf"
    t = "%.16g" % (num / den)
    return t if any(ch in t for ch in ".einf") else t + ".0"


def row_text(r):
    r = [int(v) for v in r]
    return "\t".join([str(v) for v in r[:6]] + [str(r[0] - sum(r[1:6])), str(r[6]), mean_text(r[7], r[6])])


def cli_text(table, max_cycles, suffix=""):
    """stdout of `sc fq-cycles --max-cycles=N` for one file"""
    rows, tail, _ = split(table, max_cycles)
    out = ["%d\t%s%s\n" % (p + 1, row_text(r), suffix) for p, r in enumerate(rows)]
    if tail[0] or tail[6]:
        out.append(">%d\t%s%s\n" % (max_cycles, row_text(tail), suffix))
    return "".join(out)

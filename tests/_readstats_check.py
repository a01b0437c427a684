"""The checker of fq-readstats: a plain restatement of the definitions in include/sc_fqcount.h (lines as the reference's
`lines(stream)` yields them, record i = lines 4i .. 4i+3, a missing line is empty), a numpy form of it for inputs too large
for a Python loop, and the summary computed from the per-read rows with Python integers."""
import numpy as np

REC_FIELDS = ("seq_len", "gc_bases", "n_bases", "qual_len", "qual_sum")


def lines_of(data):
    parts = data.split(b"\n")
    tail = parts.pop()                      # text behind the last real '\n'
    out = [p[:-1] if p.endswith(b"\r") else p for p in parts]
    if tail:
        out.append(tail)                    # keeps a trailing '\r'
    return out


def per_read(data):
    ls = lines_of(bytes(data))
    rows = []
    for i in range((len(ls) + 3) // 4):
        s = ls[4 * i + 1] if 4 * i + 1 < len(ls) else b""
        q = ls[4 * i + 3] if 4 * i + 3 < len(ls) else b""
        rows.append((len(s), s.count(b"G") + s.count(b"C"), s.count(b"N"), len(q), sum(q)))
    return rows


def line_spans_np(a):
    """(start, text_end) of every line of the uint8 array a, as int64 arrays"""
    n = a.size
    nl = np.flatnonzero(a == 10).astype(np.int64)
    starts = np.concatenate([np.zeros(1, np.int64), nl + 1])
    if starts[-1] >= n:                     # nothing follows a final '\n' (and an empty input has no line)
        starts = starts[:-1]
    ends = np.concatenate([nl, np.full(1, n, np.int64)])[:starts.size]
    before = a[np.maximum(ends - 1, 0)]
    cr = (ends < n) & (ends > starts) & (before == 13)
    return starts, ends - cr


def per_read_np(a):
    """per_read as an int64 array of shape (reads, 5)"""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    starts, tends = line_spans_np(a)
    lines = starts.size
    reads = (lines + 3) // 4
    out = np.zeros((reads, 5), np.int64)
    if reads == 0:
        return out, lines

    def padded(v):
        p = np.zeros(4 * reads, np.int64)
        p[:lines] = v
        return p.reshape(reads, 4)

    s4, e4 = padded(starts), padded(tends)
    out[:, 0] = e4[:, 1] - s4[:, 1]
    out[:, 3] = e4[:, 3] - s4[:, 3]

    def ranged(weights, dtype, col_line, col_out):
        c = np.zeros(a.size + 1, dtype)
        np.cumsum(weights, dtype=dtype, out=c[1:])
        out[:, col_out] = (c[e4[:, col_line]] - c[s4[:, col_line]]).astype(np.int64)

    ranged((a == 71) | (a == 67), np.uint32, 1, 1)
    ranged(a == 78, np.uint32, 1, 2)
    ranged(a, np.uint64, 3, 4)
    return out, lines


def _nx(lens_desc, bases, x):
    acc = 0
    for k, v in enumerate(lens_desc):
        acc += v
        if acc * 100 >= bases * x:
            return v, k + 1
    raise AssertionError("unreachable")


def summary_of(rows):
    """every field of scfq_read_summary that follows from the rows (a list of 5-tuples or an (reads, 5) array)"""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 5)
    reads = rows.shape[0]
    s = {"reads": reads}
    for k, name in enumerate(("bases", "gc_bases", "n_bases", "qual_bytes", "qual_sum")):
        s[name] = int(rows[:, k].sum(dtype=np.uint64)) if reads else 0
    lens = rows[:, 0]
    s["min_len"] = int(lens.min()) if reads else 0
    s["max_len"] = int(lens.max()) if reads else 0
    s["n50"] = s["l50"] = s["n90"] = s["l90"] = 0
    if s["bases"]:
        desc = np.sort(lens)[::-1]
        acc = np.cumsum(desc.astype(np.uint64)).astype(object) if reads < 100000 else None
        if acc is not None:
            s["n50"], s["l50"] = _nx([int(v) for v in desc], s["bases"], 50)
            s["n90"], s["l90"] = _nx([int(v) for v in desc], s["bases"], 90)
        else:                                # (bases * 100 < 2^63 for every input of the tests)
            acc = np.cumsum(desc, dtype=np.int64) * 100
            for x in (50, 90):
                k = int(np.searchsorted(acc, s["bases"] * x, side="left"))
                s["n%d" % x], s["l%d" % x] = int(desc[k]), k + 1
    len_hist = [0] * 65
    gc_hist = [0] * 102
    meanq_hist = [0] * 256
    if reads:
        bitlen = np.where(lens > 0, np.frexp(lens.astype(np.float64))[1], 0)      # lengths < 2^53: exact
        for k, c in zip(*np.unique(bitlen, return_counts=True)):
            len_hist[int(k)] = int(c)
        den = rows[:, 0] - rows[:, 2]
        gbin = np.where(den > 0, (100 * rows[:, 1]) // np.maximum(den, 1), 101)
        for k, c in zip(*np.unique(gbin, return_counts=True)):
            gc_hist[int(k)] = int(c)
        has_q = rows[:, 3] > 0
        qbin = rows[has_q, 4] // rows[has_q, 3]
        for k, c in zip(*np.unique(qbin, return_counts=True)):
            meanq_hist[int(k)] = int(c)
        s["no_qual"] = int((~has_q).sum())
    else:
        s["no_qual"] = 0
    s["len_hist"], s["gc_hist"], s["meanq_hist"] = len_hist, gc_hist, meanq_hist
    return s


def assert_summary(got, rows, input_bytes, lines, ctx=""):
    """got: scfq.ReadSummary; every field compared with =="""
    want = summary_of(rows)
    want["input_bytes"], want["lines"] = input_bytes, lines
    for name, v in want.items():
        g = getattr(got, name)
        g = list(g) if isinstance(v, list) else int(g)
        assert g == v, (ctx, name, g if not isinstance(v, list) else [(k, a, b) for k, (a, b) in enumerate(zip(g, v)) if a != b][:8], v if not isinstance(v, list) else "")


def row_text(rows):
    """the fq-readstats TSV row the rows give (mean_len and mean_qual by the `$float` rule: "%.16g", ".0" when bare, nan)"""
    s = summary_of(rows)

    def nim(num, den):
        if den == 0:
            return "nan" if num == 0 else "inf"
        t = "%.16g" % (num / den)
        return t if any(ch in t for ch in ".einf") else t + ".0"

    return "\t".join([str(s[k]) for k in ("reads", "bases", "min_len", "max_len")] + [nim(s["bases"], s["reads"])] +
                     [str(s[k]) for k in ("n50", "l50", "n90", "l90")] + [nim(s["qual_sum"], s["qual_bytes"])])

"""The checker of fq-adapters, twice: a plain restatement of the definitions in include/sc_fqcount.h (lines as _readstats_check.py
has them; probe j occurs at position p of a sequence line when the line's text holds it there byte for byte) with bytes.find and a
loop over the starts, and a numpy form (one shifted compare per probe byte) for inputs too large for a Python loop.  Both return
(rows, hits, total, max_seq_len, lines): rows is a dense uint64 array of shape (max_seq_len, 9) — first[0 .. 8) and any —, hits a list
of eight and total a list of nine integers."""
import numpy as np

from _readstats_check import line_spans_np, lines_of

MAX_PROBES = 8
COLS = MAX_PROBES + 1
SUMMARY_WORDS = 42
NONE = np.iinfo(np.int64).max


def _enc(probes):
    return [p.encode() if isinstance(p, str) else bytes(p) for p in probes]


def adapters_of(data, probes):
    probes = _enc(probes)
    ls = lines_of(bytes(data))
    max_len = max((len(ls[j]) for j in range(1, len(ls), 4)), default=0)
    rows = np.zeros((max_len, COLS), np.uint64)
    hits, total = [0] * MAX_PROBES, [0] * COLS
    for j in range(1, len(ls), 4):
        s = ls[j]
        firsts = []
        for k, p in enumerate(probes):
            hits[k] += sum(1 for i in range(len(s) - len(p) + 1) if s[i:i + len(p)] == p)
            f = s.find(p)
            if f >= 0:
                rows[f, k] += 1
                total[k] += 1
                firsts.append(f)
        if firsts:
            rows[min(firsts), MAX_PROBES] += 1
            total[MAX_PROBES] += 1
    return rows, hits, total, max_len, len(ls)


def adapters_of_np(a, probes):
    probes = _enc(probes)
    a = np.ascontiguousarray(a, dtype=np.uint8)
    n = a.size
    starts, tends = line_spans_np(a)
    lines = starts.size
    s, e = starts[1::4], tends[1::4]
    max_len = int((e - s).max()) if s.size else 0
    rows = np.zeros((max_len, COLS), np.uint64)
    hits, total = [0] * MAX_PROBES, [0] * COLS
    firsts = np.full((s.size, max(len(probes), 1)), NONE, np.int64)
    for k, p in enumerate(probes):
        m = len(p)
        if n < m or s.size == 0:
            continue
        ok = a[:n - m + 1] == p[0]
        for i in range(1, m):
            ok &= a[i:n - m + 1 + i] == p[i]
        q = np.flatnonzero(ok).astype(np.int64)
        ln = np.searchsorted(starts, q, side="right") - 1
        keep = (ln % 4 == 1) & (q + m <= tends[ln])
        q, ln = q[keep], ln[keep]
        hits[k] = int(q.size)
        np.minimum.at(firsts[:, k], ln // 4, q - starts[ln])
        f = firsts[:, k]
        f = f[f != NONE]
        if f.size:
            rows[:, k] = np.bincount(f, minlength=max_len)
            total[k] = int(f.size)
    if s.size:
        f = firsts.min(axis=1)
        f = f[f != NONE]
        if f.size:
            rows[:, MAX_PROBES] = np.bincount(f, minlength=max_len)
            total[MAX_PROBES] = int(f.size)
    return rows, hits, total, max_len, lines


def same(p, q):
    """two checker results, compared exactly"""
    return np.array_equal(p[0], q[0]) and p[0].shape == q[0].shape and tuple(p[1:]) == tuple(q[1:])


def row_of(r):
    return [int(v) for v in r.first] + [int(r.any)]


def assert_result(got, want, probes, cap, input_bytes, ctx=""):
    """got: (scfq.AdapterSummary, rows or None) of a call with `cap` rows; want: a checker's tuple; every field compared with =="""
    s, rows = got
    wr, hits, total, max_len, lines = want
    probes = _enc(probes)
    positions = min(cap, max_len)
    head = dict(struct_size=8 * SUMMARY_WORDS, reads=(lines + 3) // 4, lines=lines, input_bytes=input_bytes, n_probes=len(probes),
                max_seq_len=max_len, positions=positions)
    for name, v in head.items():
        assert int(getattr(s, name)) == v, (ctx, cap, name, int(getattr(s, name)), v)
    assert int(s.abi_version) > 0, ctx
    assert list(s.probe_len) == [len(p) for p in probes] + [0] * (MAX_PROBES - len(probes)), (ctx, list(s.probe_len))
    assert list(s.hits) == list(hits), (ctx, cap, "hits", list(s.hits), hits)
    assert row_of(s.total) == list(total), (ctx, cap, "total", row_of(s.total), total)
    tail = [int(v) for v in wr[positions:].sum(axis=0, dtype=np.uint64)]
    assert row_of(s.tail) == tail, (ctx, cap, "tail", row_of(s.tail), tail)
    if cap == 0:
        assert rows is None, ctx
    else:
        assert rows.shape == (positions, COLS) and rows.dtype == np.uint64, (ctx, cap, rows.shape)
        if not np.array_equal(rows, wr[:positions]):
            bad = np.flatnonzero((rows != wr[:positions]).any(axis=1))
            raise AssertionError((ctx, cap, "rows differ at", bad[:8].tolist(), rows[bad[:4]].tolist(), wr[bad[:4]].tolist()))


def nim(num, den):
    """num / den by the `$float` rule: "%.16g", ".0" when bare, nan"""
    if den == 0:
        return "nan" if num == 0 else "inf"
    t = "%.16g" % (num / den)
    return t if any(ch in t for ch in ".einf") else t + ".0"


def cli_text(want, n_probes, max_positions=1000, counts=False, suffix=""):
    """stdout of `sc fq-adapters [--counts] [--max-positions=N]` for one file"""
    wr, hits, total, max_len, lines = want
    reads = (lines + 3) // 4
    cols = list(range(n_probes)) + [MAX_PROBES]
    positions = min(max_positions, max_len)
    out = []
    acc = [0] * COLS
    for p in range(positions):
        for c in cols:
            acc[c] += int(wr[p, c])
        vals = [str(int(wr[p, c])) for c in cols] if counts else [nim(100 * acc[c], reads) for c in cols]
        out.append("%d\t%s%s\n" % (p + 1, "\t".join(vals), suffix))
    tail = [int(v) for v in wr[positions:].sum(axis=0, dtype=np.uint64)]
    if any(tail):
        vals = [str(tail[c]) for c in cols] if counts else [nim(100 * total[c], reads) for c in cols]
        out.append(">%d\t%s%s\n" % (max_positions, "\t".join(vals), suffix))
    return "".join(out)


def totals_text(want, names, probes, suffix=""):
    """stdout of `sc fq-adapters --totals` for one file"""
    wr, hits, total, max_len, lines = want
    reads = (lines + 3) // 4
    out = ["%s\t%s\t%d\t%d\t%s\t%d%s\n" % (nm, p if isinstance(p, str) else p.decode(), reads, total[k], nim(100 * total[k], reads), hits[k], suffix)
           for k, (nm, p) in enumerate(zip(names, probes))]
    out.append("any\t*\t%d\t%d\t%s\t%d%s\n" % (reads, total[MAX_PROBES], nim(100 * total[MAX_PROBES], reads), sum(hits), suffix))
    return "".join(out)

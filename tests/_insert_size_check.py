"""The checker of fq-insert-size, twice: a plain restatement of the definitions in include/sc_fqcount.h (lines as _readstats_check.py has
them; every offset of every pair, byte by byte) and a numpy form (all pairs at once, one shifted compare per offset) for inputs too
large for a Python loop.  Both return a dict: recs — an int64 array of shape (pairs, 3): offset, overlap, mismatches, (0, 0, 0) without
an accepted offset and (0, 0, 0xFFFF) for a too-long pair —, hist — 1024 uint64 —, and every integer field of scfq_insert_summary
but struct_size and abi_version."""
import math

import numpy as np

from _readstats_check import line_spans_np, lines_of

MAX_LEN = 512
HIST_BINS = 1024
SUMMARY_WORDS = 25
DEFAULTS = (30, 5, 20)
COMP = {65: 84, 84: 65, 67: 71, 71: 67}      # A <-> T, C <-> G
FIELDS = ("reads1", "reads2", "lines1", "lines2", "input_bytes1", "input_bytes2", "pairs", "unpaired", "overlapped", "not_overlapped",
          "too_long", "read_through", "overlap_bases", "mismatches", "insert_sum", "insert_sq_sum", "min_insert", "max_insert", "mode_insert",
          "median_insert", "min_overlap", "max_mismatches", "max_mismatch_pct")


def pair_of(a, b, params=DEFAULTS):
    """(offset, overlap, mismatches) of one pair of sequence texts, or None without an accepted offset"""
    min_overlap, max_mm, max_pct = params
    la, lb = len(a), len(b)
    c = [COMP.get(b[lb - 1 - y], -1) for y in range(lb)]      # (-1: agrees with nothing)
    best = None
    for d in range(-(lb - 1), la):
        lo, hi = max(0, -d), min(lb, la - d)
        ov = hi - lo
        if ov < min_overlap:
            continue
        mm = sum(1 for y in range(lo, hi) if a[y + d] != c[y])
        if mm <= max_mm and 100 * mm <= max_pct * ov:
            key = (ov, -mm, d)
            if best is None or key > best:
                best = key
    return None if best is None else (best[2], best[0], -best[1])


def _finish(out, recs, la, lb, params):
    """the histogram and every sum from the records and the lengths of the pairs"""
    recs = np.asarray(recs, np.int64).reshape(-1, 3)
    la, lb = np.asarray(la, np.int64), np.asarray(lb, np.int64)
    too_long = recs[:, 2] == 0xFFFF
    hit = (recs[:, 1] > 0) & ~too_long
    ins = (recs[:, 0] + lb)[hit]
    hist = np.bincount(ins, minlength=HIST_BINS).astype(np.uint64)
    out.update(recs=recs, hist=hist, pairs=int(recs.shape[0]), overlapped=int(hit.sum()), too_long=int(too_long.sum()),
               read_through=int((ins < np.maximum(la, lb)[hit]).sum()), overlap_bases=int(recs[hit, 1].sum()),
               mismatches=int(recs[hit, 2].sum()), insert_sum=int(ins.sum()), insert_sq_sum=int((ins * ins).sum()),
               min_insert=int(ins.min()) if ins.size else 0, max_insert=int(ins.max()) if ins.size else 0,
               mode_insert=int(hist.argmax()) if ins.size else 0, min_overlap=params[0], max_mismatches=params[1], max_mismatch_pct=params[2])
    out["not_overlapped"] = out["pairs"] - out["overlapped"] - out["too_long"]
    cum = np.cumsum(hist.astype(np.int64))
    out["median_insert"] = int(np.argmax(2 * cum >= out["overlapped"])) if ins.size else 0
    return out


def insert_of(data1, data2=None, params=DEFAULTS):
    """data2 = None: data1 is interleaved"""
    params = tuple(params)
    l1 = lines_of(bytes(data1))
    out = dict(lines1=len(l1), lines2=0, reads1=(len(l1) + 3) // 4, reads2=0, input_bytes1=len(data1), input_bytes2=0)
    seq1 = [l1[4 * i + 1] if 4 * i + 1 < len(l1) else b"" for i in range(out["reads1"])]
    if data2 is None:
        mates = [(seq1[2 * i], seq1[2 * i + 1]) for i in range(len(seq1) // 2)]
        out["unpaired"] = len(seq1) & 1
    else:
        l2 = lines_of(bytes(data2))
        out.update(lines2=len(l2), reads2=(len(l2) + 3) // 4, input_bytes2=len(data2))
        seq2 = [l2[4 * i + 1] if 4 * i + 1 < len(l2) else b"" for i in range(out["reads2"])]
        mates = list(zip(seq1, seq2))
        out["unpaired"] = abs(len(seq1) - len(seq2))
    recs = []
    for a, b in mates:
        if len(a) > MAX_LEN or len(b) > MAX_LEN:
            recs.append((0, 0, 0xFFFF))
        else:
            recs.append(pair_of(a, b, params) or (0, 0, 0))
    return _finish(out, recs, [len(a) for a, _ in mates], [len(b) for _, b in mates], params)


def _codes(a, s, ln, width, reverse, pad):
    """(pairs, width) codes of the texts [s, s + ln) of a: A C G T -> 0 1 2 3 (complemented when `reverse`, which also reads the text
    back to front), anything else and what lies behind the text -> pad"""
    y = np.arange(width, dtype=np.int64)[None, :]
    inside = y < ln[:, None]
    pos = s[:, None] + (ln[:, None] - 1 - y if reverse else y)
    b = a[np.where(inside, pos, 0)] if a.size else np.zeros(pos.shape, np.uint8)
    table = np.full(256, pad, np.uint8)
    for k, ch in enumerate(b"TGCA" if reverse else b"ACGT"):
        table[ch] = k
    return np.where(inside, table[b], pad).astype(np.uint8)


def insert_of_np(a1, a2=None, params=DEFAULTS, chunk=4096):
    params = tuple(params)
    min_overlap, max_mm, max_pct = params
    a1 = np.ascontiguousarray(a1, dtype=np.uint8)
    s1, e1 = line_spans_np(a1)
    out = dict(lines1=int(s1.size), lines2=0, reads1=(int(s1.size) + 3) // 4, reads2=0, input_bytes1=int(a1.size), input_bytes2=0)

    def seqs(s, e, reads):
        ps, pe = np.zeros(reads, np.int64), np.zeros(reads, np.int64)
        k = s[1::4].size
        ps[:k], pe[:k] = s[1::4], e[1::4]
        return ps, pe - ps

    sa, la = seqs(s1, e1, out["reads1"])
    if a2 is None:
        pairs = out["reads1"] // 2
        out["unpaired"] = out["reads1"] & 1
        arr_b, sb, lb = a1, sa[1:2 * pairs:2], la[1:2 * pairs:2]
        sa, la = sa[0:2 * pairs:2], la[0:2 * pairs:2]
    else:
        arr_b = np.ascontiguousarray(a2, dtype=np.uint8)
        s2, e2 = line_spans_np(arr_b)
        out.update(lines2=int(s2.size), reads2=(int(s2.size) + 3) // 4, input_bytes2=int(arr_b.size))
        sb, lb = seqs(s2, e2, out["reads2"])
        pairs = min(out["reads1"], out["reads2"])
        out["unpaired"] = max(out["reads1"], out["reads2"]) - pairs
        sa, la, sb, lb = sa[:pairs], la[:pairs], sb[:pairs], lb[:pairs]
    recs = np.zeros((pairs, 3), np.int64)
    too_long = (la > MAX_LEN) | (lb > MAX_LEN)
    recs[too_long, 2] = 0xFFFF
    todo = np.flatnonzero(~too_long & (la >= min_overlap) & (lb >= min_overlap))
    todo = todo[np.argsort(np.maximum(la, lb)[todo], kind="stable")]      # a chunk is as wide as its longest read: like with like
    none = np.iinfo(np.int64).max
    for c0 in range(0, todo.size, chunk):
        idx = todo[c0:c0 + chunk]
        cla, clb = la[idx], lb[idx]
        wa, wb = int(cla.max()), int(clb.max())
        # A between wb pad columns on either side: column y + d + wb of it faces column y of C
        A = np.full((idx.size, wa + 2 * wb), 4, np.uint8)
        A[:, wb:wb + wa] = _codes(a1, sa[idx], cla, wa, False, 4)
        C = _codes(arr_b, sb[idx], clb, wb, True, 5)
        best = np.full(idx.size, none, np.int64)
        for d in range(min_overlap - wb, wa - min_overlap + 1):
            ov = np.minimum(clb, cla - d) - np.maximum(0, -d)
            agree = np.count_nonzero(A[:, wb + d:wb + d + wb] == C, axis=1)
            mm = ov - agree
            ok = (ov >= min_overlap) & (mm <= max_mm) & (100 * mm <= max_pct * ov)
            key = ((1023 - ov) << 48) | (mm << 32) | (1024 - d)
            best = np.where(ok & (key < best), key, best)
        got = best != none
        recs[idx[got], 0] = 1024 - (best[got] & 0xFFFFFFFF)
        recs[idx[got], 1] = 1023 - (best[got] >> 48)
        recs[idx[got], 2] = (best[got] >> 32) & 0xFFFF
    return _finish(out, recs, la, lb, params)


def same(p, q):
    """two checker results, compared exactly"""
    return set(p) == set(q) and all(np.array_equal(p[k], q[k]) if k in ("recs", "hist") else p[k] == q[k] for k in p)


def assert_result(got, want, ctx="", recs=None):
    """got: (scfq.InsertSummary, histogram) of a call; recs: the table the call filled, rows of (offset, overlap, mismatches);
    want: a checker's dict; every field compared with =="""
    s, hist = got
    assert int(s.struct_size) == 8 * SUMMARY_WORDS and int(s.abi_version) > 0, ctx
    for name in FIELDS:
        assert int(getattr(s, name)) == want[name], (ctx, name, int(getattr(s, name)), want[name])
    assert s.pairs == s.overlapped + s.not_overlapped + s.too_long, ctx
    assert hist.shape == (HIST_BINS,) and int(hist[0]) == 0, ctx
    if not np.array_equal(hist, want["hist"]):
        bad = np.flatnonzero(hist != want["hist"])
        raise AssertionError((ctx, "histogram differs at", bad[:8].tolist(), hist[bad[:8]].tolist(), want["hist"][bad[:8]].tolist()))
    if recs is not None:
        recs = np.asarray(recs, np.int64).reshape(-1, 3)
        assert recs.shape == want["recs"].shape, (ctx, recs.shape, want["recs"].shape)
        if not np.array_equal(recs, want["recs"]):
            bad = np.flatnonzero((recs != want["recs"]).any(axis=1))
            raise AssertionError((ctx, "records differ at", bad[:8].tolist(), recs[bad[:4]].tolist(), want["recs"][bad[:4]].tolist()))


def nimf(v):
    """a double by the `$float` rule: "%.16g", ".0" when bare, nan"""
    if v != v:
        return "nan"
    t = "%.16g" % v
    return t if any(ch in t for ch in ".einf") else t + ".0"


def div(num, den):
    return float("nan") if den == 0 and num == 0 else float("inf") if den == 0 else num / den


def summary_text(w):
    """the row of scfq_format_insert_size_tsv for the integers of a checker's dict (or any mapping with those names)"""
    n = w["overlapped"]
    num = n * w["insert_sq_sum"] - w["insert_sum"] ** 2          # exact: Python integers
    sd = math.sqrt(float(num)) / n if n else float("nan")
    return "\t".join([str(w["pairs"]), str(n), nimf(div(100 * n, w["pairs"])), str(w["min_insert"]), str(w["median_insert"]),
                      nimf(div(w["insert_sum"], n)), nimf(sd), str(w["mode_insert"]), str(w["max_insert"]), str(w["read_through"]),
                      nimf(div(w["mismatches"], w["overlap_bases"]))])


def cli_text(want, dist=False, suffix=""):
    """stdout of `sc fq-insert-size [--dist]` for one pair of files (or one interleaved file)"""
    if dist:
        return "".join("%d\t%d%s\n" % (s, int(c), suffix) for s, c in enumerate(want["hist"]) if c)
    return summary_text(want) + suffix + "\n"


# ---- inputs for the tests -------------------------------------------------------------------------------------------------
_RC = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s):
    return bytes(s).translate(_RC)[::-1]


def random_dna(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def planted(rng, la, lb, insert):
    """mates of la and lb random bases whose true offset is d = insert - lb: what lies outside the overlap is unrelated"""
    d = insert - lb
    lo, hi = min(0, d), max(la, d + lb)
    g = random_dna(rng, hi - lo)
    return g[-lo:-lo + la], revcomp(g[d - lo:d - lo + lb])


def fastq(seqs, eol=b"\n", name=b"r"):
    return b"".join(b"@" + name + str(i).encode() + eol + bytes(s) + eol + b"+" + eol + b"I" * len(s) + eol for i, s in enumerate(seqs))


def interleave(m1, m2):
    return [s for pair in zip(m1, m2) for s in pair]


def paired_block(rng, pairs, la, lb, unrelated=0.1, errors=0.01):
    """(r1, r2) as uint8 arrays: `pairs` records each, mates of la and lb bases cut from one random stretch at random places (either
    sign of d, overlaps from none to whole), a share of them unrelated, a share of the bases turned into N: built without a Python loop"""
    width = la + lb + max(la, lb)
    letters = np.frombuffer(b"ACGT", np.uint8)
    g = rng.integers(0, 4, (pairs, width), dtype=np.uint8)
    sa = rng.integers(0, width - la + 1, pairs)
    sc = rng.integers(0, width - lb + 1, pairs)
    rows = np.arange(pairs)[:, None]
    a = g[rows, sa[:, None] + np.arange(la)[None, :]]
    c = g[rows, sc[:, None] + np.arange(lb)[None, :]]
    other = rng.random(pairs) < unrelated
    c[other] = rng.integers(0, 4, (int(other.sum()), lb), dtype=np.uint8)
    b = (3 - c)[:, ::-1]                                          # the reverse complement, in codes

    def records(codes, ln):
        text = letters[codes]
        text[rng.random(text.shape) < errors] = ord("N")
        rec = np.empty((pairs, 3 + ln + 3 + ln + 1), np.uint8)
        rec[:, :3] = np.frombuffer(b"@p\n", np.uint8)
        rec[:, 3:3 + ln] = text
        rec[:, 3 + ln:6 + ln] = np.frombuffer(b"\n+\n", np.uint8)
        rec[:, 6 + ln:6 + 2 * ln] = ord("I")
        rec[:, 6 + 2 * ln] = 10
        return rec.reshape(-1)

    return records(a, la), records(b, lb)

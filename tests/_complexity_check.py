"""The checker of fq-complexity: a plain restatement of the contract in include/sc_fqcount.h.  The per-read part exists twice: read_def is
the definition as written there (every interval, every sub-interval, pairs counted one by one), read_rows the row recurrence
best(i, j) = max(c / (l - 1), best(i, j - 1), best(i + 1, j)) for inputs too large for the definition (read_rows_many: the same steps on
many reads at once).  Both return (mask, score, intervals,
first): mask a Python integer with bit p set for a masked position p.  complexity_of works on whole FASTQ texts (lines as
_readstats_check.py has them) and returns a dict: out1, out2 — bytes —, recs — a list of (score, masked, first, intervals) —, hist — a
list of SCORE_BINS numbers — and every field of scfq_cplx_stats but struct_size and abi_version."""
import numpy as np

from _readstats_check import lines_of

MAX_LEN = 512
STATS_WORDS = 29
SCORE_BINS = 312
INTERLEAVED = 1
MASK_NONE, MASK_LOWER, MASK_N = 0, 1, 2
MASK_NAMES = {"none": MASK_NONE, "lower": MASK_LOWER, "n": MASK_N}
NO_FIRST = 0xFFFF
TOO_LONG_REC = (0xFFFF, 0, 0xFFFF, 0)
DEFAULTS = dict(interleaved=False, window=64, threshold=20, mask=MASK_LOWER, max_masked_pct=100)
PARAM_FIELDS = ("flags", "window", "threshold", "mask", "max_masked_pct")
FIELDS = ("reads1", "reads2", "lines1", "lines2", "input_bytes1", "input_bytes2", "pairs", "unpaired", "reads_in", "reads_out", "too_long",
          "low_reads", "dropped_reads", "masked_reads", "perfect_intervals", "bases_in", "bases_out", "masked_bases", "masked_bases_out",
          "max_score", "out1_bytes", "out2_bytes") + PARAM_FIELDS
REPORT_FIELDS = ("reads_in", "reads_out", "dropped_reads", "low_reads", "too_long", "pairs", "unpaired", "masked_reads", "perfect_intervals",
                 "bases_in", "bases_out", "masked_bases", "masked_bases_out", "max_score", "out1_bytes", "out2_bytes")
STATS_HEADER = "\t".join(REPORT_FIELDS)
REC_HEADER = "read\tlength\tscore\tmasked\tfirst\tintervals"
HIST_HEADER = "score\treads"
_CODE = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3}


def triplets(S):
    """t(i) for i in [0, L - 2): the 6-bit code, or None for a position that is not valid"""
    out = []
    for i in range(max(len(S) - 2, 0)):
        c = [_CODE.get(S[i + k]) for k in range(3)]
        out.append(None if None in c else 16 * c[0] + 4 * c[1] + c[2])
    return out


def _finish(n, perfect, score):
    mask, first = 0, NO_FIRST
    for i, j in perfect:
        mask |= ((1 << (j + 3)) - 1) & ~((1 << i) - 1)
        first = min(first, i)
    return mask, score, len(perfect), first


def read_def(S, window=64, threshold=20):
    """the definition: every interval against every one of its sub-intervals.  pairs[a, b] says a < b, both valid, t(a) == t(b); c(i, j) is
    the number of pairs inside the square [i, j] x [i, j]"""
    t = triplets(S)
    n = len(t)
    pairs = np.zeros((n, n), np.int64)
    for a in range(n):
        for b in range(a + 1, n):
            pairs[a, b] = t[a] is not None and t[a] == t[b]
    c = np.zeros((n, n), np.int64)
    for i in range(n):
        for j in range(i + 1, min(i + window - 2, n)):
            c[i, j] = pairs[i:j + 1, i:j + 1].sum()
    width = np.arange(n)[None, :] - np.arange(n)[:, None]              # l' - 1 of [a, b]
    perfect, score = [], 0
    for i in range(n):
        for j in range(i + 1, min(i + window - 2, n)):
            cij, l = int(c[i, j]), j - i + 1
            score = max(score, 10 * cij // (l - 1))
            if not 10 * cij > threshold * (l - 1):
                continue
            inside = width[i:j + 1, i:j + 1] > 0                       # the sub-intervals [a, b], i <= a < b <= j
            if (c[i:j + 1, i:j + 1] * (l - 1) <= cij * width[i:j + 1, i:j + 1])[inside].all():
                perfect.append((i, j))
    return _finish(n, perfect, score)


def read_rows(S, window=64, threshold=20):
    """the row recurrence, all starts of a read at once: step l adds triplet j = i + l - 1 to the interval of every start i"""
    t = triplets(S)
    n = len(t)
    if n < 2:
        return 0, 0, 0, NO_FIRST
    code = np.array([-1 - k if v is None else v for k, v in enumerate(t)], dtype=np.int64)      # (an invalid one equals nothing)
    steps = min(window - 2, n)
    # near[j, m]: the triplets equal to t(j) among the m in front of it
    near = np.zeros((n, steps + 1), np.int64)
    for d in range(1, steps):
        near[d:, d] = code[d:] == code[:-d]
    near = np.cumsum(near, axis=1)
    c = np.zeros(n, np.int64)
    bn, bd = np.zeros(n + 1, np.int64), np.ones(n + 1, np.int64)     # best(i, j - 1) as a fraction; entry n: no start
    end = np.full(n, -1, np.int64)
    count, score = 0, 0
    for l in range(2, steps + 1):
        m = n - l + 1                                       # starts 0 .. m - 1 have their end j = i + l - 1 inside
        i = np.arange(m)
        c[:m] += near[i + l - 1, l - 1]
        num, den = c[:m], l - 1
        nn, nd = bn[1:m + 1].copy(), bd[1:m + 1].copy()     # best(i + 1, j): the neighbour's value of the step before
        on, od = bn[:m].copy(), bd[:m].copy()
        high = 10 * num > threshold * den
        perfect = high & (num * od >= on * den) & (num * nd >= nn * den)
        end[:m] = np.where(perfect, i + l - 1, end[:m])
        count += int(perfect.sum())
        score = max(score, int((10 * num // den).max()))
        take_n = nn * od > on * nd
        xn, xd = np.where(take_n, nn, on), np.where(take_n, nd, od)
        take_c = num * xd >= xn * den
        bn[:m], bd[:m] = np.where(take_c, num, xn), np.where(take_c, den, xd)
    mask, first = 0, NO_FIRST
    for i in np.flatnonzero(end >= 0):
        mask |= ((1 << (int(end[i]) + 3)) - 1) & ~((1 << int(i)) - 1)
        first = min(first, int(i))
    return mask, score, count, first


def read_rows_many(seqs, window=64, threshold=20):
    """read_rows on many reads at once.  The reads are padded to one length with triplets that are not valid: an interval that reaches
    into the padding has the pairs of its part inside the read and is longer, so it is never high and never raises a best"""
    trips = [triplets(S) for S in seqs]
    n = max([len(t) for t in trips] + [0])
    if n < 2:
        return [(0, 0, 0, NO_FIRST)] * len(seqs)
    R = len(seqs)
    code = -1 - np.arange(R * n, dtype=np.int64).reshape(R, n)
    for r, t in enumerate(trips):
        for k, v in enumerate(t):
            if v is not None:
                code[r, k] = v
    steps = min(window - 2, n)
    near = np.zeros((R, n, steps + 1), np.int64)
    for d in range(1, steps):
        near[:, d:, d] = code[:, d:] == code[:, :-d]
    near = np.cumsum(near, axis=2)
    c = np.zeros((R, n), np.int64)
    bn, bd = np.zeros((R, n + 1), np.int64), np.ones((R, n + 1), np.int64)
    end = np.full((R, n), -1, np.int64)
    count, score = np.zeros(R, np.int64), np.zeros(R, np.int64)
    for l in range(2, steps + 1):
        m = n - l + 1
        i = np.arange(m)
        c[:, :m] += near[:, i + l - 1, l - 1]
        num, den = c[:, :m], l - 1
        nn, nd = bn[:, 1:m + 1].copy(), bd[:, 1:m + 1].copy()
        on, od = bn[:, :m].copy(), bd[:, :m].copy()
        perfect = (10 * num > threshold * den) & (num * od >= on * den) & (num * nd >= nn * den)
        end[:, :m] = np.where(perfect, i + l - 1, end[:, :m])
        count += perfect.sum(axis=1)
        score = np.maximum(score, (10 * num // den).max(axis=1))
        take_n = nn * od > on * nd
        xn, xd = np.where(take_n, nn, on), np.where(take_n, nd, od)
        take_c = num * xd >= xn * den
        bn[:, :m], bd[:, :m] = np.where(take_c, num, xn), np.where(take_c, den, xd)
    out = []
    for r in range(R):
        mask, first = 0, NO_FIRST
        for i in np.flatnonzero(end[r] >= 0):
            mask |= ((1 << (int(end[r, i]) + 3)) - 1) & ~((1 << int(i)) - 1)
            first = min(first, int(i))
        out.append((mask, int(score[r]), int(count[r]), first))
    return out


def masked_text(S, mask, mode):
    if mode == MASK_NONE or not mask:
        return bytes(S)
    out = bytearray(S)
    for p in range(len(S)):
        if mask >> p & 1:
            if mode == MASK_N:
                out[p] = ord("N")
            elif ord("A") <= out[p] <= ord("Z"):
                out[p] |= 0x20
    return bytes(out)


def resolve(kw):
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    p = dict(DEFAULTS, **kw)
    p["mask"] = MASK_NAMES.get(p["mask"], p["mask"])
    p["flags"] = INTERLEAVED if p["interleaved"] else 0
    return p


def _record(lines, i):
    return [lines[4 * i + k] if 4 * i + k < len(lines) else b"" for k in range(4)]


def complexity_of(data1, data2=None, per_read=read_rows, cache=None, **kw):
    """data2 = None: data1 is single-end, or interleaved with interleaved=True.  cache: a dict that keeps the per-read results between
    calls (the key holds the sequence and the two parameters they depend on)"""
    p = resolve(kw)
    cache = {} if cache is None else cache
    l1 = lines_of(bytes(data1))
    out = dict(lines1=len(l1), lines2=0, reads1=(len(l1) + 3) // 4, reads2=0, input_bytes1=len(data1), input_bytes2=0, pairs=0, unpaired=0)
    if data2 is not None:
        assert not p["interleaved"]
        l2 = lines_of(bytes(data2))
        out.update(lines2=len(l2), reads2=(len(l2) + 3) // 4, input_bytes2=len(data2))
        pairs = min(out["reads1"], out["reads2"])
        out.update(pairs=pairs, unpaired=max(out["reads1"], out["reads2"]) - pairs)
        units = [((l1, i), (l2, i)) for i in range(pairs)]
    elif p["interleaved"]:
        out.update(pairs=out["reads1"] // 2, unpaired=out["reads1"] & 1)
        units = [((l1, 2 * i), (l1, 2 * i + 1)) for i in range(out["pairs"])]
    else:
        units = [((l1, i),) for i in range(out["reads1"])]
    if per_read is read_rows:                                 # what the cache does not hold yet, 256 reads of like lengths at a time
        todo = sorted({_record(ls, i)[1] for unit in units for ls, i in unit} - {k[0] for k in cache if k[1:] == (p["window"], p["threshold"])}, key=len)
        todo = [S for S in todo if len(S) <= MAX_LEN]
        for at in range(0, len(todo), 256):
            for S, got in zip(todo[at:at + 256], read_rows_many(todo[at:at + 256], p["window"], p["threshold"])):
                cache[(S, p["window"], p["threshold"])] = got
    n = dict.fromkeys(("reads_in", "reads_out", "too_long", "low_reads", "dropped_reads", "masked_reads", "perfect_intervals", "bases_in",
                       "bases_out", "masked_bases", "masked_bases_out", "max_score"), 0)
    recs, hist, outs = [], [0] * SCORE_BINS, ([], [])
    for unit in units:
        reads = []
        for ls, i in unit:
            h, S, plus, q = _record(ls, i)
            L = len(S)
            if L > MAX_LEN:
                reads.append(dict(L=L, too_long=True, low=False, masked=0, rec=TOO_LONG_REC, text=b"".join(t + b"\n" for t in ls[4 * i:4 * i + 4])))
                continue
            key = (S, p["window"], p["threshold"])
            if key not in cache:
                cache[key] = per_read(S, p["window"], p["threshold"])
            mask, score, intervals, first = cache[key]
            masked = bin(mask).count("1")
            low = L >= 1 and 100 * masked > p["max_masked_pct"] * L
            text = h + b"\n" + masked_text(S, mask, p["mask"]) + b"\n" + plus + b"\n" + q + b"\n"
            reads.append(dict(L=L, too_long=False, low=low, masked=masked, rec=(score, masked, first, intervals), text=text))
        drop = any(r["low"] for r in reads)
        for k, r in enumerate(reads):
            recs.append(r["rec"])
            n["reads_in"] += 1
            n["bases_in"] += r["L"]
            n["too_long"] += r["too_long"]
            n["low_reads"] += r["low"]
            n["masked_reads"] += r["masked"] > 0
            n["masked_bases"] += r["masked"]
            n["perfect_intervals"] += r["rec"][3]
            hist[SCORE_BINS - 1 if r["too_long"] else r["rec"][0]] += 1
            if not r["too_long"]:
                n["max_score"] = max(n["max_score"], r["rec"][0])
            if drop:
                n["dropped_reads"] += 1
                continue
            n["reads_out"] += 1
            n["bases_out"] += r["L"]
            n["masked_bases_out"] += r["masked"]
            outs[0 if (k == 0 or p["interleaved"]) else 1].append(r["text"])
    o1, o2 = b"".join(outs[0]), b"".join(outs[1])
    out.update(n, recs=recs, hist=hist, out1=o1, out2=o2, out1_bytes=len(o1), out2_bytes=len(o2))
    out.update({k: p[k] for k in PARAM_FIELDS})
    return out


def check_identities(w):
    assert w["reads_in"] == w["reads_out"] + w["dropped_reads"]
    assert w["masked_bases_out"] <= w["masked_bases"] <= w["bases_in"] and w["bases_out"] <= w["bases_in"]
    assert w["low_reads"] <= w["dropped_reads"] and w["masked_reads"] <= w["reads_in"] - w["too_long"]


def assert_stats(s, want, ctx=""):
    """s: a scfq.CplxStats; want: a checker's dict; every field compared with =="""
    assert int(s.struct_size) == 8 * STATS_WORDS and int(s.abi_version) > 0, ctx
    for name in FIELDS:
        assert int(getattr(s, name)) == want[name], (ctx, name, int(getattr(s, name)), want[name])
    check_identities({name: int(getattr(s, name)) for name in FIELDS})


def stats_text(w):
    """the row of scfq_format_cplx_stats_tsv for a checker's dict"""
    return "\t".join(str(w[k]) for k in REPORT_FIELDS)


def rec_text(read, rec, length):
    """the row of scfq_format_cplx_rec_tsv"""
    score, masked, first, intervals = rec
    return "%d\t%d\t%s\t%d\t%s\t%d" % (read, length, "-" if score == 0xFFFF else str(score), masked, "-" if first == NO_FIRST else str(first), intervals)


def per_read_text(w, lengths, header=False):
    rows = [REC_HEADER] if header else []
    rows += [rec_text(i, r, lengths[i]) for i, r in enumerate(w["recs"])]
    return "".join(r + "\n" for r in rows)


def hist_text(w, header=False):
    """the rows of `sc fq-complexity --hist`: every score with a read, and the too-long reads last"""
    rows = [HIST_HEADER] if header else []
    rows += ["%d\t%d" % (s, v) for s, v in enumerate(w["hist"][:SCORE_BINS - 1]) if v]
    if w["hist"][SCORE_BINS - 1]:
        rows.append("too_long\t%d" % w["hist"][SCORE_BINS - 1])
    return "".join(r + "\n" for r in rows)


def lengths_of(data1, data2=None, interleaved=False):
    """L of every entry of the per-read table"""
    def seq_lens(data):
        ls = lines_of(bytes(data))
        return [len(_record(ls, i)[1]) for i in range((len(ls) + 3) // 4)]
    a = seq_lens(data1)
    if data2 is not None:
        b = seq_lens(data2)
        return [v for x, y in zip(a, b) for v in (x, y)]
    return a[:len(a) // 2 * 2] if interleaved else a

"""The checker of fq-merge, twice: a plain restatement of the definitions in include/sc_fqcount.h, byte by byte (lines as
_readstats_check.py has them, d* from _insert_size_check.pair_of), and a numpy form for inputs too large for a Python loop (d* from
insert_of_np, the consensus of all merged pairs at once).  Both return a dict: merged, unmerged1, unmerged2 — bytes — and every integer
field of scfq_merge_stats but struct_size and abi_version."""
import numpy as np

from _insert_size_check import DEFAULTS, MAX_LEN, insert_of_np, pair_of
from _readstats_check import line_spans_np, lines_of

STATS_WORDS = 26
FIELDS = ("reads1", "reads2", "lines1", "lines2", "input_bytes1", "input_bytes2", "pairs", "unpaired", "merged", "not_overlapped", "too_long",
          "merged_bases", "overlap_bases", "mismatches", "took_mate1", "took_mate2", "neither_valid", "merged_bytes", "unmerged1_bytes",
          "unmerged2_bytes", "min_overlap", "max_mismatches", "max_mismatch_pct", "phred_offset")
OUTPUTS = ("merged", "unmerged1", "unmerged2")
COMP = {65: 84, 84: 65, 67: 71, 71: 67}      # A <-> T, C <-> G
ACGT = (65, 67, 71, 84)


def consensus(a, qa, b, qb, d, q0=33):
    """(bases, qualities, took_mate1, took_mate2, neither_valid) of one merged pair: the table of the contract, row by row"""
    la, lb = len(a), len(b)
    s = d + lb
    bases, quals = bytearray(), bytearray()
    took1 = took2 = neither = 0
    for x in range(s):
        cov_a, cov_c = x < la, x >= d
        if cov_a:
            ba, ka = a[x], (qa[x] if x < len(qa) else q0)
        if cov_c:
            src = lb - 1 - (x - d)
            bc, kc = COMP.get(b[src], b[src]), (qb[src] if src < len(qb) else q0)
        if cov_a and not cov_c:
            base, q = ba, ka
        elif cov_c and not cov_a:
            base, q = bc, kc
        else:
            assert cov_a and cov_c, "a position of the merged read that neither mate covers"
            va, vc = ba in ACGT, bc in ACGT
            if va and vc and ba == bc:
                base, q = ba, max(ka, kc)
            elif va and vc:
                base = ba if ka >= kc else bc
                took1, took2 = took1 + (ka >= kc), took2 + (ka < kc)
                q = min(q0 + max(2, abs(ka - kc)), 126)
            elif va:
                base, q = ba, ka
            elif vc:
                base, q = bc, kc
            else:
                base, q, neither = ba, min(ka, kc), neither + 1
        bases.append(base)
        quals.append(q)
    return bytes(bases), bytes(quals), took1, took2, neither


def echo(lines, i):
    """what fq-dedup echoes for record i: each line the record has, as text + '\\n'"""
    return b"".join(t + b"\n" for t in lines[4 * i:4 * i + 4])


def _record(lines, i):
    return [lines[4 * i + k] if 4 * i + k < len(lines) else b"" for k in range(4)]


def merge_of(data1, data2=None, params=DEFAULTS, q0=33):
    """data2 = None: data1 is interleaved"""
    params = tuple(params)
    l1 = lines_of(bytes(data1))
    out = dict(lines1=len(l1), lines2=0, reads1=(len(l1) + 3) // 4, reads2=0, input_bytes1=len(data1), input_bytes2=0, min_overlap=params[0],
               max_mismatches=params[1], max_mismatch_pct=params[2], phred_offset=q0)
    if data2 is None:
        pairs = out["reads1"] // 2
        out["unpaired"] = out["reads1"] & 1
        mates = [((l1, 2 * p), (l1, 2 * p + 1)) for p in range(pairs)]
    else:
        l2 = lines_of(bytes(data2))
        out.update(lines2=len(l2), reads2=(len(l2) + 3) // 4, input_bytes2=len(data2))
        pairs = min(out["reads1"], out["reads2"])
        out["unpaired"] = max(out["reads1"], out["reads2"]) - pairs
        mates = [((l1, p), (l2, p)) for p in range(pairs)]
    merged, un1, un2 = [], [], []
    n = dict.fromkeys(("merged_count", "not_overlapped", "too_long", "merged_bases", "overlap_bases", "mismatches", "took_mate1", "took_mate2", "neither_valid"), 0)
    for (la_, i1), (lb_, i2) in mates:
        h, a, _, qa = _record(la_, i1)
        _, b, _, qb = _record(lb_, i2)
        hit = None
        if len(a) > MAX_LEN or len(b) > MAX_LEN:
            n["too_long"] += 1
        else:
            hit = pair_of(a, b, params)
            if hit is None:
                n["not_overlapped"] += 1
        if hit is None:
            un1.append(echo(la_, i1))
            (un1 if data2 is None else un2).append(echo(lb_, i2))
            continue
        d, ov, mm = hit
        bases, quals, t1, t2, nv = consensus(a, qa, b, qb, d, q0)
        assert len(bases) == d + len(b)
        merged.append(h + b"\n" + bases + b"\n+\n" + quals + b"\n")
        assert len(merged[-1]) == len(h) + 2 * len(bases) + 5
        n["merged_count"] += 1
        n["merged_bases"] += len(bases)
        n["overlap_bases"] += ov
        n["mismatches"] += mm
        n["took_mate1"] += t1
        n["took_mate2"] += t2
        n["neither_valid"] += nv
    out.update(n, pairs=pairs)
    return _finish(out, b"".join(merged), b"".join(un1), b"".join(un2))


def _finish(out, merged, un1, un2):
    """the outputs live under OUTPUTS' names, so the count of merged pairs is `merged_pairs` in the dict and `merged` in the stats"""
    out["merged_pairs"] = out.pop("merged_count")
    out.update(merged=merged, unmerged1=un1, unmerged2=un2, merged_bytes=len(merged), unmerged1_bytes=len(un1), unmerged2_bytes=len(un2))
    return out


def stat(want, name):
    """the value of the stats field `name` in a checker's dict"""
    return want["merged_pairs"] if name == "merged" else want[name]


def _gather(arr, start, ln, width, fill):
    """(rows, width) bytes of the texts [start, start + ln) of arr, `fill` behind their ends"""
    y = np.arange(width, dtype=np.int64)[None, :]
    inside = y < ln[:, None]
    pos = np.where(inside, start[:, None] + y, 0)
    return np.where(inside, arr[pos] if arr.size else 0, fill).astype(np.int64)


def merge_of_np(a1, a2=None, params=DEFAULTS, q0=33, chunk=2048):
    params = tuple(params)
    a1 = np.ascontiguousarray(a1, dtype=np.uint8)
    ins = insert_of_np(a1, a2, params)
    out = {k: ins[k] for k in ("reads1", "reads2", "lines1", "lines2", "input_bytes1", "input_bytes2", "pairs", "unpaired", "not_overlapped", "too_long",
                               "min_overlap", "max_mismatches", "max_mismatch_pct")}
    out["phred_offset"] = q0
    pairs, recs = ins["pairs"], ins["recs"]
    arr_b = a1 if a2 is None else np.ascontiguousarray(a2, dtype=np.uint8)
    stride, second = (2, 1) if a2 is None else (1, 0)

    def spans(arr):
        s, e = line_spans_np(arr)
        lines = s.size
        pad = 4 * ((lines + 3) // 4) - lines                 # the lines a last record does not have are empty
        return np.concatenate([s, np.zeros(pad, np.int64)]), np.concatenate([e, np.zeros(pad, np.int64)]), lines

    s1, e1, n1 = spans(a1)
    s2, e2, n2 = (s1, e1, n1) if a2 is None else spans(arr_b)
    i1 = np.arange(pairs, dtype=np.int64) * stride
    i2 = i1 + second
    hit = recs[:, 1] > 0
    m = np.flatnonzero(hit)
    took1 = took2 = neither = bases = 0
    parts = []
    comp = np.arange(256, dtype=np.int64)
    for k, v in COMP.items():
        comp[k] = v
    valid = np.zeros(256, bool)
    valid[list(ACGT)] = True
    for c0 in range(0, m.size, chunk):                       # (a chunk at a time: the arrays below are pairs x positions)
        mc = m[c0:c0 + chunk]
        d = recs[mc, 0]
        sa, la = s1[4 * i1[mc] + 1], e1[4 * i1[mc] + 1] - s1[4 * i1[mc] + 1]
        qa, qla = s1[4 * i1[mc] + 3], np.minimum(e1[4 * i1[mc] + 3] - s1[4 * i1[mc] + 3], la)
        sb, lb = s2[4 * i2[mc] + 1], e2[4 * i2[mc] + 1] - s2[4 * i2[mc] + 1]
        qb, qlb = s2[4 * i2[mc] + 3], np.minimum(e2[4 * i2[mc] + 3] - s2[4 * i2[mc] + 3], lb)
        s = d + lb
        bases += int(s.sum())
        width = int(s.max())
        x = np.arange(width, dtype=np.int64)[None, :]
        inside = x < s[:, None]
        cov_a, cov_c = inside & (x < la[:, None]), inside & (x >= d[:, None])
        A = _gather(a1, sa, la, width, 0)
        QA = _gather(a1, qa, qla, width, q0)
        src = np.where(cov_c, lb[:, None] - 1 - (x - d[:, None]), 0)
        B = np.where(cov_c, arr_b[sb[:, None] + src], 0).astype(np.int64)
        has_q = cov_c & (src < qlb[:, None])
        QC = np.where(has_q, arr_b[np.where(has_q, qb[:, None] + src, 0)], q0).astype(np.int64)
        C = comp[B]
        both = cov_a & cov_c
        va, vc = valid[A], valid[C]
        differ = both & va & vc & (A != C)
        none = both & ~va & ~vc
        a_wins = QA >= QC
        take_c = ~cov_a | (both & vc & (~va | ((A != C) & ~a_wins)))
        base = np.where(take_c, C, A)
        q = np.where(take_c, QC, QA)
        q = np.where(both & va & vc, np.maximum(QA, QC), q)
        q = np.where(differ, np.minimum(q0 + np.maximum(2, np.abs(QA - QC)), 126), q)
        q = np.where(none, np.minimum(QA, QC), q)
        took1, took2, neither = took1 + int((differ & a_wins).sum()), took2 + int((differ & ~a_wins).sum()), neither + int(none.sum())
        hs = s1[4 * i1[mc]]
        hl = e1[4 * i1[mc]] - hs
        base8, q8 = base.astype(np.uint8), q.astype(np.uint8)
        for k in range(mc.size):                             # (one concatenation per merged pair; the consensus above is the work)
            sk = int(s[k])
            parts += [a1[hs[k]:hs[k] + hl[k]].tobytes(), b"\n", base8[k, :sk].tobytes(), b"\n+\n", q8[k, :sk].tobytes(), b"\n"]
    merged = b"".join(parts)

    def echoes(arr, starts, ends, lines, recs_idx):
        parts = []
        for i in recs_idx:
            for j in range(4 * i, min(4 * i + 4, lines)):
                parts += [arr[starts[j]:ends[j]].tobytes(), b"\n"]
        return parts

    u = np.flatnonzero(~hit)
    if a2 is None:
        un1 = b"".join(echoes(a1, s1, e1, n1, np.stack([i1[u], i2[u]], axis=1).reshape(-1).tolist()))
        un2 = b""
    else:
        un1 = b"".join(echoes(a1, s1, e1, n1, i1[u].tolist()))
        un2 = b"".join(echoes(arr_b, s2, e2, n2, i2[u].tolist()))
    out.update(merged_count=int(m.size), merged_bases=bases, overlap_bases=int(recs[m, 1].sum()), mismatches=int(recs[m, 2].sum()),
               took_mate1=took1, took_mate2=took2, neither_valid=neither)
    return _finish(out, merged, un1, un2)


def same(p, q):
    return set(p) == set(q) and all(p[k] == q[k] for k in p)


def assert_stats(s, want, ctx=""):
    """s: a scfq.MergeStats; want: a checker's dict; every field compared with =="""
    assert int(s.struct_size) == 8 * STATS_WORDS and int(s.abi_version) > 0, ctx
    for name in FIELDS:
        assert int(getattr(s, name)) == stat(want, name), (ctx, name, int(getattr(s, name)), stat(want, name))
    assert s.pairs == s.merged + s.not_overlapped + s.too_long, ctx


def stats_text(want):
    """the row of scfq_format_merge_stats_tsv for a checker's dict"""
    from _insert_size_check import div, nimf
    names = ("not_overlapped", "too_long", "unpaired", "merged_bases", "overlap_bases", "mismatches", "took_mate1", "took_mate2", "neither_valid",
             "merged_bytes", "unmerged1_bytes", "unmerged2_bytes")
    return "\t".join([str(want["pairs"]), str(stat(want, "merged")), nimf(div(100 * stat(want, "merged"), want["pairs"]))] + [str(want[k]) for k in names])


STATS_HEADER = ("pairs\tmerged\tpercent_merged\tnot_overlapped\ttoo_long\tunpaired\tmerged_bases\toverlap_bases\tmismatches\ttook_mate1\ttook_mate2\t"
                "neither_valid\tmerged_bytes\tunmerged1_bytes\tunmerged2_bytes")


def with_random_qualities(rng, arr, lo=ord("!"), hi=ord("I")):
    """a copy of the FASTQ in the uint8 array arr (records of four lines) with every quality byte drawn from lo .. hi"""
    out = np.array(arr, dtype=np.uint8, copy=True)
    s, e = line_spans_np(out)
    qs, qe = s[3::4], e[3::4]
    if qs.size:
        ln = qe - qs
        idx = np.repeat(qs, ln) + (np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln, ln))
        out[idx] = rng.integers(lo, hi + 1, idx.size, dtype=np.uint8)
    return out

"""The checker of fq-trim, twice: a plain restatement of the contract in include/sc_fqcount.h, read by read and position by position
(lines as _readstats_check.py has them, d* from _insert_size_check.pair_of), and a numpy form for inputs too large for a Python loop (d*
from insert_of_np, every step on all reads at once).  The two decide the cut points on their own; the records and the statistics are
put together from the cut points by one function.  Both return a dict: out1, out2 — bytes — and every field of scfq_trim_stats but
struct_size and abi_version (adapter_reads: a list of eight)."""
import numpy as np

from _insert_size_check import MAX_LEN, insert_of_np, pair_of
from _readstats_check import line_spans_np, lines_of

STATS_WORDS = 49
INTERLEAVED, NO_OVERLAP, NO_ADAPTERS = 1, 2, 4
DEFAULT_PROBES = (b"AGATCGGAAGAG", b"TGGAATTCTCGG", b"GATCGTCGGACT", b"CTGTCTCTTATA", b"CGCCTTGGCCGT")      # scfq_adapters_default without poly*
DEFAULTS = dict(interleaved=False, no_overlap=False, no_adapters=False, probes=None, min_overlap=30, max_mismatches=5, max_mismatch_pct=20,
                min_adapter_overlap=5, adapter_mismatch_pct=10, poly_g=0, window=4, window_quality=0, min_length=15, phred_offset=33)
PARAM_FIELDS = ("flags", "min_overlap", "max_mismatches", "max_mismatch_pct", "min_adapter_overlap", "adapter_mismatch_pct", "poly_g", "window",
                "window_quality", "min_length", "phred_offset", "n_probes")
FIELDS = ("reads1", "reads2", "lines1", "lines2", "input_bytes1", "input_bytes2", "pairs", "unpaired", "reads_in", "reads_out", "too_long",
          "short_reads", "dropped_reads", "bases_in", "bases_out", "cut_overlap", "cut_adapter", "cut_polyg", "cut_quality", "bases_overlap",
          "bases_adapter", "bases_polyg", "bases_quality", "adapter_reads", "bases_dropped", "overlapped_pairs", "out1_bytes",
          "out2_bytes") + PARAM_FIELDS
STATS_HEADER = ("reads_in\treads_out\tdropped_reads\tshort_reads\ttoo_long\tpairs\tunpaired\toverlapped_pairs\tbases_in\tbases_out\tbases_dropped\t"
                "cut_overlap\tbases_overlap\tcut_adapter\tbases_adapter\tcut_polyg\tbases_polyg\tcut_quality\tbases_quality\tadapter_reads\t"
                "out1_bytes\tout2_bytes")


def resolve(kw):
    """the parameters of a call, the defaults filled in; `probes` as a tuple of bytes"""
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    p = dict(DEFAULTS, **kw)
    if p["no_adapters"]:
        assert not p["probes"]
        p["probes"] = ()
    else:
        p["probes"] = tuple(x.encode() if isinstance(x, str) else bytes(x) for x in (p["probes"] or DEFAULT_PROBES))
    p["flags"] = (INTERLEAVED if p["interleaved"] else 0) | (NO_OVERLAP if p["no_overlap"] else 0) | (NO_ADAPTERS if p["no_adapters"] else 0)
    p["n_probes"] = len(p["probes"])
    return p


def cut_of(S, Q, e, p):
    """steps 2 to 4 on one read that step 1 left at e: (e after adapters, after poly-G, after the window, the probe or None)"""
    probe = None
    for pos in range(e):
        for j, pr in enumerate(p["probes"]):
            t = min(len(pr), e - pos)
            if t < p["min_adapter_overlap"]:
                continue
            mm = sum(1 for k in range(t) if S[pos + k] != pr[k])
            if 100 * mm <= p["adapter_mismatch_pct"] * t:
                probe = j
                break
        if probe is not None:
            e = pos
            break
    e1 = e
    if p["poly_g"]:
        g = 0
        while g < e and S[e - 1 - g] == ord("G"):
            g += 1
        if g >= p["poly_g"]:
            e -= g
    e2 = e
    if p["window_quality"]:
        w, q0 = p["window"], p["phred_offset"]
        q = [(Q[i] - q0 if i < len(Q) else 0) for i in range(e)]
        for pos in range(0, e - w + 1):
            if sum(q[pos:pos + w]) < p["window_quality"] * w:
                e = pos
                break
    return e1, e2, e, probe


def _record(lines, i):
    return [lines[4 * i + k] if 4 * i + k < len(lines) else b"" for k in range(4)]


def _echo(lines, i):
    return b"".join(t + b"\n" for t in lines[4 * i:4 * i + 4])


def _assemble(out, p, units, interleaved):
    """units: per single read or pair a list of reads (texts of the four lines, the echo, L, too_long, e0, e1, e2, e3, probe).  Adds the
    outputs and every statistic to `out`"""
    n = dict.fromkeys(("reads_in", "reads_out", "too_long", "short_reads", "dropped_reads", "bases_in", "bases_out", "cut_overlap", "cut_adapter",
                       "cut_polyg", "cut_quality", "bases_overlap", "bases_adapter", "bases_polyg", "bases_quality", "bases_dropped"), 0)
    reads_per_probe = [0] * 8
    outs = ([], [])
    for unit in units:
        short = [not r["too_long"] and r["e"][3] < p["min_length"] for r in unit]
        drop = any(short)
        for k, r in enumerate(unit):
            L = r["L"]
            e0, e1, e2, e3 = (L, L, L, L) if r["too_long"] else r["e"]
            assert L >= e0 >= e1 >= e2 >= e3 >= 0
            n["reads_in"] += 1
            n["too_long"] += r["too_long"]
            n["short_reads"] += short[k]
            n["bases_in"] += L
            for name, hi, lo in (("overlap", L, e0), ("adapter", e0, e1), ("polyg", e1, e2), ("quality", e2, e3)):
                n["cut_" + name] += lo < hi
                n["bases_" + name] += hi - lo
            if e1 < e0:
                reads_per_probe[r["probe"]] += 1
            if drop:
                n["dropped_reads"] += 1
                n["bases_dropped"] += e3
                continue
            n["reads_out"] += 1
            n["bases_out"] += e3
            if r["too_long"]:
                rec = r["echo"]
            else:
                h, s, plus, q = r["texts"]
                rec = h + b"\n" + s[:e3] + b"\n" + plus + b"\n" + q[:e3] + b"\n"
            outs[0 if (k == 0 or interleaved) else 1].append(rec)
    o1, o2 = b"".join(outs[0]), b"".join(outs[1])
    out.update(n, adapter_reads=reads_per_probe, out1=o1, out2=o2, out1_bytes=len(o1), out2_bytes=len(o2))
    out.update({k: p[k] for k in PARAM_FIELDS})
    return out


def trim_of(data1, data2=None, **kw):
    """data2 = None: data1 is single-end, or interleaved with interleaved=True"""
    p = resolve(kw)
    l1 = lines_of(bytes(data1))
    out = dict(lines1=len(l1), lines2=0, reads1=(len(l1) + 3) // 4, reads2=0, input_bytes1=len(data1), input_bytes2=0, pairs=0, unpaired=0,
               overlapped_pairs=0)
    if data2 is not None:
        assert not p["interleaved"]
        l2 = lines_of(bytes(data2))
        out.update(lines2=len(l2), reads2=(len(l2) + 3) // 4, input_bytes2=len(data2))
        pairs = min(out["reads1"], out["reads2"])
        out.update(pairs=pairs, unpaired=max(out["reads1"], out["reads2"]) - pairs)
        mates = [((l1, i), (l2, i)) for i in range(pairs)]
    elif p["interleaved"]:
        out.update(pairs=out["reads1"] // 2, unpaired=out["reads1"] & 1)
        mates = [((l1, 2 * i), (l1, 2 * i + 1)) for i in range(out["pairs"])]
    else:
        mates = [((l1, i),) for i in range(out["reads1"])]
    units = []
    for unit in mates:
        texts = [_record(ls, i) for ls, i in unit]
        long_ = [len(t[1]) > MAX_LEN for t in texts]
        e0 = [len(t[1]) for t in texts]
        if len(unit) == 2 and not p["no_overlap"] and not any(long_):
            hit = pair_of(texts[0][1], texts[1][1], (p["min_overlap"], p["max_mismatches"], p["max_mismatch_pct"]))
            if hit is not None:
                out["overlapped_pairs"] += 1
                s = hit[0] + len(texts[1][1])
                e0 = [min(v, s) for v in e0]
        reads = []
        for (ls, i), t, tl, e in zip(unit, texts, long_, e0):
            r = dict(texts=t, echo=_echo(ls, i), L=len(t[1]), too_long=tl, probe=None, e=None)
            if not tl:
                e1, e2, e3, r["probe"] = cut_of(t[1], t[3], e, p)
                r["e"] = (e, e1, e2, e3)
            reads.append(r)
        units.append(reads)
    return _assemble(out, p, units, p["interleaved"])


def cuts_np(S, Q, L, LQ, e0, p):
    """steps 2 to 4 on all reads at once.  S, Q: (reads, width) bytes, 0 behind the texts; L, LQ, e0: per read.  Returns e1, e2, e3 and the
    probe (-1: none)"""
    reads, width = S.shape
    pos = np.arange(width, dtype=np.int64)[None, :]
    e = e0.astype(np.int64).copy()
    best = np.full(reads, width + 1, np.int64)
    probe = np.full(reads, -1, np.int64)
    for j, pr in enumerate(p["probes"]):
        m = len(pr)
        pad = np.zeros((reads, width + m), np.uint8)
        pad[:, :width] = S
        mm = np.zeros((reads, width), np.int64)
        for k in range(m):
            mm += (pad[:, k:k + width] != pr[k]) & (pos + k < e[:, None])
        t = np.clip(e[:, None] - pos, 0, m)
        ok = (t >= p["min_adapter_overlap"]) & (100 * mm <= p["adapter_mismatch_pct"] * t)
        first = np.where(ok.any(axis=1), ok.argmax(axis=1), width + 1)
        better = first < best                                 # (a later probe wins only with a smaller p)
        best = np.where(better, first, best)
        probe = np.where(better, j, probe)
    e = np.where(probe >= 0, best, e)
    e1 = e.copy()
    if p["poly_g"]:
        other = (S != ord("G")) & (pos < e[:, None])
        last = np.where(other.any(axis=1), width - 1 - other[:, ::-1].argmax(axis=1), -1)
        g = e - 1 - last
        e = np.where(g >= p["poly_g"], e - g, e)
    e2 = e.copy()
    if p["window_quality"]:
        w = p["window"]
        q = np.where(pos < LQ[:, None], Q.astype(np.int64) - p["phred_offset"], 0)
        E = np.zeros((reads, width + w + 1), np.int64)
        E[:, 1:width + 1] = np.cumsum(q, axis=1)
        E[:, width + 1:] = E[:, width:width + 1]
        sums = E[:, w:w + width] - E[:, :width]
        bad = (pos + w <= e[:, None]) & (sums < p["window_quality"] * w)
        e = np.where(bad.any(axis=1), bad.argmax(axis=1), e)
    return e1, e2, e, probe


def trim_of_np(a1, a2=None, **kw):
    p = resolve(kw)
    a1 = np.ascontiguousarray(a1, dtype=np.uint8)
    paired = a2 is not None or p["interleaved"]
    arrs = [a1] if a2 is None else [a1, np.ascontiguousarray(a2, dtype=np.uint8)]
    spans = []
    for a in arrs:
        s, e = line_spans_np(a)
        lines = int(s.size)
        padn = 4 * ((lines + 3) // 4) - lines                 # the lines a last record does not have are empty
        spans.append((np.concatenate([s, np.zeros(padn, np.int64)]), np.concatenate([e, np.zeros(padn, np.int64)]), lines))
    out = dict(lines1=spans[0][2], lines2=0, reads1=(spans[0][2] + 3) // 4, reads2=0, input_bytes1=int(a1.size), input_bytes2=0, pairs=0, unpaired=0,
               overlapped_pairs=0)
    if a2 is not None:
        assert not p["interleaved"]
        out.update(lines2=spans[1][2], reads2=(spans[1][2] + 3) // 4, input_bytes2=int(arrs[1].size))
        pairs = min(out["reads1"], out["reads2"])
        out.update(pairs=pairs, unpaired=max(out["reads1"], out["reads2"]) - pairs)
        who = [(0, np.arange(pairs, dtype=np.int64)), (1, np.arange(pairs, dtype=np.int64))]
    elif p["interleaved"]:
        pairs = out["reads1"] // 2
        out.update(pairs=pairs, unpaired=out["reads1"] & 1)
        who = [(0, 2 * np.arange(pairs, dtype=np.int64)), (0, 2 * np.arange(pairs, dtype=np.int64) + 1)]
    else:
        who = [(0, np.arange(out["reads1"], dtype=np.int64))]
    # per mate: the spans of the four lines of its records
    mates = []
    for which, idx in who:
        s, e, lines = spans[which]
        mates.append(dict(arr=arrs[which], lines=lines, idx=idx, s=[s[4 * idx + k] for k in range(4)], e=[e[4 * idx + k] for k in range(4)]))
    for m in mates:
        m["L"] = m["e"][1] - m["s"][1]
        m["LQ"] = m["e"][3] - m["s"][3]
        m["too_long"] = m["L"] > MAX_LEN
        m["e0"] = m["L"].copy()
    if paired and not p["no_overlap"] and mates[0]["idx"].size:
        ins = insert_of_np(a1, a2, (p["min_overlap"], p["max_mismatches"], p["max_mismatch_pct"]))
        recs = ins["recs"]
        hit = recs[:, 1] > 0
        out["overlapped_pairs"] = int(hit.sum())
        s = recs[:, 0] + mates[1]["L"]
        for m in mates:
            m["e0"] = np.where(hit, np.minimum(m["L"], s), m["L"])
    for m in mates:
        keep = np.flatnonzero(~m["too_long"])
        width = int(m["L"][keep].max()) if keep.size else 0
        width = max(width, 1)
        y = np.arange(width, dtype=np.int64)[None, :]

        def gather(start, ln):
            inside = y < ln[:, None]
            src = np.where(inside, start[:, None] + y, 0)
            return np.where(inside, m["arr"][src] if m["arr"].size else 0, 0).astype(np.uint8)

        S = gather(m["s"][1][keep], m["L"][keep])
        Q = gather(m["s"][3][keep], np.minimum(m["LQ"], m["L"])[keep])
        e1, e2, e3, probe = cuts_np(S, Q, m["L"][keep], m["LQ"][keep], m["e0"][keep], p)
        m["cuts"] = {int(r): (int(m["e0"][r]), int(a), int(b), int(c), int(j)) for r, a, b, c, j in zip(keep, e1, e2, e3, probe)}
    units = []
    n_units = mates[0]["idx"].size
    for u in range(n_units):
        unit = []
        for m in mates:
            arr, i = m["arr"], int(m["idx"][u])
            texts = [arr[m["s"][k][u]:m["e"][k][u]].tobytes() for k in range(4)]
            echo = b"".join(t + b"\n" for k, t in enumerate(texts) if 4 * i + k < m["lines"])
            r = dict(texts=texts, echo=echo, L=int(m["L"][u]), too_long=bool(m["too_long"][u]), probe=None, e=None)
            if not r["too_long"]:
                c = m["cuts"][u]
                r["e"], r["probe"] = c[:4], (c[4] if c[4] >= 0 else None)
            unit.append(r)
        units.append(unit)
    return _assemble(out, p, units, p["interleaved"])


def same(p, q):
    return set(p) == set(q) and all(p[k] == q[k] for k in p)


def check_identities(w):
    assert w["reads_in"] == w["reads_out"] + w["dropped_reads"]
    assert w["bases_in"] == w["bases_out"] + w["bases_overlap"] + w["bases_adapter"] + w["bases_polyg"] + w["bases_quality"] + w["bases_dropped"]
    assert sum(w["adapter_reads"]) == w["cut_adapter"]


def assert_stats(s, want, ctx=""):
    """s: a scfq.TrimStats; want: a checker's dict; every field compared with =="""
    assert int(s.struct_size) == 8 * STATS_WORDS and int(s.abi_version) > 0, ctx
    for name in FIELDS:
        got = list(s.adapter_reads) if name == "adapter_reads" else int(getattr(s, name))
        assert got == want[name], (ctx, name, got, want[name])
    check_identities({name: (list(s.adapter_reads) if name == "adapter_reads" else int(getattr(s, name))) for name in FIELDS})


def stats_text(w):
    """the row of scfq_format_trim_stats_tsv for a checker's dict"""
    names = ("reads_in", "reads_out", "dropped_reads", "short_reads", "too_long", "pairs", "unpaired", "overlapped_pairs", "bases_in", "bases_out",
             "bases_dropped", "cut_overlap", "bases_overlap", "cut_adapter", "bases_adapter", "cut_polyg", "bases_polyg", "cut_quality", "bases_quality")
    per_probe = ",".join(str(v) for v in w["adapter_reads"][:w["n_probes"]]) or "-"
    return "\t".join([str(w[k]) for k in names] + [per_probe, str(w["out1_bytes"]), str(w["out2_bytes"])])

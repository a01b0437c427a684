"""fq-rmdup restated in plain Python (include/sc_fqcount.h has the definition): a dictionary from a unit's key to the first unit that has
it.  Nothing of the device's hash is in here, so `collisions` and `rounds` are not restated: they are the two values that depend on it.
rmdup_of is what every test compares with ==; classes_by_pairs states the definition once more by comparing all pairs of units."""
from _readstats_check import lines_of

STATS_WORDS = 26
HIST_BINS = 1025
INTERLEAVED, SWAPPED = 1, 2
DEFAULTS = dict(interleaved=False, swapped=False, prefix=0)
FIELDS = ("reads1", "reads2", "lines1", "lines2", "input_bytes1", "input_bytes2", "pairs", "unpaired", "units_in", "units_out", "reads_in", "reads_out",
          "duplicate_units", "duplicated_classes", "max_copies", "bases_in", "bases_out", "out1_bytes", "out2_bytes", "flags", "prefix")
HASH_FIELDS = ("collisions", "rounds", "hash_bits")      # not restated
REPORT_FIELDS = ("units_in", "units_out", "duplicate_units", "duplicate_pct", "duplicated_classes", "max_copies", "reads_in", "reads_out", "pairs", "unpaired",
                 "bases_in", "bases_out", "out1_bytes", "out2_bytes")
STATS_HEADER = "\t".join(REPORT_FIELDS)
REC_HEADER = "unit\trep\tcopies"
HIST_HEADER = "copies\tclasses\tunits"


def resolve(kw):
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    p = dict(DEFAULTS, **kw)
    assert 0 <= p["prefix"] <= 65535
    p["flags"] = (INTERLEAVED if p["interleaved"] else 0) | (SWAPPED if p["swapped"] else 0)
    return p


def key_of(S, prefix=0):
    """the key of a read: the compared bytes, which carry their length"""
    return bytes(S[:prefix]) if prefix else bytes(S)


def unit_key(keys, swapped=False):
    """what two units have in common iff they are equal: the keys in order, or as an unordered pair"""
    return tuple(sorted(keys)) if swapped and len(keys) == 2 else tuple(keys)


def units_equal(x, y, swapped=False):
    """the definition, on two tuples of keys"""
    if len(x) == 1:
        return x[0] == y[0]
    return (x[0] == y[0] and x[1] == y[1]) or (swapped and x[0] == y[1] and x[1] == y[0])


def classes_of(keys, swapped=False):
    """keys: per unit a tuple of one or two keys.  Returns the table [(rep, copies)] by a dictionary from key to first unit"""
    first, rep = {}, []
    for u, k in enumerate(keys):
        rep.append(first.setdefault(unit_key(k, swapped), u))
    copies = [0] * len(keys)
    for r in rep:
        copies[r] += 1
    return [(r, copies[u] if r == u else 0) for u, r in enumerate(rep)]


def classes_by_pairs(keys, swapped=False):
    """the same table from the definition alone: the representative of a unit is the first unit it equals"""
    rep = [next(v for v in range(u + 1) if units_equal(keys[v], k, swapped)) for u, k in enumerate(keys)]
    return [(r, rep.count(u) if r == u else 0) for u, r in enumerate(rep)]


def _record(lines, i):
    return [lines[4 * i + k] if 4 * i + k < len(lines) else b"" for k in range(4)]


def _echo(lines, i):
    return b"".join(t + b"\n" for t in lines[4 * i:4 * i + 4])


def rmdup_of(data1, data2=None, **kw):
    """data2 = None: data1 is single-end, or interleaved with interleaved=True"""
    p = resolve(kw)
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
        assert not p["swapped"]
        units = [((l1, i),) for i in range(out["reads1"])]
    seqs = [tuple(_record(ls, i)[1] for ls, i in unit) for unit in units]
    recs = classes_of([tuple(key_of(S, p["prefix"]) for S in unit) for unit in seqs], p["swapped"])
    hist, outs = [0] * HIST_BINS, ([], [])
    n = dict(units_in=len(units), units_out=0, reads_in=sum(len(u) for u in units), reads_out=0, duplicated_classes=0, max_copies=0,
             bases_in=sum(len(S) for unit in seqs for S in unit), bases_out=0)
    for u, (unit, (rep, copies)) in enumerate(zip(units, recs)):
        if rep != u:
            continue
        n["units_out"] += 1
        n["reads_out"] += len(unit)
        n["duplicated_classes"] += copies >= 2
        n["max_copies"] = max(n["max_copies"], copies)
        n["bases_out"] += sum(len(S) for S in seqs[u])
        hist[min(copies, HIST_BINS - 1)] += 1
        for k, (ls, i) in enumerate(unit):
            outs[0 if (k == 0 or p["interleaved"]) else 1].append(_echo(ls, i))
    n["duplicate_units"] = n["units_in"] - n["units_out"]
    o1, o2 = b"".join(outs[0]), b"".join(outs[1])
    out.update(n, recs=recs, hist=hist, out1=o1, out2=o2, out1_bytes=len(o1), out2_bytes=len(o2), flags=p["flags"], prefix=p["prefix"])
    return out


def check_identities(w, hist=None, recs=None):
    assert w["units_in"] == w["units_out"] + w["duplicate_units"] and w["bases_out"] <= w["bases_in"]
    assert w["duplicated_classes"] <= w["units_out"] and w["duplicated_classes"] <= w["duplicate_units"]
    assert w["max_copies"] <= w["units_in"] and (w["max_copies"] >= 1) == (w["units_in"] >= 1)
    if hist is not None:
        assert len(hist) == HIST_BINS and hist[0] == 0 and sum(hist) == w["units_out"] and sum(hist[2:]) == w["duplicated_classes"]
    if recs is not None:
        assert len(recs) == w["units_in"] and sum(c for _, c in recs) == w["units_in"]
        assert all((r == u) == (c > 0) and r <= u for u, (r, c) in enumerate(recs))


def assert_stats(s, want, ctx=""):
    """s: a scfq.RmdupStats; want: a checker's dict; every field but the hash's compared with =="""
    assert int(s.struct_size) == 8 * STATS_WORDS and int(s.abi_version) > 0, ctx
    for name in FIELDS:
        assert int(getattr(s, name)) == want[name], (ctx, name, int(getattr(s, name)), want[name])
    check_identities({name: int(getattr(s, name)) for name in FIELDS})


def pct_text(dup, units):
    """floor(10000 dup / units) as X.YY, in integers"""
    q = 10000 * dup // units if units else 0
    return "%d.%02d" % (q // 100, q % 100)


def stats_text(w):
    """the row of scfq_format_rmdup_stats_tsv for a checker's dict"""
    return "\t".join(pct_text(w["duplicate_units"], w["units_in"]) if k == "duplicate_pct" else str(w[k]) for k in REPORT_FIELDS)


def rec_text(unit, rec):
    """the row of scfq_format_rmdup_rec_tsv"""
    return "%d\t%d\t%d" % (unit, rec[0], rec[1])


def per_read_text(w, header=False):
    rows = [REC_HEADER] if header else []
    rows += [rec_text(u, r) for u, r in enumerate(w["recs"])]
    return "".join(r + "\n" for r in rows)


def hist_text(w, header=False):
    """the rows of `sc fq-rmdup --hist`: every class size that occurs, the classes of 1024 and more in a last row"""
    rows = [HIST_HEADER] if header else []
    rows += ["%d\t%d\t%d" % (c, v, c * v) for c, v in enumerate(w["hist"][:HIST_BINS - 1]) if v]
    if w["hist"][HIST_BINS - 1]:
        rows.append("1024+\t%d\t%d" % (w["hist"][HIST_BINS - 1], sum(c for _, c in w["recs"] if c >= HIST_BINS - 1)))
    return "".join(r + "\n" for r in rows)

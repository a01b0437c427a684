"""The checker of fq-normalize: the definitions of include/sc_fqcount.h restated in plain Python over a table {key: count} as
_kcount_check.kcount_of returns it: the counts of a read's windows, the record of a read (k-mers, lower median, minimum, weak), the
rule of a unit with its hash, the outputs, the statistics, the histogram and the report texts.  Every comparison is ==."""
from _kmers_check import CODE
from _readstats_check import lines_of
from _screen_check import _layout

INTERLEAVED, KEEP_NO_KMERS = 1, 2
CANONICAL = 1
MAX_DEPTH = 2 ** 32 - 2
MASK64 = 2 ** 64 - 1
GOLDEN = 0x9E3779B97F4A7C15
EARG, EHIP, EFULL = -5, -3, -10
KEPT, NO_KMERS, LOW, HIGH = 0, 1, 2, 3
FIELDS = ("reads1", "reads2", "lines1", "lines2", "input_bytes1", "input_bytes2", "pairs", "unpaired", "units_in", "units_out", "reads_in",
          "reads_out", "dropped_no_kmers", "dropped_low", "dropped_high", "short_reads", "bases_in", "bases_out", "windows", "kmers", "skipped",
          "weak_kmers", "absent_kmers", "out1_bytes", "out2_bytes", "flags", "k", "table_flags", "target", "min_depth", "weak_below", "seed",
          "distinct")
ROW_FIELDS = ("units_in", "units_out", "reads_in", "reads_out", "dropped_no_kmers", "dropped_low", "dropped_high", "bases_in", "bases_out", "kmers",
              "skipped", "weak_kmers", "absent_kmers", "k", "target", "min_depth")
ROW_HEADER = "\t".join(ROW_FIELDS)
HIST_HEADER = "depth\tunits_in\tunits_out"
STATS_WORDS = 37


def mix64(x):
    """MurmurHash3's 64-bit finalizer"""
    x ^= x >> 33
    x = x * 0xFF51AFD7ED558CCD & MASK64
    x ^= x >> 33
    x = x * 0xC4CEB9FE1A85EC53 & MASK64
    x ^= x >> 33
    return x


def counts_of(S, table, k, canonical):
    """the saturated counts of the k-mers of the text S, in window order (skipped windows have no entry)"""
    out = []
    fw = rc = run = 0
    full = 4 ** k - 1
    for b in S:
        if b not in CODE:
            run = 0
            continue
        c = CODE[b]
        fw = (4 * fw + c) & full
        rc = (rc >> 2) | ((3 - c) << (2 * (k - 1)))
        run += 1
        if run >= k:
            out.append(min(table.get(min(fw, rc) if canonical else fw, 0), MAX_DEPTH))
    return out


def record_of(counts, weak_below=2):
    """(kmers, depth, min_count, weak) of a read"""
    if not counts:
        return (0, 0, 0, 0)
    return (len(counts), sorted(counts)[(len(counts) - 1) // 2], min(counts), sum(1 for c in counts if c < weak_below))


def classify(mates, u, target=0, min_depth=0, seed=0):
    """mates: [(kmers, depth)] of the unit; returns (class, D)"""
    depths = [d for kmers, d in mates if kmers > 0]
    if not depths:
        return NO_KMERS, 0
    D = min(depths)
    if D < min_depth:
        return LOW, D
    if target > 0 and D > target:
        r = mix64(seed ^ (u * GOLDEN & MASK64)) >> 32
        if (r * D) >> 32 >= target:
            return HIGH, D
    return KEPT, D


def normalize_of(table, k, canonical, data1, data2=None, interleaved=False, keep_no_kmers=False, target=0, min_depth=0, weak_below=2, seed=0,
                 bins=0):
    """data2 = None: data1 is single-end, or interleaved with interleaved=True.  Returns a dict: the statistics, recs, out1, out2, hist"""
    assert not (interleaved and data2 is not None)
    ls = [lines_of(bytes(data1))] + ([lines_of(bytes(data2))] if data2 is not None else [])
    out, who = _layout(len(ls[0]), len(ls[1]) if data2 is not None else 0, interleaved, data2 is not None)
    out.update(input_bytes1=len(data1), input_bytes2=len(data2) if data2 is not None else 0)
    n = dict.fromkeys(("units_in", "units_out", "reads_in", "reads_out", "dropped_no_kmers", "dropped_low", "dropped_high", "short_reads", "bases_in",
                       "bases_out", "windows", "kmers", "skipped", "weak_kmers", "absent_kmers"), 0)
    outs, recs, classes = ([], []), [], []
    hist = [[0, 0] for _ in range(bins)]
    for u, unit in enumerate(who):
        mates = []
        for which, i in unit:
            lines = ls[which]
            S = lines[4 * i + 1] if 4 * i + 1 < len(lines) else b""
            counts = counts_of(S, table, k, canonical)
            rec = record_of(counts, weak_below)
            recs.append(rec)
            windows = max(0, len(S) - k + 1)
            n["reads_in"] += 1
            n["short_reads"] += len(S) < k
            n["bases_in"] += len(S)
            n["windows"] += windows
            n["kmers"] += rec[0]
            n["skipped"] += windows - rec[0]
            n["weak_kmers"] += rec[3]
            n["absent_kmers"] += sum(1 for c in counts if c == 0)
            mates.append((len(S), b"".join(t + b"\n" for t in lines[4 * i:4 * i + 4])))
        cls, D = classify([r[:2] for r in recs[-len(unit):]], u, target, min_depth, seed)
        kept = cls == KEPT or (cls == NO_KMERS and keep_no_kmers)
        classes.append(cls)
        n["units_in"] += 1
        n["units_out"] += kept
        n["dropped_no_kmers"] += cls == NO_KMERS and not kept
        n["dropped_low"] += cls == LOW
        n["dropped_high"] += cls == HIGH
        if bins and cls != NO_KMERS:
            hist[min(D, bins - 1)][0] += 1
            hist[min(D, bins - 1)][1] += kept
        if kept:
            for m, (L, echo) in enumerate(mates):
                n["reads_out"] += 1
                n["bases_out"] += L
                outs[0 if (m == 0 or interleaved) else 1].append(echo)
    o1, o2 = b"".join(outs[0]), b"".join(outs[1])
    out.update(n, out1=o1, out2=o2, out1_bytes=len(o1), out2_bytes=len(o2), recs=recs, classes=classes, hist=hist)
    out.update(flags=(INTERLEAVED if interleaved else 0) | (KEEP_NO_KMERS if keep_no_kmers else 0), k=k, table_flags=CANONICAL if canonical else 0,
               target=target, min_depth=min_depth, weak_below=weak_below, seed=seed, distinct=len(table))
    check_identities(out)
    return out


def check_identities(w):
    assert w["windows"] == w["kmers"] + w["skipped"]
    assert w["units_in"] == w["units_out"] + w["dropped_no_kmers"] + w["dropped_low"] + w["dropped_high"]


def stats_dict(s):
    return {name: int(getattr(s, name)) for name in FIELDS}


def assert_stats(s, want, ctx=""):
    """s: a scfq.NormStats; want: normalize_of's dict; every field but the two diagnostics of the table compared with =="""
    assert int(s.struct_size) == 8 * STATS_WORDS and int(s.abi_version) > 0, ctx
    got = stats_dict(s)
    for name in FIELDS:
        assert got[name] == want[name], (ctx, name, got[name], want[name])
    check_identities(got)
    assert int(s.passes) >= 1 and int(s.slots) >= 1024 and int(s.slots) & (int(s.slots) - 1) == 0, (ctx, int(s.passes), int(s.slots))


def recs_list(recs):
    """a ctypes array of scfq.NormRec (or a numpy array of shape (n, 4)) as the checker's list of tuples"""
    if hasattr(recs, "tolist"):
        return [tuple(r) for r in recs.tolist()]
    return [(r.kmers, r.depth, r.min_count, r.weak) for r in recs]


def report_row(w):
    return "\t".join(str(w[f]) for f in ROW_FIELDS)


def hist_rows(hist):
    return ["%d\t%d\t%d" % (d, a, b) for d, (a, b) in enumerate(hist)]


def per_read_rows(w):
    return ["%d\t%d\t%d\t%d\t%d" % ((i,) + r) for i, r in enumerate(w["recs"])]

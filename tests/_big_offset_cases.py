"""Inputs whose byte offsets pass 2^32, and what the record pipelines owe for them.

An input is filler + tail with filler = block x R.  The block is whole records (whole pairs for the paired commands) of about 0.6 MB
from the generators the pipelines' own tests use; its length B is odd and no multiple of 3, so repetition r starts at every residue
mod 16 and mod 4096 over the run and the bytes at 2^31 and 2^32 fall inside records at places nobody chose.  R is the smallest count
with R * B >= 2^32 + 2^22.  The tail is a few hundred records of another shape with the pipeline's planted cases; all of it lies
beyond 2^32.

The expectation is never computed on the whole input: it is the checker's result on the block and on the tail, composed.  Counters,
histograms and tables add up (R * block + tail); per-record rows and outputs are the block's R times, then the tail's (`Tiled`);
what a checker derives at its end (N50, the median insert, ...) is derived again from the composed rows by the checker's own code.
A k-mer table is merged key by key; fq-demux's outputs are tiled destination by destination; under fq-normalize's sampled rule the
class of a unit depends on its number in the whole input and is computed again for all of them (compose_normalize_sampled).
tests/test_big_offset_cases_host.py proves every composition against the checker on block x 3 + tail."""
import numpy as np

from _adapters_check import adapters_of_np
from _cycles_check import table_of_np
from _insert_size_check import DEFAULTS as INSERT_DEFAULTS, _finish as insert_finish, insert_of_np, planted, paired_block, random_dna, revcomp
from _demux_check import demux_of as demux_check_of
from _kcount_check import Want as KcountWant, kcount_of_np
from _kmers_check import kmers_of_np
from _normalize_check import GOLDEN as NORM_GOLDEN, HIGH as NORM_HIGH, KEPT as NORM_KEPT, LOW as NORM_LOW, NO_KMERS as NORM_NO_KMERS, \
    normalize_of as normalize_check_of
from _merge_check import merge_of_np, with_random_qualities
from _readstats_check import line_spans_np, per_read_np
from _screen_check import PARAM_FIELDS as SCREEN_PARAMS, PER_REF, screen_of_np
from _trim_check import PARAM_FIELDS as TRIM_PARAMS, trim_of_np

LIMIT = 2 ** 32 + 2 ** 22
MARKS = (2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32)                          # the bytes whose repetitions `layout` names
CUTS = (2 ** 31 - 1, 2 ** 31 + 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1)         # lengths at which the same buffer is run again
LONG_ADAPTER = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCACGATCTCGTATGCCGTCTTCTGCTTG"  # (test_gpu_trim.py's)
TRIM_ALL = dict(poly_g=5, window_quality=20)                                  # every step on (test_gpu_trim.py's ALL)
SCREEN_KW = dict(min_hits=3)
FIELD = 8                                                                      # hex digits of the repetition number in a header
DEMUX_SAMPLES = (("s0", "ACGTACGT", "TTGACCAG"), ("s1", "GGATCCTA", "CATGGTCA"), ("s2", "TCAGGACT", "AGCTTGTC"), ("s3", "CTTCAGAC", "GTCAAGGT"),
                 ("s4", "TAGCTTGA", "CCATGACT"))          # dual barcodes of 8 + 8 letters, any two at least 4 letters apart in either
DEMUX_KW = dict(mismatches=1)


def layout(B, tail_len, R=None):
    """the facts of an input of block length B: R (given for the second file of a pair, which repeats as often as the first), the
    lengths, and for every byte of MARKS the repetition that holds it"""
    assert B % 2 == 1 and B % 3 != 0, B
    if R is None:
        R = -(-LIMIT // B)
    assert R * B >= LIMIT
    return dict(B=B, R=R, filler=R * B, n=R * B + tail_len, tail_at=R * B, marks={m: m // B for m in MARKS})


def lengthen(block, at):
    """(block with 'x' bytes put in at `at` — inside its first header — until its length is odd and no multiple of 3, how many)"""
    a = np.asarray(block, np.uint8)
    add = 0
    while (a.size + add) % 2 == 0 or (a.size + add) % 3 == 0:
        add += 1
    return np.concatenate([a[:at], np.full(add, ord("x"), np.uint8), a[at:]]), add


def as_u8(data):
    return np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data


class Tiled:
    """`block` R times, then `tail`: bytes, or arrays of rows.  step: what repetition r adds to its rows (r * step; line offsets), the
    tail's get R * step"""

    def __init__(self, block, R, tail, step=0):
        if not isinstance(block, bytes):
            block, tail = np.asarray(block), np.asarray(tail)
            assert block.shape[1:] == tail.shape[1:] and block.dtype == tail.dtype, (block.shape, tail.shape)
        self.block, self.R, self.tail, self.step = block, R, tail, step

    def __len__(self):
        return self.R * len(self.block) + len(self.tail)

    def whole(self):
        if isinstance(self.block, bytes):
            return self.block * self.R + self.tail
        reps = np.tile(self.block, (self.R,) + (1,) * (self.block.ndim - 1))
        tail = self.tail
        if self.step:
            assert self.block.ndim == 1
            reps = reps + np.repeat(np.arange(self.R, dtype=self.block.dtype) * self.block.dtype.type(self.step), len(self.block))
            tail = tail + self.block.dtype.type(self.R * self.step)
        return np.concatenate([reps, tail])


def _added(b, t, R):
    if isinstance(b, np.ndarray):                     # tables of positions: the shorter one has nothing at the other's last rows
        top = max(b.shape[0], t.shape[0])
        out = np.zeros((top,) + b.shape[1:], b.dtype)
        out[:b.shape[0]] += b * b.dtype.type(R)
        out[:t.shape[0]] += t
        return out
    if isinstance(b, (list, tuple)):
        return [R * x + y for x, y in zip(b, t)]
    assert isinstance(b, int) and not isinstance(b, bool), type(b)
    return R * b + t


def compose(block, tail, R, same=(), longest=(), tiled=()):
    """the checker's dict for block x R + tail from its dicts for the block and for the tail: fields of `same` are parameters, those
    of `longest` maxima, those of `tiled` rows or outputs; every other field adds up"""
    assert set(block) == set(tail), set(block) ^ set(tail)
    out = {}
    for k, b in block.items():
        t = tail[k]
        if k in same:
            assert b == t, (k, b, t)
            out[k] = b
        elif k in longest:
            out[k] = max(b, t)
        elif k in tiled:
            out[k] = Tiled(b, R, t)
        else:
            out[k] = _added(b, t, R)
    return out


def whole(want):
    """a composed dict with every Tiled field written out"""
    return {k: v.whole() if isinstance(v, Tiled) else v for k, v in want.items()}


def equal(p, q):
    """two written-out dicts, compared exactly, field by field; returns the names that differ"""
    bad = sorted(set(p) ^ set(q))
    for k in set(p) & set(q):
        a, b = p[k], q[k]
        if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
            a, b = np.asarray(a), np.asarray(b)
            ok = a.shape == b.shape and bool((a == b).all())
        else:
            ok = isinstance(a, bytes) == isinstance(b, bytes) and a == b
        if not ok:
            bad.append(k)
    return bad


# ---- the pipelines: the checker as a dict, and how two of its dicts compose ---------------------------------------------------

def index_of(a):
    """line_off of scfq_index_lines for an input that ends with '\\n' or is cut anywhere: every line start, then the sentinel"""
    a = as_u8(a)
    nl = np.flatnonzero(a == 10).astype(np.int64)
    starts = np.concatenate([np.zeros(1, np.int64), nl + 1])
    if a.size and a[-1] != 10:
        starts = np.concatenate([starts, np.array([a.size + 1], np.int64)])      # the implied final '\n'
    return dict(lines=int(starts.size - 1), off=starts)


def compose_index(block, tail, R, B):
    """the block ends with '\\n': its sentinel is the next repetition's first line"""
    assert int(block["off"][-1]) == B
    return dict(lines=R * block["lines"] + tail["lines"], off=Tiled(block["off"][:-1], R, tail["off"], step=B))


def readstats_of(a):
    rows, lines = per_read_np(as_u8(a))
    return dict(rows=rows, lines=lines, input_bytes=int(as_u8(a).size))


def compose_readstats(block, tail, R):
    """(the summary is summary_of over the rows written out: _readstats_check.assert_summary does that)"""
    return compose(block, tail, R, tiled=("rows",))


def cycles_of(a):
    table, lines, ms, mq = table_of_np(as_u8(a))
    return dict(table=table, lines=lines, max_seq_len=ms, max_qual_len=mq, input_bytes=int(as_u8(a).size))


def compose_cycles(block, tail, R):
    return compose(block, tail, R, longest=("max_seq_len", "max_qual_len"))


def kmers_of(a, k, canonical):
    table, windows, kmers, skipped, short, lines = kmers_of_np(as_u8(a), k, canonical, dense=True)
    return dict(table=table, windows=windows, kmers=kmers, skipped=skipped, short_lines=short, lines=lines, input_bytes=int(as_u8(a).size))


def compose_kmers(block, tail, R):
    """(distinct and max_count are read off the composed table by _kmers_check.assert_result)"""
    return compose(block, tail, R)


def kmers_tuple(w):
    return w["table"], w["windows"], w["kmers"], w["skipped"], w["short_lines"], w["lines"]


def adapters_of(a, probes):
    rows, hits, total, max_len, lines = adapters_of_np(as_u8(a), probes)
    return dict(rows=rows, hits=list(hits), total=list(total), max_seq_len=max_len, lines=lines, input_bytes=int(as_u8(a).size))


def compose_adapters(block, tail, R):
    return compose(block, tail, R, longest=("max_seq_len",))


def adapters_tuple(w):
    return w["rows"], w["hits"], w["total"], w["max_seq_len"], w["lines"]


INSERT_HEAD = ("lines1", "lines2", "reads1", "reads2", "input_bytes1", "input_bytes2", "unpaired")


def _seq_lengths(a, reads):
    s, e = line_spans_np(as_u8(a))
    ln = np.zeros(reads, np.int64)
    k = s[1::4].size
    ln[:k] = e[1::4] - s[1::4]
    return ln


def insert_of(a1, a2=None, params=INSERT_DEFAULTS):
    """insert_of_np's dict, and the lengths of the mates that its finishing code needs"""
    w = insert_of_np(as_u8(a1), None if a2 is None else as_u8(a2), params)
    l1 = _seq_lengths(a1, w["reads1"])
    if a2 is None:
        w["la"], w["lb"] = l1[0:2 * w["pairs"]:2], l1[1:2 * w["pairs"]:2]
    else:
        w["la"], w["lb"] = l1[:w["pairs"]], _seq_lengths(a2, w["reads2"])[:w["pairs"]]
    return w


def compose_insert(block, tail, R):
    """the counts of the inputs add up, the records are tiled, and _insert_size_check._finish makes the histogram, the sums, min, median,
    mode and max from the records written out, as it does for the checker.  (Whole pairs in the block: the pairing starts afresh.)"""
    assert block["unpaired"] == 0 and (block["reads2"] == 0 or block["reads1"] == block["reads2"])
    params = (block["min_overlap"], block["max_mismatches"], block["max_mismatch_pct"])
    assert params == (tail["min_overlap"], tail["max_mismatches"], tail["max_mismatch_pct"])
    rows = {k: Tiled(block[k], R, tail[k]) for k in ("recs", "la", "lb")}
    out = {k: R * block[k] + tail[k] for k in INSERT_HEAD}
    insert_finish(out, rows["recs"].whole(), rows["la"].whole(), rows["lb"].whole(), params)
    out.update(rows)
    return out


MERGE_PARAMS = ("min_overlap", "max_mismatches", "max_mismatch_pct", "phred_offset")
MERGE_OUTPUTS = ("merged", "unmerged1", "unmerged2")


def merge_of(a1, a2=None):
    return merge_of_np(as_u8(a1), None if a2 is None else as_u8(a2))


def compose_merge(block, tail, R):
    return compose(block, tail, R, same=MERGE_PARAMS, tiled=MERGE_OUTPUTS)


def trim_of(a1, a2=None, **kw):
    return trim_of_np(as_u8(a1), None if a2 is None else as_u8(a2), **kw)


def compose_trim(block, tail, R):
    return compose(block, tail, R, same=TRIM_PARAMS, tiled=("out1", "out2"))


def screen_of(index, a1, a2=None, **kw):
    w = screen_of_np(index, as_u8(a1), None if a2 is None else as_u8(a2), **kw)
    w["recs"] = np.array(w["recs"], np.int64).reshape(-1, 5)
    return w


def compose_screen(block, tail, R):
    """(ref_best_reads and ref_only_reads — "best" and "alone" — count decisions made read by read: they add up like the rest)"""
    assert set(PER_REF) <= set(block)
    return compose(block, tail, R, same=SCREEN_PARAMS, tiled=("out1", "out2", "recs"))


KCOUNT_SUMS = ("windows", "kmers", "skipped", "short_lines", "lines", "reads", "input_bytes")


def kcount_of(a1, a2, k, canonical):
    w = kcount_of_np([as_u8(a1)] + ([as_u8(a2)] if a2 is not None else []), k, canonical)
    return dict({f: getattr(w, f) for f in KCOUNT_SUMS}, table=w.table)


def compose_kcount(block, tail, R):
    """the table is merged key by key (R * the block's count + the tail's), the sums add up.  (distinct, unique and max_count are read
    off the merged table by _kcount_check.Want: see kcount_want)"""
    table = {key: R * c for key, c in block["table"].items()}
    for key, c in tail["table"].items():
        table[key] = table.get(key, 0) + c
    return dict({f: R * block[f] + tail[f] for f in KCOUNT_SUMS}, table=table)


def kcount_want(w):
    """a (composed) dict as the _kcount_check.Want that assert_summary, dump_of and hist_of take"""
    return KcountWant(w["table"], *[w[f] for f in KCOUNT_SUMS])


def _record_bytes(a):
    """the byte length of every record of an input of whole records"""
    a = as_u8(a)
    off = index_of(a)["off"]
    assert (off.size - 1) % 4 == 0 and (a.size == 0 or a[-1] == 10)
    return np.diff(off[::4])


def _unit_sums(per_read1, per_read2, units, two):
    """per-unit sums of a per-read quantity, for out1 and out2: both mates of an interleaved unit go to out1"""
    if two:
        return per_read1[:units], per_read2[:units]
    return per_read1[0:2 * units:2] + per_read1[1:2 * units:2], np.zeros(units, np.int64)


DEMUX_SAME = ("flags", "mismatches", "n_samples", "dual")
DEMUX_ROW_SUMS = ("units", "perfect", "mismatched", "bases_out", "bytes1", "bytes2")


def demux_of(a1, a2=None, samples=DEMUX_SAMPLES, **kw):
    w = demux_check_of(as_u8(a1).tobytes(), None if a2 is None else as_u8(a2).tobytes(), list(samples), **kw)
    w["recs"] = np.array(w["recs"], np.int64).reshape(-1, 4)
    return w


def _dest_slice(w, which, d):
    row = w["rows"][d]
    return w["out" + which][row["off" + which]:row["off" + which] + row["bytes" + which]]


def compose_demux(block, tail, R):
    """counters and the rows' counts add up, off1 / off2 are the running sums of the composed bytes, the per-unit table is tiled.  An
    output is ordered by destination: out1 / out2 come back as one Tiled per destination — the block's slice R times, then the tail's —
    and are never written out here"""
    assert block["unpaired"] == 0 and set(block) == set(tail)
    out = {}
    for k, b in block.items():
        if k in DEMUX_SAME:
            assert b == tail[k], (k, b, tail[k])
            out[k] = b
        elif k not in ("rows", "recs", "out1", "out2"):
            out[k] = R * b + tail[k]
    rows, off1, off2 = [], 0, 0
    for rb, rt in zip(block["rows"], tail["rows"]):
        row = {f: R * rb[f] + rt[f] for f in DEMUX_ROW_SUMS}
        row["off1"], row["off2"] = off1, off2
        off1, off2 = off1 + row["bytes1"], off2 + row["bytes2"]
        rows.append(row)
    assert (off1, off2) == (out["out1_bytes"], out["out2_bytes"])
    out["rows"], out["recs"] = rows, Tiled(block["recs"], R, tail["recs"])
    for which in "12":
        out["out" + which] = [Tiled(_dest_slice(block, which, d), R, _dest_slice(tail, which, d)) for d in range(len(rows))]
    return out


def demux_R(block):
    """the repetitions after which the block's last destination (undetermined) starts beyond LIMIT in every output it has"""
    last = block["rows"][-1]
    return -(-LIMIT // min(last["off" + w] for w in "12" if block["out%s_bytes" % w]))


NORM_SAME = ("flags", "k", "table_flags", "target", "min_depth", "weak_below", "seed", "distinct")
NORM_TILED = ("recs", "out1", "out2", "classes", "len1", "len2", "bases")
NORM_RULE = ("units_out", "reads_out", "dropped_no_kmers", "dropped_low", "dropped_high", "bases_out", "out1_bytes", "out2_bytes")
NORM_SAMPLED = dict(target=3, min_depth=2, seed=77)


def normalize_of(table, k, canonical, a1, a2=None, **kw):
    """normalize_of's dict with recs as an int64 array of shape (reads, 4), classes and hist as arrays, and per unit the bytes it has in
    out1 and out2 when kept (len1, len2) and its bases: inputs of whole pairs, and no '\\r'"""
    a1, a2 = as_u8(a1), None if a2 is None else as_u8(a2)
    w = normalize_check_of(table, k, canonical, a1.tobytes(), None if a2 is None else a2.tobytes(), **kw)
    w["recs"] = np.array(w["recs"], np.int64).reshape(-1, 4)
    w["classes"] = np.array(w["classes"], np.uint8)
    w["hist"] = np.array(w["hist"], np.int64).reshape(-1, 2)
    two, units = a2 is not None, w["units_in"]
    assert w["unpaired"] == 0 and w["reads_in"] == 2 * units and 13 not in a1
    second = a2 if two else np.zeros(0, np.uint8)
    w["len1"], w["len2"] = _unit_sums(_record_bytes(a1), _record_bytes(second), units, two)
    s1, s2 = _unit_sums(_seq_lengths(a1, w["reads1"]), _seq_lengths(second, w["reads2"]), units, two)
    w["bases"] = s1 + s2
    return w


def compose_normalize(block, tail, R):
    """a rule that does not hash the unit number (target = 0), for a fixed table: counters and the histogram add up"""
    assert block["target"] == 0
    return compose(block, tail, R, same=NORM_SAME, tiled=NORM_TILED)


def mix64_np(x):
    """_normalize_check.mix64 over a uint64 array (products wrap)"""
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xFF51AFD7ED558CCD)
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xC4CEB9FE1A85EC53)
    return x ^ (x >> np.uint64(33))


def classify_np(kmers1, depth1, kmers2, depth2, u, target=0, min_depth=0, seed=0):
    """_normalize_check.classify for arrays of units of two mates with the numbers u: (class, D)"""
    u = np.asarray(u).astype(np.uint64)
    has1, has2 = np.asarray(kmers1) > 0, np.asarray(kmers2) > 0
    none = ~(has1 | has2)
    far = np.int64(2 ** 62)
    D = np.minimum(np.where(has1, np.asarray(depth1, np.int64), far), np.where(has2, np.asarray(depth2, np.int64), far))
    D[none] = 0
    cls = np.full(u.shape, NORM_KEPT, np.uint8)
    low = ~none & (D < min_depth)
    cls[low] = NORM_LOW
    cls[none] = NORM_NO_KMERS
    if target > 0:
        r = mix64_np(np.full(u.shape, seed, np.uint64) ^ (u * np.uint64(NORM_GOLDEN))) >> np.uint64(32)
        high = ~none & ~low & (D > target) & (((r * D.astype(np.uint64)) >> np.uint64(32)) >= np.uint64(target))
        cls[high] = NORM_HIGH
    return cls, D


def compose_normalize_sampled(block, tail, R, target, min_depth, seed, keep_no_kmers=False, u=None):
    """a rule that hashes the unit number (target > 0), for a fixed table; block and tail are normalize_of's dicts under any rule.  What a
    read is (recs, the counters of the reads) is tiled or adds up; the class of every unit is found again for its number in the whole
    input — r * U_block + i in the filler, R * U_block + j in the tail (u: other numbers, to show that they matter) —, and the kept
    units give the other counters, the histogram and the output sizes.  The outputs are described: `kept` (uint8, per unit) and the
    bytes a kept unit has in them (len1, len2)"""
    assert set(block) == set(tail)
    Ub, Ut = len(block["classes"]), len(tail["classes"])
    units = R * Ub + Ut
    out = {}
    for k, b in block.items():
        if k in ("k", "table_flags", "weak_below", "distinct"):
            assert b == tail[k], (k, b, tail[k])
            out[k] = b
        elif k not in NORM_SAME + NORM_TILED + NORM_RULE + ("hist",):
            out[k] = R * b + tail[k]
    assert out["units_in"] == units

    def per_unit(f):
        return np.concatenate([np.tile(f(block), R), f(tail)])

    mates = [per_unit(lambda w, m=m, j=j: w["recs"][m::2, j]) for m in (0, 1) for j in (0, 1)]
    cls, D = classify_np(*mates, np.arange(units, dtype=np.uint64) if u is None else u, target, min_depth, seed)
    kept = (cls == NORM_KEPT) | ((cls == NORM_NO_KMERS) & bool(keep_no_kmers))
    rows = {f: Tiled(block[f], R, tail[f]) for f in ("recs", "len1", "len2", "bases")}
    len1, len2, bases = (rows[f].whole() for f in ("len1", "len2", "bases"))
    out.update(units_out=int(kept.sum()), reads_out=2 * int(kept.sum()), dropped_no_kmers=int(((cls == NORM_NO_KMERS) & ~kept).sum()),
               dropped_low=int((cls == NORM_LOW).sum()), dropped_high=int((cls == NORM_HIGH).sum()), bases_out=int(bases[kept].sum()),
               out1_bytes=int(len1[kept].sum()), out2_bytes=int(len2[kept].sum()), target=target, min_depth=min_depth, seed=seed,
               flags=(block["flags"] & 1) | (2 if keep_no_kmers else 0))
    bins = block["hist"].shape[0]
    hist = np.zeros((bins, 2), np.int64)
    if bins:
        seen = cls != NORM_NO_KMERS
        hist[:, 0] = np.bincount(np.minimum(D[seen], bins - 1), minlength=bins)
        hist[:, 1] = np.bincount(np.minimum(D[seen & kept], bins - 1), minlength=bins)
    out.update(rows, hist=hist, classes=cls, kept=kept.astype(np.uint8))
    return out


def cut_of(checker, composer, block, n, **kw):
    """what is owed for the first n bytes of block x R: n // B whole repetitions, then the checker on the block cut at n % B"""
    block = as_u8(block)
    q, c = divmod(n, block.size)
    assert c > 0
    return composer(checker(block), checker(block[:c]), q, **kw)


# ---- the inputs ---------------------------------------------------------------------------------------------------------------

def _header_starts(a):
    nl = np.flatnonzero(a == 10)
    return np.concatenate([[0], nl[3::4] + 1])[:nl.size // 4]


def _plant(rng, a, probes, every):
    """a probe written over the sequence of every `every`-th record at a random place (cut by the read's end or whole)"""
    s, e = line_spans_np(a)
    for i in range(0, s.size // 4, every):
        lo, hi = int(s[4 * i + 1]), int(e[4 * i + 1])
        p = probes[(i // every) % len(probes)]
        at = int(rng.integers(lo, max(lo + 1, hi - 3)))
        w = min(len(p), hi - at)
        if w > 0:
            a[at:at + w] = np.frombuffer(p[:w], np.uint8)


def single_block(rng, probes, records=1500):
    """(block, fields): make_fastq records; every header carries FIELD hex digits at fields[i] (all '0' here) behind its '@'"""
    from test_gpu_hist_spec import make_fastq
    a = make_fastq(rng, records, read_len=(120, 260), header_len=(24, 60)).copy()
    _plant(rng, a, probes, 9)
    heads = _header_starts(a)
    assert heads.size == records
    for h in heads:
        a[h + 1:h + 1 + FIELD] = ord("0")
    a, add = lengthen(a, 1 + FIELD)
    fields = heads + 1
    fields[1:] += add
    assert len({bytes(a[h - 1:h + 23]) for h in fields}) == records, "the block's headers must differ in their first 24 bytes"
    return a, fields


def header_with(block, fields, i, rep):
    """the header line of record i of the block as repetition `rep` holds it (without the '\\n')"""
    at = int(fields[i]) - 1
    end = at + int(np.flatnonzero(block[at:at + 4096] == 10)[0])
    h = bytearray(block[at:end].tobytes())
    h[1:1 + FIELD] = b"%08x" % rep
    return bytes(h)


def single_tail(rng, probes, block, fields, dup_reps, records=300):
    """short reads under short or borrowed headers.  Every fifth record carries the header of a record of the filler — of the
    repetitions dup_reps in turn —, one fresh header comes twice; the rest are fresh"""
    seqs, quals, names = [], [], []
    q_alpha = np.frombuffer(b"FFFFFFFF:,#I5?", np.uint8)
    for i in range(records):
        ln = int(rng.integers(1, 90)) if i % 17 else 0
        seqs.append(bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), ln, p=[.29, .2, .2, .29, .02])))
        quals.append(bytes(rng.choice(q_alpha, ln)))
        if i % 5 == 2:
            rep = dup_reps[(i // 5) % len(dup_reps)]
            names.append(header_with(block, fields, int(rng.integers(0, fields.size)), rep)[1:])
        elif i == 101:
            names.append(names[11])
        else:
            names.append(b"tail:%d/%d" % (i, i * i))
    a = np.frombuffer(b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in zip(names, seqs, quals)), np.uint8).copy()
    _plant(rng, a, probes, 7)
    return a


def dedup_of(block, fields, R, tail):
    """fq-dedup of block x R + tail, the repetition number written into every header of the filler: the filler comes out verbatim (all
    its headers differ), then the tail's first occurrences — by set membership over the header texts.
    Returns (records of the tail that come out, as bytes; total_reads, duplicates, records_out, bytes_out)"""
    zeroed = {header_with(block, fields, i, 0) for i in range(fields.size)}
    assert len(zeroed) == fields.size
    lines = tail.tobytes().split(b"\n")[:-1]
    seen, kept, dups = set(), [], 0
    for i in range(0, len(lines), 4):
        h = lines[i]
        digits = h[1:1 + FIELD]
        in_filler = False
        if len(digits) == FIELD and all(c in b"0123456789abcdef" for c in digits):
            in_filler = int(digits, 16) < R and (h[:1] + b"0" * FIELD + h[1 + FIELD:]) in zeroed
        if in_filler or h in seen:
            dups += 1
            continue
        seen.add(h)
        kept.append(b"".join(x + b"\n" for x in lines[i:i + 4]))
    out = b"".join(kept)
    records = R * fields.size + len(lines) // 4
    return out, dict(total_reads=records, duplicates=dups, records_out=records - dups, bytes_out=R * block.size + len(out))


def numbered(block, fields, R):
    """block x R on the host with the repetition numbers written in (small R: what the device does by one indexed assignment)"""
    a = np.tile(block, R).reshape(R, block.size)
    for r in range(R):
        for f in fields:
            a[r, f:f + FIELD] = np.frombuffer(b"%08x" % r, np.uint8)
    return a.reshape(-1)


def _ref_reads(rng, refs, ln):
    text = refs[int(rng.integers(0, len(refs)))]
    at = int(rng.integers(0, len(text) - ln))
    return text[at:at + ln]


def _paired_rows(rng, refs, pairs, la, lb):
    """paired_blocks' records as two arrays of `pairs` rows: "@p\n" S "\n+\n" Q "\n", one length per file"""
    r1, r2 = paired_block(rng, pairs, la, lb)
    r1, r2 = with_random_qualities(rng, r1, 33 + 22, 33 + 40), with_random_qualities(rng, r2, 33 + 22, 33 + 40)
    for a, ln in ((r1.reshape(pairs, -1), la), (r2.reshape(pairs, -1), lb)):     # quality that falls at a random place in every fifth read
        for k in range(2, pairs, 5):
            at = int(rng.integers(0, ln))
            a[k, 6 + ln + at:6 + 2 * ln] = rng.integers(33 + 2, 33 + 13, ln - at, dtype=np.uint8)
    a1, a2 = r1.reshape(pairs, -1), r2.reshape(pairs, -1)
    for k in range(0, pairs, 7):
        at = int(rng.integers(20, la))
        a1[k, 3 + at:3 + la] = np.frombuffer((LONG_ADAPTER + b"A" * la)[:la - at], np.uint8)
    for k in range(3, pairs, 11):
        g = int(rng.integers(5, 40))
        a2[k, 3 + lb - g:3 + lb] = ord("G")
    for k in range(5, pairs, 13):
        a1[k, 6 + la:6 + 2 * la] = ord("I")
        a2[k, 6 + lb:6 + 2 * lb] = ord("I")
    for k in range(1, pairs, 10):
        frag = _ref_reads(rng, refs, la + 60)
        a1[k, 3:3 + la] = np.frombuffer(frag[:la], np.uint8)
        a2[k, 3:3 + lb] = np.frombuffer(revcomp(frag)[:lb], np.uint8)
    return a1, a2


def _three_blocks(a1, a2):
    il = np.concatenate([a1, a2], axis=1).reshape(-1)
    return lengthen(a1.reshape(-1), 2)[0], lengthen(a2.reshape(-1), 2)[0], lengthen(il, 2)[0]


def paired_blocks(rng, refs, pairs=1900, la=150, lb=140):
    """(r1, r2, interleaved): paired_block's pairs with random qualities and the planted cases of test_gpu_trim.py — adapters in mate 1,
    G tails in mate 2, quality that stays high —, and every 10th pair drawn from the screen's references.  Three blocks of
    different lengths"""
    return _three_blocks(*_paired_rows(rng, refs, pairs, la, lb))


TAIL_LENGTHS = (0, 1, 29, 30, 31, 63, 64, 65, 100, 127, 128, 129, 250, 511, 512, 513)


def _tail_mates(rng, refs):
    m1, m2 = [], []
    for la in TAIL_LENGTHS:
        for lb in TAIL_LENGTHS:
            ins = (max(la, lb) + 20, min(la, lb) - 7, 40)[(la + lb) % 3]
            if la and lb and 0 < ins < la + lb and la <= 512 and lb <= 512:
                a, b = planted(rng, la, lb, ins)
            else:
                a, b = random_dna(rng, la), random_dna(rng, lb)
            m1.append(a), m2.append(b)
    for i in range(40):
        frag = _ref_reads(rng, refs, 90 + i)
        ln = 60 + 2 * i
        a, b = frag[:ln], revcomp(frag)[:ln]
        if ln > len(frag):                                    # a fragment shorter than the reads: both run into the adapter
            a, b = (frag + LONG_ADAPTER)[:ln], (revcomp(frag) + LONG_ADAPTER)[:ln]
        m1.append(a), m2.append(b)
    return m1, m2


def _tail_files(rng, m1, m2):
    def fq(mates, tag):
        return b"".join(b"@t%d/%s\n" % (i, tag) + s + b"\n+\n" + (rng.integers(15, 41, len(s)) + 33).astype(np.uint8).tobytes() + b"\n"
                        for i, s in enumerate(mates))

    r1, r2 = fq(m1, b"1"), fq(m2, b"2")

    def records(data):
        lines = data.split(b"\n")[:-1]
        return [b"".join(x + b"\n" for x in lines[k:k + 4]) for k in range(0, len(lines), 4)]

    il = b"".join(x for pair in zip(records(r1), records(r2)) for x in pair)
    return as_u8(r1), as_u8(r2), as_u8(il)


def paired_tails(rng, refs):
    """(r1, r2, interleaved): pairs of many lengths — fragments shorter than, as long as and longer than the reads, mates too long for
    the overlap search, empty ones, reads of the references, adapters behind short fragments"""
    return _tail_files(rng, *_tail_mates(rng, refs))


def _barcode(rng, samples, s1, s2):
    """the barcodes of a random sample over the first letters of both mates (mutable, at least as long as the barcodes): one pair in 8
    keeps its letters, about one in 10 of the others gets one substituted letter, one in 20 an N"""
    if rng.random() < 1 / 8:
        return
    _, b1, b2 = samples[int(rng.integers(len(samples)))]
    codes = [bytearray(b1.encode()), bytearray(b2.encode())]
    y = rng.random()
    if y < 0.15:
        c = codes[int(rng.integers(2))]
        at = int(rng.integers(len(c)))
        c[at] = ord("N") if y >= 0.10 else [x for x in b"ACGT" if x != c[at]][int(rng.integers(3))]
    s1[:len(codes[0])] = list(codes[0])
    s2[:len(codes[1])] = list(codes[1])


def barcoded_blocks(rng, refs, samples=DEMUX_SAMPLES, pairs=1900, la=147, lb=145):
    """(r1, r2, interleaved): paired_blocks' three blocks, of other lengths, with the samples' barcodes written over the first letters of
    both mates: roughly equal shares for the samples, one pair in 8 undetermined"""
    a1, a2 = _paired_rows(rng, refs, pairs, la, lb)
    for u in range(pairs):
        _barcode(rng, samples, a1[u, 3:3 + la], a2[u, 3:3 + lb])
    return _three_blocks(a1, a2)


def barcoded_tails(rng, refs, samples=DEMUX_SAMPLES):
    """(r1, r2, interleaved): paired_tails' pairs, barcodes over those whose mates are both long enough; the lengths 0 and 1 stay
    shorter than every barcode"""
    m1, m2 = _tail_mates(rng, refs)
    need1, need2 = max(len(s[1]) for s in samples), max(len(s[2]) for s in samples)
    for i, (a, b) in enumerate(zip(m1, m2)):
        if len(a) >= need1 and len(b) >= need2:
            a, b = bytearray(a), bytearray(b)
            _barcode(rng, samples, a, b)
            m1[i], m2[i] = bytes(a), bytes(b)
    return _tail_files(rng, m1, m2)


TABLES_PAIR_SEED, BARCODED_SEED = 20261023, 20261024


def tables_pair_data(refs):
    """(blocks, tails) of the paired input that tests/test_gpu_big_offsets_tables.py gives fq-kcount and fq-normalize"""
    rng = np.random.default_rng(TABLES_PAIR_SEED)
    return paired_blocks(rng, refs), paired_tails(rng, refs)


def barcoded_data(refs):
    """(blocks, tails) of the input that tests/test_gpu_big_offsets_tables.py gives fq-demux"""
    rng = np.random.default_rng(BARCODED_SEED)
    return barcoded_blocks(rng, refs), barcoded_tails(rng, refs)


def normalize_counted(b1, b2, t1, t2):
    """the input whose k-mers fq-normalize's given table counts: the records of both blocks once, those of every 4th pair three more
    times, those of every 9th pair eight more times, then both tails.  Depths 1, 4, 9 and 12 where the mates do not overlap"""
    parts = []
    for b in (b1, b2):
        off = index_of(b)["off"]
        recs = [b[off[4 * i]:off[4 * i + 4]] for i in range((off.size - 1) // 4)]
        parts += recs + recs[::4] * 3 + recs[::9] * 8
    return np.concatenate(parts + [as_u8(t1), as_u8(t2)])


FA_ALPHABET = np.frombuffer(b"ACGTACGTACGTACGTACGT", np.uint8)
FA_CONTIGS = ((b"a", 200_003, 60), (b"b", 150_000, 70), (b"c", 100_000, 61), (b"d", 99_991, 80), (b"e", 64, 64), (b"f", 50_001, 100))


def fasta_block(rng, contigs=FA_CONTIGS):
    """(block, fields, names): contigs of different line widths, the third with lower case, N runs and IUPAC letters; every name is
    a letter and FIELD hex digits (all '0' here)"""
    out, fields, at = [], [], 0
    for k, (name, length, width) in enumerate(contigs):
        head = b">" + name + b"0" * FIELD + b" contig %d\n" % k
        fields.append(at + 1 + len(name))
        s = rng.choice(FA_ALPHABET, length)
        if k == 2:
            s = rng.choice(np.frombuffer(b"ACGTacgtacgtNNnRYKMSWryk", np.uint8), length)
            for _ in range(length // 300):
                p = int(rng.integers(0, length - 50))
                s[p:p + int(rng.integers(1, 40))] = ord("N")
        s = s.tobytes()
        body = b"".join(s[i:i + width] + b"\n" for i in range(0, length, width))
        out += [head, body]
        at += len(head) + len(body)
    a = as_u8(b"".join(out)).copy()
    first_nl = int(np.flatnonzero(a == 10)[0])
    a, add = lengthen(a, first_nl)                            # behind the first header's text: the name stays
    fields = np.array(fields, np.int64)
    fields[1:] += add
    return a, fields, [c[0] for c in contigs]


def fasta_tail(rng):
    a, _, _ = fasta_block(rng, ((b"tail-x", 3_001, 50), (b"tail-y", 777, 777), (b"tail-z", 20_000, 33)))
    return a


def fasta_intervals(rng, model, first_contig, per_contig=6):
    """(contig, begin, end) rows over the contigs of `model`, numbered from first_contig: inside one line, across many lines, from the
    contig's start, to its end, the whole contig, an empty interval"""
    q = []
    for j, (_, _, _, length) in enumerate(model.contigs):
        a = int(rng.integers(0, max(1, length - 40)))
        picks = [(a, min(length, a + 7)), (a, min(length, a + int(rng.integers(1, length + 1)))), (0, min(length, 1 + a)), (a, length), (0, length),
                 (a, a)]
        q += [(first_contig + j, lo, hi) for lo, hi in picks[:per_contig]]
    return q

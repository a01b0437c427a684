"""The checker of fq-screen, twice: a plain restatement of the contract in include/sc_fqcount.h — a dict from canonical key to mask, then
read by read and window by window — and a numpy form for inputs too large for a Python loop (every window of the whole input at once,
membership by a sorted key array).  The two find the hits on their own; decisions, outputs and statistics are put together from the
per-read hits by one function.  index_of / index_of_np return a dict: k, names, keys (dict key -> mask), refs (a dict per reference:
contigs, bases, windows, kmers, distinct, shared), distinct, slots.  screen_of / screen_of_np return a dict: out1, out2 — bytes —, recs — a
list of (kmers, hit_kmers, best_hits, mask, best) per read — and every field of scfq_screen_stats but struct_size and abi_version."""
import numpy as np

from _readstats_check import line_spans_np, lines_of

STATS_WORDS = 94
MAX_REFS, MAX_K, MAX_REF_BASES = 16, 32, 1 << 27
INTERLEAVED, KEEP_MATCHED = 1, 2
CODE = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3}
REF_FIELDS = ("contigs", "bases", "windows", "kmers", "distinct", "shared")
PER_REF = ("ref_reads", "ref_only_reads", "ref_best_reads", "ref_kmer_hits")
PARAM_FIELDS = ("flags", "min_hits", "min_hit_pct", "k", "n_refs")
FIELDS = ("reads1", "reads2", "lines1", "lines2", "input_bytes1", "input_bytes2", "pairs", "unpaired", "reads_in", "reads_out", "dropped_reads",
          "matched_reads", "matched_pairs", "multi_reads", "short_reads", "bases_in", "bases_out", "windows", "kmers", "skipped", "hit_kmers") + \
    PER_REF + ("out1_bytes", "out2_bytes") + PARAM_FIELDS
REPORT_HEADER = "ref\tref_bases\tref_kmers\treads_in\treads\tpct_reads\tonly_reads\tbest_reads\tkmer_hits"
PER_READ_HEADER = "read_index\tkmers\thit_kmers\tbest\tbest_hits\tmask"


def key_of(kmer):
    """the canonical index of k bytes that are all A C G T"""
    k = len(kmer)
    fwd = 0
    for b in kmer:
        fwd = (fwd << 2) | CODE[b]
    rc = 0
    for j, b in enumerate(kmer):
        rc |= (3 - CODE[b]) << (2 * j)
    assert fwd < (1 << (2 * k)) and rc < (1 << (2 * k))
    return min(fwd, rc)


def contigs_of(text):
    """the contigs of a FASTA text: sequence bytes 0x21 .. 0x7E, upper-cased; a header line is a line whose first byte is '>'"""
    contigs, cur = [], None
    for line in bytes(text).split(b"\n"):
        if line[:1] == b">":
            if cur is not None:
                contigs.append(bytes(cur))
            cur = bytearray()
            continue
        seq = bytes(b for b in line if 0x21 <= b <= 0x7E).upper()
        if seq and cur is None:
            cur = bytearray()
        if seq:
            cur += seq
    if cur is not None:
        contigs.append(bytes(cur))
    return contigs


def slots_of(windows):
    s = 1024
    while s < 2 * windows:
        s *= 2
    return s


def _finish_index(k, names, per_ref_keys, refs):
    keys = {}
    for r, ks in enumerate(per_ref_keys):
        for key in ks:
            keys[key] = keys.get(key, 0) | (1 << r)
    for r, info in enumerate(refs):
        info["distinct"] = sum(1 for m in keys.values() if m >> r & 1)
        info["shared"] = sum(1 for m in keys.values() if m >> r & 1 and m != 1 << r)
    return dict(k=k, names=list(names), keys=keys, refs=refs, distinct=len(keys), slots=slots_of(sum(i["windows"] for i in refs)))


def index_of(refs, k=31):
    """refs: a list of (name, FASTA text)"""
    assert 8 <= k <= MAX_K and 1 <= len(refs) <= MAX_REFS
    per_ref, infos = [], []
    for name, text in refs:
        cs = contigs_of(text)
        info = dict(contigs=len(cs), bases=sum(len(c) for c in cs), windows=0, kmers=0)
        assert info["bases"] > 0, "an empty reference"
        ks = set()
        for c in cs:
            for p in range(len(c) - k + 1):
                info["windows"] += 1
                w = c[p:p + k]
                if all(b in CODE for b in w):
                    info["kmers"] += 1
                    ks.add(key_of(w))
        per_ref.append(ks)
        infos.append(info)
    return _finish_index(k, [n for n, _ in refs], per_ref, infos)


def windows_np(a, k):
    """for the uint8 array a: (key, valid) of the window at every position p with p + k <= a.size — valid iff its k bytes are exactly A C G T"""
    n = a.size
    m = max(n - k + 1, 0)
    code = np.full(256, 4, np.uint8)
    for b, c in CODE.items():
        code[b] = c
    c = code[a]
    bad = np.concatenate([np.zeros(1, np.int64), np.cumsum(c == 4)])
    valid = (bad[k:k + m] - bad[:m]) == 0 if m else np.zeros(0, bool)
    c = (c & 3).astype(np.uint64)
    fwd = np.zeros(m, np.uint64)
    rc = np.zeros(m, np.uint64)
    for j in range(k):
        fwd = (fwd << np.uint64(2)) | c[j:j + m]              # (k = 32: the top bits fall off only after all 32 are in)
        rc |= (np.uint64(3) - c[j:j + m]) << np.uint64(2 * j)
    return np.minimum(fwd, rc), valid


def index_of_np(refs, k=31):
    per_ref, infos = [], []
    for name, text in refs:
        cs = contigs_of(text)
        info = dict(contigs=len(cs), bases=sum(len(c) for c in cs), windows=0, kmers=0)
        assert info["bases"] > 0, "an empty reference"
        ks = set()
        for c in cs:
            key, valid = windows_np(np.frombuffer(c, np.uint8), k)
            info["windows"] += int(key.size)
            info["kmers"] += int(valid.sum())
            ks.update(int(x) for x in np.unique(key[valid]))
        per_ref.append(ks)
        infos.append(info)
    return _finish_index(k, [n for n, _ in refs], per_ref, infos)


def hits_of(S, index):
    """(kmers, hit_kmers, hits per reference) of one sequence text"""
    k, keys = index["k"], index["keys"]
    kmers = hit = 0
    hits = [0] * MAX_REFS
    for p in range(len(S) - k + 1):
        w = S[p:p + k]
        if not all(b in CODE for b in w):
            continue
        kmers += 1
        m = keys.get(key_of(w), 0)
        hit += m != 0
        for r in range(MAX_REFS):
            hits[r] += m >> r & 1
    return kmers, hit, hits


def decide(kmers, hits, min_hits, min_hit_pct):
    """(mask, best, best_hits)"""
    mask, best, best_hits = 0, 0xFF, 0
    for r, h in enumerate(hits):
        if h >= max(1, min_hits) and 100 * h >= min_hit_pct * kmers:
            mask |= 1 << r
            if h > best_hits:
                best, best_hits = r, h
    return mask, best, best_hits


def _layout(n_lines1, n_lines2, interleaved, two):
    """the counts of the inputs and, per unit, its reads as (input, record)"""
    out = dict(lines1=n_lines1, lines2=n_lines2, reads1=(n_lines1 + 3) // 4, reads2=(n_lines2 + 3) // 4, pairs=0, unpaired=0)
    if two:
        pairs = min(out["reads1"], out["reads2"])
        out.update(pairs=pairs, unpaired=max(out["reads1"], out["reads2"]) - pairs)
        units = [((0, i), (1, i)) for i in range(pairs)]
    elif interleaved:
        out.update(pairs=out["reads1"] // 2, unpaired=out["reads1"] & 1)
        units = [((0, 2 * i), (0, 2 * i + 1)) for i in range(out["pairs"])]
    else:
        units = [((0, i),) for i in range(out["reads1"])]
    return out, units


def _assemble(out, index, units, per_read, p):
    """units: per unit its reads as (L, echo); per_read: (kmers, hit_kmers, hits) in the order of the reads"""
    k = index["k"]
    n = dict.fromkeys(("reads_in", "reads_out", "dropped_reads", "matched_reads", "matched_pairs", "multi_reads", "short_reads", "bases_in", "bases_out",
                       "windows", "kmers", "skipped", "hit_kmers"), 0)
    per_ref = {f: [0] * MAX_REFS for f in PER_REF}
    outs, recs = ([], []), []
    at = 0
    for unit in units:
        decided = []
        for L, echo in unit:
            kmers, hit, hits = per_read[at]
            at += 1
            mask, best, best_hits = decide(kmers, hits, p["min_hits"], p["min_hit_pct"])
            decided.append(mask)
            recs.append((kmers, hit, best_hits, mask, best))
            windows = max(0, L - k + 1)
            n["reads_in"] += 1
            n["matched_reads"] += mask != 0
            n["multi_reads"] += bin(mask).count("1") >= 2
            n["short_reads"] += L < k
            n["bases_in"] += L
            n["windows"] += windows
            n["kmers"] += kmers
            n["skipped"] += windows - kmers
            n["hit_kmers"] += hit
            for r in range(MAX_REFS):
                per_ref["ref_reads"][r] += mask >> r & 1
                per_ref["ref_only_reads"][r] += mask == 1 << r
                per_ref["ref_best_reads"][r] += best == r
                per_ref["ref_kmer_hits"][r] += hits[r]
        matched = any(decided)
        n["matched_pairs"] += matched and len(unit) == 2
        if matched != p["keep_matched"]:
            n["dropped_reads"] += len(unit)
            continue
        for m, (L, echo) in enumerate(unit):
            n["reads_out"] += 1
            n["bases_out"] += L
            outs[0 if (m == 0 or p["interleaved"]) else 1].append(echo)
    o1, o2 = b"".join(outs[0]), b"".join(outs[1])
    out.update(n, out1=o1, out2=o2, out1_bytes=len(o1), out2_bytes=len(o2), recs=recs, **per_ref)
    out.update(flags=(INTERLEAVED if p["interleaved"] else 0) | (KEEP_MATCHED if p["keep_matched"] else 0), min_hits=p["min_hits"],
               min_hit_pct=p["min_hit_pct"], k=k, n_refs=len(index["names"]))
    return out


def _params(kw):
    p = dict(interleaved=False, keep_matched=False, min_hits=1, min_hit_pct=0)
    assert not set(kw) - set(p), kw
    p.update(kw)
    assert 1 <= p["min_hits"] <= 65535 and 0 <= p["min_hit_pct"] <= 100
    return p


def screen_of(index, data1, data2=None, **kw):
    """data2 = None: data1 is single-end, or interleaved with interleaved=True"""
    p = _params(kw)
    assert not (p["interleaved"] and data2 is not None)
    ls = [lines_of(bytes(data1))] + ([lines_of(bytes(data2))] if data2 is not None else [])
    out, who = _layout(len(ls[0]), len(ls[1]) if data2 is not None else 0, p["interleaved"], data2 is not None)
    out.update(input_bytes1=len(data1), input_bytes2=len(data2) if data2 is not None else 0)
    units, per_read = [], []
    for unit in who:
        reads = []
        for which, i in unit:
            lines = ls[which]
            S = lines[4 * i + 1] if 4 * i + 1 < len(lines) else b""
            reads.append((len(S), b"".join(t + b"\n" for t in lines[4 * i:4 * i + 4])))
            per_read.append(hits_of(S, index))
        units.append(reads)
    return _assemble(out, index, units, per_read, p)


def screen_of_np(index, a1, a2=None, **kw):
    p = _params(kw)
    assert not (p["interleaved"] and a2 is not None)
    k = index["k"]
    arrs = [np.ascontiguousarray(a1, dtype=np.uint8)] + ([np.ascontiguousarray(a2, dtype=np.uint8)] if a2 is not None else [])
    table = np.array(sorted(index["keys"]), dtype=np.uint64)
    masks = np.array([index["keys"][int(x)] for x in table], dtype=np.int64)
    per_input = []
    for a in arrs:
        s, e = line_spans_np(a)
        lines = int(s.size)
        reads = (lines + 3) // 4
        padn = 4 * reads - lines
        s, e = np.concatenate([s, np.zeros(padn, np.int64)]), np.concatenate([e, np.zeros(padn, np.int64)])
        ss, se = s[1::4], e[1::4]
        key, valid = windows_np(a, k)
        # a window belongs to the read whose sequence text holds all of it
        owner = np.full(key.size, -1, np.int64)
        for i in range(reads):
            if se[i] - ss[i] >= k:
                owner[ss[i]:se[i] - k + 1] = i
        use = valid & (owner >= 0)
        own, kk = owner[use], key[use]
        at = np.searchsorted(table, kk)
        found = (at < table.size) & (table[np.minimum(at, max(table.size - 1, 0))] == kk) if table.size else np.zeros(kk.size, bool)
        m = np.where(found, masks[np.minimum(at, max(table.size - 1, 0))] if table.size else 0, 0)
        kmers = np.bincount(own, minlength=reads)
        hit = np.bincount(own[found], minlength=reads)
        hits = np.stack([np.bincount(own[(m >> r & 1) == 1], minlength=reads) for r in range(MAX_REFS)], axis=1) if reads else np.zeros((0, MAX_REFS), np.int64)
        per_input.append(dict(a=a, lines=lines, s=s, e=e, L=se - ss, kmers=kmers, hit=hit, hits=hits))
    out, who = _layout(per_input[0]["lines"], per_input[1]["lines"] if a2 is not None else 0, p["interleaved"], a2 is not None)
    out.update(input_bytes1=int(arrs[0].size), input_bytes2=int(arrs[1].size) if a2 is not None else 0)
    units, per_read = [], []
    for unit in who:
        reads = []
        for which, i in unit:
            d = per_input[which]
            echo = b"".join(d["a"][d["s"][j]:d["e"][j]].tobytes() + b"\n" for j in range(4 * i, min(4 * i + 4, d["lines"])))
            reads.append((int(d["L"][i]), echo))
            per_read.append((int(d["kmers"][i]), int(d["hit"][i]), [int(x) for x in d["hits"][i]]))
        units.append(reads)
    return _assemble(out, index, units, per_read, p)


def same(p, q):
    return set(p) == set(q) and all(p[k] == q[k] for k in p)


def check_identities(w):
    assert w["windows"] == w["kmers"] + w["skipped"]
    assert w["reads_in"] == w["reads_out"] + w["dropped_reads"]
    assert sum(w["ref_best_reads"]) == w["matched_reads"]
    assert sum(w["ref_only_reads"]) + w["multi_reads"] == w["matched_reads"]


def stats_dict(s):
    return {name: (list(getattr(s, name)) if name in PER_REF else int(getattr(s, name))) for name in FIELDS}


def assert_stats(s, want, ctx=""):
    """s: a scfq.ScreenStats; want: a checker's dict; every field compared with =="""
    assert int(s.struct_size) == 8 * STATS_WORDS and int(s.abi_version) > 0, ctx
    got = stats_dict(s)
    for name in FIELDS:
        assert got[name] == want[name], (ctx, name, got[name], want[name])
    check_identities(got)


def assert_summary(s, index, ctx=""):
    """s: a scfq.ScreenSummary; index: a checker's index"""
    assert (int(s.n_refs), int(s.k), int(s.distinct)) == (len(index["names"]), index["k"], index["distinct"]), ctx
    for r, info in enumerate(index["refs"]):
        for f in REF_FIELDS:
            assert int(getattr(s.ref[r], f)) == info[f], (ctx, r, f, int(getattr(s.ref[r], f)), info[f])
    for r in range(len(index["refs"]), MAX_REFS):
        assert all(int(getattr(s.ref[r], f)) == 0 for f in REF_FIELDS), (ctx, r)


def pct_text(reads, reads_in):
    v = 10000 * reads // reads_in if reads_in else 0
    return "%d.%02d" % (v // 100, v % 100)


def report_rows(w, index):
    """the rows of scfq_format_screen_row_tsv, the row '*' last"""
    rows = []
    for r, (name, info) in enumerate(zip(index["names"], index["refs"])):
        rows.append("\t".join([name] + [str(v) for v in (info["bases"], info["kmers"], w["reads_in"], w["ref_reads"][r])] + [pct_text(w["ref_reads"][r], w["reads_in"])] +
                              [str(v) for v in (w["ref_only_reads"][r], w["ref_best_reads"][r], w["ref_kmer_hits"][r])]))
    rows.append("\t".join(["*"] + [str(v) for v in (sum(i["bases"] for i in index["refs"]), sum(i["kmers"] for i in index["refs"]), w["reads_in"],
                                                    w["matched_reads"])] + [pct_text(w["matched_reads"], w["reads_in"])] +
                          [str(v) for v in (w["matched_reads"] - w["multi_reads"], w["multi_reads"], w["hit_kmers"])]))
    return rows


def per_read_rows(w, index):
    """the rows of the CLI's --per-read file"""
    return ["%d\t%d\t%d\t%s\t%d\t%d" % (i, kmers, hit, index["names"][best] if best != 0xFF else "-", best_hits, mask)
            for i, (kmers, hit, best_hits, mask, best) in enumerate(w["recs"])]

"""One table of jobs for the code between a caller and the kernels: the caller-stream rule, the stream leases, the scratch pool and
the shared handles (tests/test_gpu_caller_stream.py, tests/test_gpu_threads.py).  A job is one `*_device` wrapper of pyhost/scfq.py
with fixed options:

  make(seed)            the input arrays (uint8), one or two
  decoy(seed)           other valid inputs of exactly the same byte lengths: another record count, other line lengths, other content
  wanted(inputs)        what the call owes, from the command's plain checker or the CPU oracle: a dict of parts, each comparable with ==
  run(torch, scfq, ptrs, outs, want, ctx)
                        the call on device pointers; returns (the host parts, {output: items written})
  outs                  the outputs the call writes to device memory: (part, bytes per item)
  context(scfq, inputs) what the call needs besides its inputs (a screen index, a sample sheet, a k-mer table), or None

About 300 pairs of 100 to 140 bases per input: every checker takes a fraction of a second, every call milliseconds.  One generator
serves all commands.  A pair is cut from a 1.5 kb genome (depth for fq-kcount and fq-normalize), from the screen's references or from
random text; inserts of 50 to 330 bases give mates that overlap, mates that run through into the adapters and mates that do not meet;
two thirds of the pairs begin with the barcodes of a five-sample sheet, some with a wrong letter; quality falls towards the end of every
fifth read, every eleventh second mate ends in G, every ninth header repeats an earlier one.  tests/test_caller_cases_host.py proves
without a GPU that every planted case occurs and that the decoys and the seeds can be told apart in every part that is compared."""
import functools
import os

import numpy as np

import _big_offset_cases as C
from conftest import GOLDEN, make_oracle
from _adapters_check import adapters_of_np
from _cycles_check import split as cycles_split, table_of_np
from _demux_check import FIELDS as DEMUX_FIELDS, demux_of
from _fa_gc_check import FaModel
from _insert_size_check import FIELDS as INSERT_FIELDS, insert_of_np, random_dna, revcomp
from _kcount_check import CANONICAL, dump_of, hist_of, kcount_of_np
from _kmers_check import kmers_of_np
from _merge_check import FIELDS as MERGE_FIELDS, merge_of_np, stat as merge_stat
from _normalize_check import FIELDS as NORM_FIELDS, normalize_of
from _readstats_check import per_read_np, summary_of
from _screen_check import FIELDS as SCREEN_FIELDS, PER_REF, contigs_of, index_of_np, screen_of_np
from _trim_check import FIELDS as TRIM_FIELDS, trim_of_np

WORKER_SEEDS = tuple(range(12))
SHORT_LINES, CRLF, SINGLE, EMPTY = 1, 2, 3, 12      # the seeds that are special on purpose; EMPTY is no worker seed: it has no decoy
ALL_SEEDS = WORKER_SEEDS + (EMPTY,)
TINY = 2000                                          # records of 8 bytes behind the others under SHORT_LINES

OUTSIDE_THE_CONTRACT = {
    "synth_device": "launches on the legacy default stream and synchronises the device: the header promises it no caller stream",
    "partial_simple_device": "a debug entry point (sc_fqcount_debug.h): the header promises it no caller stream",
}

SCREEN_NAMES = ("spike", "vector", "rrna")
SCREEN_FA = [os.path.join(GOLDEN, "screen", n + ".fa") for n in SCREEN_NAMES]
SAMPLES = C.DEMUX_SAMPLES
ADAPTER1, ADAPTER2 = C.LONG_ADAPTER, b"AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGTAGATCTCGGTGGTCGCCGTATCATT"
K = 21
NORM_RULE = dict(target=8, min_depth=2, seed=5)
NORM_BINS = 64
KCOUNT_BINS = 64

OVERLAP_REC = np.dtype([("offset", "<i4"), ("overlap", "<u2"), ("mismatches", "<u2")])
SCREEN_REC = np.dtype([("kmers", "<u4"), ("hit_kmers", "<u4"), ("best_hits", "<u4"), ("mask", "<u2"), ("best", "u1"), ("reserved", "u1")])
DEMUX_REC = np.dtype([("sample", "<u2"), ("mm1", "u1"), ("mm2", "u1"), ("state", "u1"), ("reserved", "u1", (3,))])
NORM_REC = np.dtype([("kmers", "<u4"), ("depth", "<u4"), ("min_count", "<u4"), ("weak", "<u4")])


def packed(recs, dtype, cols):
    """rows of a checker's table as the bytes of the library's records"""
    recs = np.asarray(recs, np.int64).reshape(-1, cols)
    out = np.zeros(recs.shape[0], dtype)
    for j, name in enumerate(n for n in dtype.names if n != "reserved"):
        out[name] = recs[:, j]
    return out.tobytes()


# ---- the inputs ---------------------------------------------------------------------------------------------------------------

_GENOME = random_dna(np.random.default_rng(20261100), 1500)


@functools.lru_cache(maxsize=None)
def ref_texts():
    return [c for p in SCREEN_FA for c in contigs_of(open(p, "rb").read()) if len(c) > 400]


@functools.lru_cache(maxsize=None)
def screen_index():
    """the checker's index of the three fixture references"""
    return index_of_np([(n, open(p, "rb").read()) for n, p in zip(SCREEN_NAMES, SCREEN_FA)], 31)


def shape(seed, decoy):
    """(pairs, bases of mate 1, bases of mate 2): another one for every seed, and far shorter reads in the decoys"""
    la = 104 + 3 * seed
    if seed == SINGLE:
        return (4, la // 3, la // 3 - 2) if decoy else (1, la, la - 4)
    return (420 + 7 * seed, la - 23, la - 30) if decoy else (300 + 7 * seed, la, la - 4)


def _barcodes(rng):
    """the letters before both mates: a sample's barcodes (one in seven with a wrong letter or an N), or nothing"""
    if rng.random() < 0.3:
        return b"", b""
    _, b1, b2 = SAMPLES[int(rng.integers(len(SAMPLES)))]
    codes = [bytearray(b1.encode()), bytearray(b2.encode())]
    y = rng.random()
    if y < 0.15:
        c = codes[int(rng.integers(2))]
        at = int(rng.integers(len(c)))
        c[at] = ord("N") if y >= 0.10 else [x for x in b"ACGT" if x != c[at]][int(rng.integers(3))]
    return bytes(codes[0]), bytes(codes[1])


def _quality(rng, n, falls):
    q = rng.integers(33 + 22, 33 + 41, n, dtype=np.uint8)
    if falls and n > 4:
        at = int(rng.integers(n // 2, n))
        q[at:] = rng.integers(33 + 2, 33 + 13, n - at, dtype=np.uint8)
    return q.tobytes()


def _records(seed, decoy):
    """[(record of mate 1, record of mate 2)] as lists of the four lines' texts"""
    rng = np.random.default_rng([20261101, int(decoy), seed])
    pairs, la, lb = shape(seed, decoy)
    refs, tag = ref_texts(), b"d" if decoy else b"s"
    out, names = [], []
    for i in range(pairs):
        u = rng.random()
        ins = int(rng.integers(50, 330))
        if seed == SINGLE and not decoy:
            u, ins = 0.6, la - 20                           # a reference's text, and both mates run through it into the adapters
        if u < 0.55:
            at = int(rng.integers(len(_GENOME)))
            frag = (_GENOME + _GENOME)[at:at + ins]
        elif u < 0.70:
            text = refs[int(rng.integers(len(refs)))]
            at = int(rng.integers(0, len(text) - ins))
            frag = text[at:at + ins]
        else:
            frag = random_dna(rng, ins)
        b1, b2 = _barcodes(rng) if pairs > 1 else (b"", b"")
        s1 = bytearray((b1 + frag + ADAPTER1 + random_dna(rng, la))[:la])
        s2 = bytearray((b2 + revcomp(frag) + ADAPTER2 + random_dna(rng, lb))[:lb])
        if i % 11 == 3:
            g = int(rng.integers(5, 25))
            s2[lb - g:] = b"G" * g
        if rng.random() < 0.04:
            s1[int(rng.integers(la))] = ord("N")
        name = b"%s%d.%d len=%d" % (tag, seed, i, ins)
        if i % 9 == 4:
            name = names[i - 3]
        names.append(name)
        out.append(([b"@" + name, bytes(s1), b"+", _quality(rng, la, i % 5 == 2)], [b"@" + name, bytes(s2), b"+", _quality(rng, lb, i % 5 == 4)]))
    if seed == SHORT_LINES:
        out += [([b"@" + b"t" * (j % 3), b"ACGT"[j % 4:j % 4 + 1], b"+", b"I"], [b"@" + b"t" * (j % 3), b"TGCA"[j % 4:j % 4 + 1], b"+", b"5"]) for j in range(TINY)]
    return out


def _text(records, eol):
    return b"".join(line + eol for rec in records for line in rec)


def _fit(records, eol, target, limit=None):
    """the longest run of whole units (tuples of records; `limit` at most) from the front that fits `target` bytes, its last header
    lengthened to fit"""
    size = lambda unit: sum(len(line) + len(eol) for rec in unit for line in rec)
    total, m = 0, 0
    while m < len(records) and m != limit and total + size(records[m]) <= target:
        total += size(records[m])
        m += 1
    assert m >= 1 and (m < len(records) or m == limit), (m, len(records), target)
    kept = [[list(rec) for rec in unit] for unit in records[:m]]
    kept[-1][-1][0] += b"x" * (target - total)
    return kept


@functools.lru_cache(maxsize=None)
def fastq(seed, decoy=False):
    """(mate 1, mate 2, interleaved) as uint8 arrays.  A decoy has the byte lengths of the seed's real inputs, file by file"""
    eol = b"\r\n" if seed == CRLF else b"\n"
    if seed == EMPTY:
        assert not decoy
        return (np.zeros(0, np.uint8),) * 3
    recs = _records(seed, decoy)
    if not decoy:
        texts = [_text([r[0] for r in recs], eol), _text([r[1] for r in recs], eol), _text([x for r in recs for x in r], eol)]
    else:
        real = fastq(seed)
        # the two files hold the same number of records: what fits both
        m = min(len(_fit([(r[j],) for r in recs], eol, real[j].size)) for j in (0, 1))
        texts = [_text([u[0] for u in _fit([(r[j],) for r in recs], eol, real[j].size, m)], eol) for j in (0, 1)]
        texts.append(_text([x for u in _fit(recs, eol, real[2].size) for x in u], eol))
    return tuple(np.frombuffer(t, np.uint8) for t in texts)


FA_LENGTHS = (30_011, 18_000, 64, 25_003, 9_000)


@functools.lru_cache(maxsize=None)
def fasta(seed, decoy=False):
    """contigs of the same lengths in the real input and in the decoy (the intervals asked are valid in both), other text, other line
    widths and so other offsets; the decoy's first header is lengthened to the real input's size"""
    if seed == EMPTY:
        return (np.zeros(0, np.uint8),)
    rng = np.random.default_rng([20261102, int(decoy), seed])
    eol = b"\r\n" if seed == CRLF else b"\n"
    lengths = (FA_LENGTHS[seed % 5],) if seed == SINGLE else tuple(v + 17 * seed for v in FA_LENGTHS[:3 + seed % 3])
    base = 7 if seed == SHORT_LINES else 50 + seed
    parts = []
    for j, length in enumerate(lengths):
        width = length if seed == SINGLE and decoy else base + 3 * j + (11 if decoy else 0)
        alphabet = b"ACGTACGTACGTACGTacgtNNRYgc" if j == 1 else b"ACGT"
        s = np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), length)].tobytes()
        parts += [b">%s%d_%d some text" % (b"d" if decoy else b"c", seed, j) + eol] + [s[i:i + width] + eol for i in range(0, length, width)]
    if decoy:
        pad = fasta(seed)[0].size - sum(map(len, parts))
        assert pad >= 0, pad
        parts[0] = parts[0][:-len(eol)] + b"x" * pad + eol
    return (np.frombuffer(b"".join(parts), np.uint8),)


def fa_queries(model):
    """intervals that depend on the contigs' lengths only"""
    return C.fasta_intervals(np.random.default_rng(5), model, 0)


# ---- the jobs -----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def oracle():
    return make_oracle()


def fields_of(s, names, lists=()):
    return {n: (list(getattr(s, n)) if n in lists else int(getattr(s, n))) for n in names}


def pick(w, names):
    return {n: w[n] for n in names}


def _args(ptrs):
    """(ptr1, n1, ptr2, n2) of one or two inputs"""
    return list(ptrs[0]) + (list(ptrs[1]) if len(ptrs) > 1 else [None, 0])


def _out(outs, name):
    return outs.get(name) if outs else None


def _host_head(scfq, host):
    """(ptr1, n1, ptr2, n2, is_device = 0) of one or two host arrays, for the entry points behind the `*_device` wrappers: the form
    with the input in host memory and the outputs in device memory, which no wrapper has"""
    head = []
    for a in host:
        head += [a.ctypes.data if a.size else None, a.size]
    return head + ([None, 0] if len(host) == 1 else []) + [0]


class Job:
    kind = "single"            # which of fastq()'s texts: "single" (mate 1), "pair", "interleaved"; or "fasta"
    outs = ()                  # (part, bytes per item) of the outputs in device memory
    accepts_empty = True

    def __init__(self, name, **kw):
        self.name = name
        self.__dict__.update(kw)

    def make(self, seed, decoy=False):
        if self.kind == "fasta":
            return list(fasta(seed, decoy))
        f = fastq(seed, decoy)
        return {"single": [f[0]], "pair": [f[0], f[1]], "interleaved": [f[2]]}[self.kind]

    def decoy(self, seed):
        return self.make(seed, True)

    def context(self, scfq, inputs):
        return None

    def wanted(self, inputs, base=None):
        """base: the inputs the context was made from, when they are not `inputs` (a decoy under the real input's k-mer table)"""
        raise NotImplementedError

    def __repr__(self):
        return self.name


class Count(Job):
    FIELDS = ("reads", "gc_bases", "n_bases", "bases", "lines", "newlines", "input_bytes", "bad_at", "bad_plus")
    parts, primary = ("counts", "qual_hist"), "counts"

    def wanted(self, inputs, base=None):
        c = oracle().count(inputs[0])
        return dict(counts=fields_of(c, self.FIELDS), qual_hist=list(c.qual_hist))

    def run(self, torch, scfq, ptrs, outs, want, ctx=None, host=None, **kw):
        c = scfq.count_device(*ptrs[0], flags=scfq.SCFQ_QUAL_HIST | scfq.SCFQ_STRUCT_CHECK, **kw)
        return dict(counts=fields_of(c, self.FIELDS), qual_hist=list(c.qual_hist)), {}


class Partial(Job):
    hist = False
    primary = "words"

    @property
    def parts(self):
        return ("words", "hist") if self.hist else ("words",)

    def wanted(self, inputs, base=None):
        if not self.hist:
            return dict(words=[int(x) for x in oracle().partial(inputs[0], -1)[:25]])
        w, h = oracle().partial(inputs[0], -1, want_hist=True)
        return dict(words=[int(x) for x in w[:25]], hist=[int(x) for x in h])

    def run(self, torch, scfq, ptrs, outs, want, ctx=None, host=None, **kw):
        if not self.hist:
            return dict(words=scfq.partial_device(*ptrs[0], -1, flags=scfq.SCFQ_STRUCT_CHECK, **kw).words()[:25]), {}
        p, h = scfq.partial_device(*ptrs[0], -1, flags=scfq.SCFQ_QUAL_HIST | scfq.SCFQ_HIST_EXACT | scfq.SCFQ_STRUCT_CHECK, want_hist=True, **kw)
        return dict(words=p.words()[:25], hist=list(h)), {}


class IndexLines(Job):
    parts, primary, outs = ("lines", "off"), "off", (("off", 8),)

    def wanted(self, inputs, base=None):
        w = C.index_of(inputs[0])
        return dict(lines=w["lines"], off=w["off"].astype("<i8").tobytes())

    def run(self, torch, scfq, ptrs, outs, want, ctx=None, host=None):
        if not outs:
            return dict(lines=scfq.index_lines_device(*ptrs[0])), {}
        lines = scfq.index_lines_device(*ptrs[0], *outs["off"])
        return dict(lines=lines), dict(off=lines + 1)


class Dedup(Job):
    FIELDS = ("total_reads", "duplicates", "records_out", "bytes_out")
    parts, primary, outs = ("stats", "out"), "out", (("out", 1),)

    def wanted(self, inputs, base=None):
        out, st = oracle().dedup(inputs[0])
        return dict(stats=fields_of(st, self.FIELDS), out=out)

    def run(self, torch, scfq, ptrs, outs, want, ctx=None, host=None):
        if host is None:
            nb, st = scfq.dedup_device(*ptrs[0], *(outs["out"] if outs else (None, 0)))
        else:
            import ctypes
            st, n = scfq._new_dedup_stats(), ctypes.c_uint64()
            scfq._check(scfq.lib().scfq_dedup_buffer(*_host_head(scfq, host)[:2], 0, ctypes.c_void_p(outs["out"][0]), outs["out"][1], 1, ctypes.byref(n),
                                                     ctypes.byref(st)), "scfq_dedup_buffer")
            nb = n.value
        assert nb == st.bytes_out
        return dict(stats=fields_of(st, self.FIELDS)), (dict(out=nb) if outs else {})


class ReadStats(Job):
    parts, primary, outs = ("summary", "rows"), "rows", (("rows", 40),)

    def wanted(self, inputs, base=None):
        rows, lines = per_read_np(inputs[0])
        s = summary_of(rows)
        s.update(input_bytes=int(inputs[0].size), lines=lines)
        return dict(summary=s, rows=np.asarray(rows, "<i8").tobytes())

    def run(self, torch, scfq, ptrs, outs, want, ctx=None, host=None):
        if host is None:
            s = scfq.read_stats_device(*ptrs[0], *(outs["rows"] if outs else (None, 0)))
        else:
            import ctypes
            s = scfq._new_read_summary()
            scfq._check_read_stats(scfq.lib().scfq_read_stats_buffer(*_host_head(scfq, host)[:2], 0, ctypes.c_void_p(outs["rows"][0]), outs["rows"][1],
                                                                     ctypes.byref(s)), "scfq_read_stats_buffer")
        got = {n: (list(getattr(s, n)) if isinstance(v, list) else int(getattr(s, n))) for n, v in want["summary"].items()}
        return dict(summary=got), (dict(rows=int(s.reads)) if outs else {})


class Cycles(Job):
    HEAD = ("reads", "lines", "input_bytes", "max_seq_len", "max_qual_len", "cycles")
    parts, primary = ("head", "tail", "total", "rows"), "rows"

    def wanted(self, inputs, base=None):
        table, lines, ms, mq = table_of_np(inputs[0])
        cap = 64                                        # fewer positions than the reads have: the rest lands in tail
        rows, tail, total = cycles_split(table, cap)
        return dict(head=dict(reads=(lines + 3) // 4, lines=lines, input_bytes=int(inputs[0].size), max_seq_len=ms, max_qual_len=mq, cycles=min(cap, max(ms, mq))),
                    tail=tail, total=total, rows=np.asarray(rows, "<i8").tobytes(), cap=cap)

    def run(self, torch, scfq, ptrs, outs, want, ctx=None, host=None):
        from _cycles_check import row_ints
        s, rows = scfq.cycles_device(*ptrs[0], want["cap"])
        return dict(head=fields_of(s, self.HEAD), tail=row_ints(s.tail), total=row_ints(s.total), rows=rows.tobytes()), {}


class Kmers(Job):
    HEAD = ("reads", "lines", "input_bytes", "k", "flags", "windows", "kmers", "skipped", "short_lines", "distinct", "max_count", "table_entries")
    parts, primary = ("head", "table"), "table"
    k, canonical = 5, False

    def wanted(self, inputs, base=None):
        table, windows, kmers, skipped, short, lines = kmers_of_np(inputs[0], self.k, self.canonical, dense=True)
        head = dict(reads=(lines + 3) // 4, lines=lines, input_bytes=int(inputs[0].size), k=self.k, flags=int(self.canonical), windows=windows, kmers=kmers,
                    skipped=skipped, short_lines=short, distinct=int((table > 0).sum()), max_count=int(table.max()), table_entries=4 ** self.k)
        return dict(head=head, table=table.astype("<u8").tobytes())

    def run(self, torch, scfq, ptrs, outs, want, ctx=None, host=None):
        s, table = scfq.kmers_device(*ptrs[0], self.k, scfq.SCFQ_KMERS_CANONICAL if self.canonical else 0, True)
        return dict(head=fields_of(s, self.HEAD), table=table.tobytes()), {}


class Adapters(Job):
    HEAD = ("reads", "lines", "input_bytes", "n_probes", "max_seq_len", "positions")
    parts, primary = ("head", "hits", "total", "rows"), "rows"
    PROBES = (b"AGATCGGAAGAGC", b"CACACGTCTGAACTCC", b"ACGTACGT")      # the adapter's head, its middle, and the first sample's barcode

    def wanted(self, inputs, base=None):
        rows, hits, total, max_len, lines = adapters_of_np(inputs[0], self.PROBES)
        cap = 64
        head = dict(reads=(lines + 3) // 4, lines=lines, input_bytes=int(inputs[0].size), n_probes=len(self.PROBES), max_seq_len=max_len, positions=min(cap, max_len))
        return dict(head=head, hits=[int(v) for v in hits], total=[int(v) for v in total], rows=np.asarray(rows[:cap], "<u8").tobytes(), cap=cap)

    def run(self, torch, scfq, ptrs, outs, want, ctx=None, host=None):
        from _adapters_check import row_of
        s, rows = scfq.adapters_device(*ptrs[0], list(self.PROBES), want["cap"])
        return dict(head=fields_of(s, self.HEAD), hits=list(s.hits), total=row_of(s.total), rows=rows.tobytes()), {}


class Paired(Job):
    """two files, or one interleaved"""
    kind = "pair"

    @property
    def interleaved(self):
        return self.kind == "interleaved"

    def texts(self, inputs):
        return (inputs[0], inputs[1] if len(inputs) > 1 else None)

    def drop_second(self, names):
        return tuple(n for n in names if not (self.interleaved and n in ("out2", "unmerged2")))


class InsertSize(Paired):
    primary, outs = "recs", (("recs", 8),)
    parts = ("summary", "hist", "recs")

    def wanted(self, inputs, base=None):
        w = insert_of_np(*self.texts(inputs))
        return dict(summary=pick(w, INSERT_FIELDS), hist=np.asarray(w["hist"], "<u8").tobytes(), recs=packed(w["recs"], OVERLAP_REC, 3))

    def run(self, torch, scfq, ptrs, outs, want, ctx=None, host=None):
        if host is None:
            s, hist = scfq.insert_size_device(*_args(ptrs), None, *(outs["recs"] if outs else (None, 0)))
        else:
            s, hist = scfq._insert_call(scfq.lib().scfq_insert_size_buffers, "scfq_insert_size_buffers", None, self.interleaved, *outs["recs"],
                                        *_host_head(scfq, host))
        return dict(summary=fields_of(s, INSERT_FIELDS), hist=hist.tobytes()), (dict(recs=int(s.pairs)) if outs else {})


class Merge(Paired):
    primary = "merged"

    @property
    def parts(self):
        return self.drop_second(("stats", "merged", "unmerged1", "unmerged2"))

    @property
    def outs(self):
        return tuple((n, 1) for n in self.parts[1:])

    def wanted(self, inputs, base=None):
        w = merge_of_np(*self.texts(inputs))
        return dict(stats={n: merge_stat(w, n) for n in MERGE_FIELDS}, merged=bytes(w["merged"]), unmerged1=bytes(w["unmerged1"]), unmerged2=bytes(w["unmerged2"]))

    def run(self, torch, scfq, ptrs, outs, want, ctx=None, host=None):
        three = (_out(outs, "merged"), _out(outs, "unmerged1"), _out(outs, "unmerged2"))
        if host is None:
            s = scfq.merge_device(*_args(ptrs), None, 33, *three)
        else:
            s = scfq._merge_call(scfq.lib().scfq_merge_buffers, "scfq_merge_buffers", None, 33, self.interleaved, _host_head(scfq, host),
                                 scfq._merge_outputs(three) + [1])
        used = dict(merged=int(s.merged_bytes), unmerged1=int(s.unmerged1_bytes), unmerged2=int(s.unmerged2_bytes))
        return dict(stats=fields_of(s, MERGE_FIELDS)), ({n: used[n] for n in outs} if outs else {})


class TwoOutputs(Paired):
    """the commands that write out1 and out2, most of them with a per-read table"""
    primary, rec = "out1", None       # rec: (bytes per entry, the stats field that counts the entries)

    @property
    def parts(self):
        return self.drop_second(("stats",) + (("recs",) if self.rec else ()) + ("out1", "out2")) + self.more

    more = ()

    @property
    def outs(self):
        return tuple((n, self.rec[0] if n == "recs" else 1) for n in self.parts if n in ("recs", "out1", "out2"))

    @staticmethod
    def table_args(recs):
        import ctypes
        return [ctypes.c_void_p(recs[0]) if recs else None, recs[1] if recs else 0]

    def used(self, s, outs):
        sizes = dict(out1=int(s.out1_bytes), out2=int(s.out2_bytes))
        if self.rec:
            sizes["recs"] = int(getattr(s, self.rec[1]))
        return {n: sizes[n] for n in outs} if outs else {}


class Trim(TwoOutputs):
    def wanted(self, inputs, base=None):
        w = trim_of_np(*self.texts(inputs), interleaved=self.interleaved, **C.TRIM_ALL)
        return dict(stats=pick(w, TRIM_FIELDS), out1=bytes(w["out1"]), out2=bytes(w["out2"]))

    def run(self, torch, scfq, ptrs, outs, want, ctx=None, host=None):
        opts, two = scfq.trim_opts(interleaved=self.interleaved, **C.TRIM_ALL), (_out(outs, "out1"), _out(outs, "out2"))
        if host is None:
            s = scfq.trim_device(*_args(ptrs), opts, *two)
        else:
            s = scfq._trim_call(scfq.lib().scfq_trim_buffers, "scfq_trim_buffers", opts, _host_head(scfq, host), scfq._trim_outputs(two) + [1])
        return dict(stats=fields_of(s, TRIM_FIELDS, ("adapter_reads",))), self.used(s, outs)


class Screen(TwoOutputs):
    rec = (16, "reads_in")
    opts = dict(min_hits=3)

    def context(self, scfq, inputs):
        return scfq.screen_index_files(SCREEN_FA)

    def wanted(self, inputs, base=None):
        w = screen_of_np(screen_index(), *self.texts(inputs), interleaved=self.interleaved, **self.opts)
        return dict(stats=pick(w, SCREEN_FIELDS), recs=packed(w["recs"], SCREEN_REC, 5), out1=bytes(w["out1"]), out2=bytes(w["out2"]))

    def run(self, torch, scfq, ptrs, outs, want, ctx=None, host=None):
        opts, two, recs = scfq.screen_opts(interleaved=self.interleaved, **self.opts), (_out(outs, "out1"), _out(outs, "out2")), _out(outs, "recs")
        if host is None:
            s = scfq.screen_device(ctx, *_args(ptrs), opts, *two, recs=recs)
        else:
            s = scfq._screen_call(scfq.lib().scfq_screen_buffers, "scfq_screen_buffers", ctx, opts, _host_head(scfq, host),
                                  self.table_args(recs) + scfq._trim_outputs(two) + [1])
        return dict(stats=fields_of(s, SCREEN_FIELDS, PER_REF)), self.used(s, outs)


class Demux(TwoOutputs):
    rec = (8, "units_in")
    more = ("rows",)
    opts = dict(mismatches=1)

    def context(self, scfq, inputs):
        return scfq.demux_sheet(list(SAMPLES))

    def wanted(self, inputs, base=None):
        a1, a2 = self.texts(inputs)
        w = demux_of(a1.tobytes(), None if a2 is None else a2.tobytes(), list(SAMPLES), interleaved=self.interleaved, **self.opts)
        return dict(stats=pick(w, DEMUX_FIELDS), rows=w["rows"], recs=packed(w["recs"], DEMUX_REC, 4), out1=w["out1"], out2=w["out2"])

    def run(self, torch, scfq, ptrs, outs, want, ctx=None, host=None):
        from _demux_check import rows_of
        opts, two, recs = scfq.demux_opts(interleaved=self.interleaved, **self.opts), (_out(outs, "out1"), _out(outs, "out2")), _out(outs, "recs")
        if host is None:
            s, rows = scfq.demux_device(ctx, *_args(ptrs), opts, *two, recs=recs)
        else:
            s, rows = scfq._demux_call(scfq.lib().scfq_demux_buffers, "scfq_demux_buffers", ctx, opts, _host_head(scfq, host), self.table_args(recs),
                                       scfq._trim_outputs(two) + [1])
        return dict(stats=fields_of(s, DEMUX_FIELDS), rows=rows_of(rows)), self.used(s, outs)


def kcount_table(inputs):
    """the checker's {key: count} of fq-kcount -k 21 --canonical over one or two inputs"""
    return kcount_of_np(list(inputs), K, True)


class Kcount(Paired):
    HEAD = ("reads", "lines", "input_bytes", "k", "flags", "windows", "kmers", "skipped", "short_lines", "distinct", "unique", "max_count")
    parts, primary = ("head", "hist", "dump"), "dump"

    def wanted(self, inputs, base=None):
        w = kcount_table(inputs)
        head = dict(reads=w.reads, lines=w.lines, input_bytes=w.input_bytes, k=K, flags=CANONICAL, windows=w.windows, kmers=w.kmers, skipped=w.skipped,
                    short_lines=w.short_lines, distinct=w.distinct, unique=w.unique, max_count=w.max_count)
        return dict(head=head, hist=hist_of(w.table, KCOUNT_BINS), dump=np.array(dump_of(w.table), "<u8").reshape(-1, 2).tobytes())

    def run(self, torch, scfq, ptrs, outs, want, ctx=None, host=None):
        s, t = scfq.kcount_device(*_args(ptrs), k=K, flags=scfq.SCFQ_KCOUNT_CANONICAL)
        with t:
            return dict(head=fields_of(s, self.HEAD), hist=t.hist(KCOUNT_BINS).tolist(), dump=t.dump(1, 0).tobytes()), {}


class Normalize(TwoOutputs):
    rec = (16, "reads_in")
    more = ("hist",)
    two_pass = False

    def context(self, scfq, inputs):
        if self.two_pass:
            return None
        s, t = scfq.kcount_host(*inputs, k=K, flags=scfq.SCFQ_KCOUNT_CANONICAL)
        return t

    def wanted(self, inputs, base=None):
        a1, a2 = self.texts(inputs)
        table = kcount_table(inputs if base is None or self.two_pass else base).table
        w = normalize_of(table, K, True, a1.tobytes(), None if a2 is None else a2.tobytes(), interleaved=self.interleaved, bins=NORM_BINS, **NORM_RULE)
        return dict(stats=pick(w, NORM_FIELDS), hist=[list(r) for r in w["hist"]], recs=packed(w["recs"], NORM_REC, 4), out1=w["out1"], out2=w["out2"])

    def run(self, torch, scfq, ptrs, outs, want, ctx=None, host=None):
        more = dict(k=K, canonical=True) if self.two_pass else {}
        opts, two, recs = scfq.norm_opts(interleaved=self.interleaved, **NORM_RULE, **more), (_out(outs, "out1"), _out(outs, "out2")), _out(outs, "recs")
        if host is None:
            s, hist = scfq.norm_device(ctx, *_args(ptrs), opts, *two, recs=recs, bins=NORM_BINS)
        else:
            s, hist = scfq._norm_call(scfq.lib().scfq_norm_buffers, "scfq_norm_buffers", ctx, opts, _host_head(scfq, host),
                                      self.table_args(recs) + scfq._trim_outputs(two) + [1], NORM_BINS)
        return dict(stats=fields_of(s, NORM_FIELDS), hist=hist.tolist()), self.used(s, outs)


class FaGc(Job):
    """fa_index_device, then fa_count_intervals, which reads the caller's buffer again"""
    kind = "fasta"
    SUMMARY = ("input_bytes", "contigs", "bases", "gc_bases", "acgt_bases", "orphan_bases")
    parts, primary = ("summary", "contigs", "counts"), "counts"

    def wanted(self, inputs, base=None):
        m = FaModel(inputs[0])
        return dict(summary=dict(input_bytes=m.n, contigs=len(m.contigs), bases=m.bases, gc_bases=m.gc_bases, acgt_bases=m.acgt_bases, orphan_bases=m.orphan_bases),
                    contigs=[(c[0].decode("latin-1"), c[1], c[3]) for c in m.contigs], counts=m.count_many(fa_queries(m)).astype("<u8").tobytes(),
                    queries=fa_queries(m))

    def run(self, torch, scfq, ptrs, outs, want, ctx=None, host=None):
        with scfq.fa_index_device(*ptrs[0]) as ix:
            counts = scfq.fa_count_intervals(ix, want["queries"]) if want["queries"] else np.zeros((0, 3), np.uint64)
            return dict(summary=fields_of(ix.summary, self.SUMMARY), contigs=list(ix.contigs), counts=counts.tobytes()), {}


JOBS = (
    Count("count_device"),
    Partial("partial_device"),
    Partial("partial_device+hist", hist=True),
    IndexLines("index_lines_device"),
    Dedup("dedup_device"),
    ReadStats("read_stats_device"),
    Cycles("cycles_device"),
    Kmers("kmers_device k=5", k=5),
    Kmers("kmers_device k=9 canonical", k=9, canonical=True),
    Adapters("adapters_device"),
    InsertSize("insert_size_device"),
    InsertSize("insert_size_device interleaved", kind="interleaved"),
    Merge("merge_device"),
    Merge("merge_device interleaved", kind="interleaved"),
    Trim("trim_device"),
    Trim("trim_device interleaved", kind="interleaved"),
    Screen("screen_device"),
    Screen("screen_device interleaved", kind="interleaved"),
    Demux("demux_device"),
    Demux("demux_device interleaved", kind="interleaved"),
    Kcount("kcount_device"),
    Normalize("norm_device"),
    Normalize("norm_device interleaved", kind="interleaved"),
    Normalize("norm_device two-pass", two_pass=True),
    FaGc("fa_index_device"),
)
BY_NAME = {j.name: j for j in JOBS}


def wrapper_of(job):
    """the attribute of scfq that the job calls"""
    return job.name.split(" ")[0].split("+")[0]


_wanted = {}


def wanted(job, seed, decoy=False):
    """a job's wanted result for a seed, computed once per process.  A decoy under a context made from the real input (fq-normalize
    against a given table) is judged against that context"""
    key = (job.name, seed, decoy)
    if key not in _wanted:
        _wanted[key] = job.wanted(job.make(seed, decoy), base=job.make(seed) if decoy else None)
    return _wanted[key]


# ---- device memory for a call: what both GPU files do around run() ---------------------------------------------------------------

SENTINEL, BLANK, GUARD, SLACK = 0xA5, 0x11, 256, 16      # SLACK: items of capacity beyond what the call writes


def place(torch, arr, offset=0):
    """tests/test_gpu_parity.py's to_dev (guard bytes 'G', `offset` bytes past a 4 KiB boundary, synchronised): (tensor, address, the
    input's bytes as a view of the tensor)"""
    from test_gpu_parity import to_dev
    t, ptr = to_dev(torch, arr, offset)
    start = ptr - t.data_ptr()
    assert ptr % 4096 == offset % 4096
    return t, ptr, t[start:start + arr.size]


class Room:
    """device memory for `items` items of `size` bytes and SLACK more, between GUARD bytes on either side"""

    def __init__(self, torch, items, size, fill=SENTINEL):
        self.size, self.cap = size, items + SLACK
        self.t = torch.full((2 * GUARD + self.cap * size,), fill, dtype=torch.uint8, device="cuda")
        self.ptr = self.t.data_ptr() + GUARD

    def arg(self):
        return (self.ptr, self.cap)

    def check(self, host, used, want, ctx):
        """host: the whole tensor read back.  The first `used` items are `want`; every other byte is still the sentinel"""
        body = host[GUARD:GUARD + self.cap * self.size].tobytes()
        assert used * self.size == len(want), (ctx, "items written", used, len(want) // self.size)
        if body[:len(want)] != want:
            at = next(i for i, (a, b) in enumerate(zip(body, want)) if a != b)
            kind = "the sentinel: the output was overwritten" if body[at] == SENTINEL else "other bytes"
            raise AssertionError((ctx, "differs from byte %d of %d on" % (at, len(want)), kind, body[at:at + 40], want[at:at + 40]))
        assert body[len(want):] == bytes([SENTINEL]) * (len(body) - len(want)), (ctx, "bytes behind the reported size were written")
        assert bool((host[:GUARD] == SENTINEL).all()) and bool((host[GUARD + self.cap * self.size:] == SENTINEL).all()), (ctx, "guard bytes were written")


def rooms_of(torch, job, want, fill=SENTINEL):
    return {name: Room(torch, len(want[name]) // size, size, fill) for name, size in job.outs}


def compare(job, got, want, ctx, other=None):
    """every host part of a call against the wanted result; other: the decoy's wanted result, named when that is what came back"""
    for part in job.parts:
        if part in got and (type(got[part]) != type(want[part]) or got[part] != want[part]):
            is_other = other is not None and type(got[part]) == type(other[part]) and got[part] == other[part]
            detail = got[part] if not isinstance(got[part], bytes) or len(got[part]) < 200 else "%d bytes" % len(got[part])
            raise AssertionError((ctx, part, "is the decoy's result" if is_other else "differs", detail))


def call(torch, scfq, job, ptrs, want, ctx, label, host=None):
    """one call with fresh outputs, everything compared; the device outputs are read back on the current stream"""
    rooms = rooms_of(torch, job, want)
    got, used = job.run(torch, scfq, ptrs, {n: r.arg() for n, r in rooms.items()}, want, ctx, host=host)
    compare(job, got, want, label)
    assert set(used) == set(rooms), (label, used)
    for name, room in rooms.items():
        room.check(room.t.cpu().numpy(), used[name], want[name], (label, name))
    return got

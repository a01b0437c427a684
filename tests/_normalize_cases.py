"""The cases of test_gpu_normalize.py that also run in a child process under another environment (tests/_normalize_child.py):
SCFQ_NORM_LDS_WINDOWS and SCFQ_KCOUNT_START_BITS are read once per process.  Every function takes (torch, scfq), compares what the
library returns with the checker of _normalize_check.py with == and returns the number of calls it compared."""
import numpy as np

from _every_k_cases import NORM_OPTS, OFFSETS, cases
from _kcount_check import kcount_of, kcount_of_np
from _normalize_check import assert_stats, normalize_of

BUILT_IN_C = 2048                   # kNmC of csrc/scfq_norm.hip
SENTINEL, GUARD = 0xA5, 256
COMP = bytes.maketrans(b"ACGT", b"TGCA")
REC = np.dtype([("kmers", "<u4"), ("depth", "<u4"), ("min_count", "<u4"), ("weak", "<u4")])


def revcomp(s):
    return s.translate(COMP)[::-1]


def dna(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))


def fastq(seqs, eol=b"\n", final=True):
    data = b"".join(b"@r%d" % i + eol + s + eol + b"+" + eol + b"I" * len(s) + eol for i, s in enumerate(seqs))
    return data if final else data[:len(data) - len(eol)]


def as_array(data):
    return None if data is None else np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data


def to_dev(torch, arr, offset=0, pad=8192):
    """device copy of arr placed `offset` bytes past a 4 KiB-aligned address, with guard bytes around"""
    t = torch.full((pad + offset + arr.size + pad,), 0x47, dtype=torch.uint8, device="cuda")   # guards are 'G'
    base = t.data_ptr()
    start = ((base + pad + 4095) // 4096) * 4096 - base + offset
    if arr.size:
        t[start:start + arr.size] = torch.from_numpy(arr.copy())
    torch.cuda.synchronize()
    return t, base + start


class Out:
    """device memory for `cap` bytes between sentinel bytes, `off` bytes past a 256-byte boundary"""

    def __init__(self, torch, cap, off=1):
        self.cap, self.off = cap, off
        self.t = torch.full((2 * GUARD + off + cap,), SENTINEL, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 256 == 0
        self.ptr = self.t.data_ptr() + GUARD + off
        torch.cuda.synchronize()

    def arg(self):
        return (self.ptr, self.cap)

    def bytes(self, n):
        """the first n bytes; everything else still holds the sentinel"""
        h = self.t.cpu().numpy()
        lo = GUARD + self.off
        assert (h[:lo] == SENTINEL).all() and (h[lo + n:] == SENTINEL).all(), "bytes outside [0, %d) were written" % n
        return h[lo:lo + n].tobytes()


def differ(ctx, name, have, want):
    if have != want:
        at = next((i for i in range(min(len(have), len(want))) if have[i] != want[i]), min(len(have), len(want)))
        raise AssertionError((ctx, name, "differs at byte", at, len(have), len(want), have[max(0, at - 40):at + 40], want[max(0, at - 40):at + 40]))


def table_of(counted, k, canonical, big=False):
    """the checker's table {key: count} of the counted inputs (bytes, or a list of one or two)"""
    if big:
        counted = [counted] if isinstance(counted, (bytes, bytearray)) else counted
        return kcount_of_np([as_array(c) for c in counted], k, canonical).table
    return kcount_of(counted, k, canonical).table


def device_table(scfq, counted, k, canonical, table_bits=0):
    counted = [counted] if isinstance(counted, (bytes, bytearray)) else counted
    s, t = scfq.kcount_host(counted[0], counted[1] if len(counted) > 1 else None, k=k, flags=1 if canonical else 0, table_bits=table_bits)
    return t


def compare(scfq, got, hist, want, ctx, outs=None, table=None, reads=None):
    assert_stats(got, want, ctx)
    if hist is not None:
        assert hist.tolist() == want["hist"], (ctx, "hist", [(d, h, w) for d, (h, w) in enumerate(zip(hist.tolist(), want["hist"])) if h != w][:5])
    for key, o in zip(("out1", "out2"), outs or ()):
        if o is not None:
            differ(ctx, key, o.bytes(len(want[key])), want[key])
    if table is not None:
        recs = np.frombuffer(table.bytes(16 * reads), REC)
        have = [tuple(int(x) for x in r) for r in recs.tolist()]
        if have != want["recs"]:
            at = next(i for i in range(reads) if have[i] != want["recs"][i])
            raise AssertionError((ctx, "read", at, have[at], want["recs"][at]))


def check_device(torch, scfq, dtable, ctable, k, canonical, d1, d2=None, ctx="", bins=40, offs=(0, 0), out_offs=(1, 3), want=None, extra=7, two_pass=None, **kw):
    """the device entry point on d1 / d2 against the table dtable (None: the two-pass form with the options two_pass): the sizing call,
    then outputs of the reported sizes + extra bytes between sentinels, the per-read table between sentinels, and the histogram"""
    a1, a2 = as_array(d1), as_array(d2)
    if want is None:
        want = normalize_of(ctable, k, canonical, bytes(d1), None if d2 is None else bytes(d2), bins=bins, **kw)
    opts = scfq.norm_opts(**dict(kw, **(two_pass or {})))
    t1, p1 = to_dev(torch, a1, offs[0])
    t2, p2 = to_dev(torch, a2, offs[1]) if a2 is not None else (None, None)
    n2 = a2.size if a2 is not None else 0
    s, _ = scfq.norm_device(dtable, p1, a1.size, p2, n2, opts)
    compare(scfq, s, None, want, (ctx, "sizing"))
    outs = [Out(torch, len(want["out1"]) + extra, out_offs[0]), Out(torch, len(want["out2"]) + extra, out_offs[1]) if a2 is not None else None]
    reads = want["reads_in"]
    table = Out(torch, 16 * reads + 16, 0)
    got, hist = scfq.norm_device(dtable, p1, a1.size, p2, n2, opts, *[o.arg() if o else None for o in outs], recs=(table.ptr, reads), bins=bins)
    compare(scfq, got, hist, want, (ctx, kw, offs), outs, table, reads)
    return want, got


# ---- 2. read lengths ------------------------------------------------------------------------------------------------------------
def lengths(torch, scfq, c=BUILT_IN_C):
    """reads of k - 1, k, k + 1 bases; 63 / 64 / 65, 511 / 512 / 513 and c - 1 / c / c + 1 windows (c: the windows a wave keeps in LDS);
    a line of 50 000 bases; reads of N, of lower case, with every other byte invalid; "\\r\\n" and no final newline; the table is counted
    from the same input, whose reads overlap in a genome of 3000 bases"""
    rng = np.random.default_rng(20261022)
    genome = dna(rng, 3000)
    calls = 0
    for k in (13, 21, 31, 32):
        for canonical in (False, True):
            def piece(n):
                at = int(rng.integers(0, len(genome) - min(n, 2500)))
                s = (genome[at:] + genome)[:n] if n <= len(genome) else b"".join(piece(int(rng.integers(100, 400))) for _ in range(n // 100))[:n]
                return revcomp(s) if rng.integers(2) else s
            windows = sorted({63, 64, 65, 511, 512, 513, c - 1, c, c + 1, BUILT_IN_C - 1, BUILT_IN_C, BUILT_IN_C + 1})
            seqs = [piece(k - 1), piece(k), piece(k + 1)] + [piece(w + k - 1) for w in windows]
            long = b"".join(piece(int(rng.integers(100, 400))) for _ in range(260))[:50000]
            assert len(long) == 50000
            odd = bytes(b if i % 2 else ord("N") for i, b in enumerate(piece(90)))
            seqs += [long, b"N" * 70, piece(80).lower(), odd, piece(40) + b"N" + piece(40), b"", piece(k + 5)]
            for eol, final in ((b"\n", True), (b"\r\n", True), (b"\n", False), (b"\r\n", False)):
                data = fastq(seqs if eol == b"\n" and final else seqs[:8] + seqs[-6:], eol, final)
                ctable = table_of(data, k, canonical, big=True)
                with device_table(scfq, data, k, canonical) as dtable:
                    check_device(torch, scfq, dtable, ctable, k, canonical, data, ctx=("lengths", k, canonical, eol, final, c), target=6, min_depth=2, bins=12)
                calls += 1
    return calls


# ---- 3. the select --------------------------------------------------------------------------------------------------------------
def planted(rng, counts, k):
    """a read of len(counts) windows and the lines that give window i the count counts[i] in a plain table"""
    s = dna(rng, len(counts) + k - 1)
    lines = []
    for i, c in enumerate(counts):
        lines += [s[i:i + k]] * c
    return s, lines


def select(torch, scfq):
    rng = np.random.default_rng(20261023)
    k = 21
    shapes = {"all equal": [7] * 12, "two values, even": [3] * 5 + [9] * 5, "two values, odd": [3] * 5 + [9] * 6, "two values, odd, low": [3] * 6 + [9] * 5,
              "maximum last": [4] * 9 + [300], "minimum first": [1] + [20] * 9, "one k-mer": [5], "zero and more": [0, 0, 0, 6, 6], "all absent": [0] * 30,
              "steps": list(range(1, 66)), "steps, down": list(range(130, 0, -1)), "powers": [1 << b for b in range(11)] * 3}
    reads, lines = [], []
    for name, counts in shapes.items():
        s, ls = planted(rng, counts, k)
        reads.append(s)
        lines += ls
    poly = b"A" * 70000                                   # one count above 2^16: rounds above bit 15
    reads += [b"A" * (k + 4), b"A" * (k + 2) + dna(rng, 30), dna(rng, 30) + b"A" * (k + 1)]
    counted = fastq(lines + [poly])
    ctable = table_of(counted, k, False, big=True)
    assert ctable[0] == 70000 - k + 1 > 1 << 16
    data = fastq(reads)
    want = normalize_of(ctable, k, False, data, bins=8)
    by_name = dict(zip(shapes, want["recs"]))
    assert by_name["all equal"] == (12, 7, 7, 0) and by_name["two values, even"] == (10, 3, 3, 0) and by_name["two values, odd"] == (11, 9, 3, 0)
    assert by_name["two values, odd, low"] == (11, 3, 3, 0) and by_name["maximum last"] == (10, 4, 4, 0) and by_name["minimum first"] == (10, 20, 1, 1)
    assert by_name["all absent"] == (30, 0, 0, 30) and by_name["steps"][1] == 33 and by_name["steps, down"][1] == 65
    assert want["recs"][len(shapes)] == (5, 69980, 69980, 0) and want["absent_kmers"] > 30
    with device_table(scfq, counted, k, False) as dtable:
        check_device(torch, scfq, dtable, ctable, k, False, data, ctx="select", want=want, bins=8)
        check_device(torch, scfq, dtable, ctable, k, False, data, ctx="select, weak", weak_below=7, target=5, bins=70000)
    return 2


# ---- 4. special keys ------------------------------------------------------------------------------------------------------------
def special_keys(torch, scfq):
    rng = np.random.default_rng(20261024)
    calls = 0
    # the all-ones key at k = 32, plain: the handle's `ones`
    a = dna(rng, 50)
    counted = fastq([b"T" * 40, b"T" * 33, a, b"G" + b"T" * 35])
    data = fastq([b"T" * 35, b"T" * 32, a[:40] + b"T" * 34, b"A" * 40, b"T" * 31 + b"N" + b"T" * 40])
    for canonical in (False, True):
        ctable = table_of(counted, 32, canonical)
        assert ctable[0 if canonical else 2 ** 64 - 1] == 9 + 2 + 4
        with device_table(scfq, counted, 32, canonical) as dtable:
            want, _ = check_device(torch, scfq, dtable, ctable, 32, canonical, data, ctx=("ones", canonical), min_depth=1)
        assert want["recs"][0] == (4, 15, 15, 0) and want["recs"][3] == ((9, 15, 15, 0) if canonical else (9, 0, 0, 9))
        calls += 1
    # palindromes in canonical mode; a plain table against reverse-complemented reads
    pal = b"ACGTACG" + b"CGTACGT"
    assert revcomp(pal) == pal
    b = dna(rng, 60)
    counted = fastq([pal, pal, b, pal + b[:20]])
    reads = fastq([pal, revcomp(b), b, pal + b"A"])
    for canonical in (False, True):
        ctable = table_of(counted, 14, canonical)
        with device_table(scfq, counted, 14, canonical) as dtable:
            want, _ = check_device(torch, scfq, dtable, ctable, 14, canonical, reads, ctx=("palindrome", canonical))
        assert want["recs"][0] == (1, 3, 3, 0)
        assert want["recs"][1][1] == (1 if canonical else 0) and (want["absent_kmers"] > 40) == (not canonical)
        calls += 1
    return calls


# ---- 5. the rule ----------------------------------------------------------------------------------------------------------------
def rule(torch, scfq):
    rng = np.random.default_rng(20261025)
    k, D = 21, 12
    s, lines = planted(rng, [D] * 10, k)
    low, low_lines = planted(rng, [5] * 10, k)
    counted = fastq(lines + low_lines)
    ctable = table_of(counted, k, False)
    calls = 0
    with device_table(scfq, counted, k, False) as dtable:
        data = fastq([s] * 300)                              # 300 units of depth D: the ordinal alone tells them apart
        kept = {}
        for name, kw in (("D == target", dict(target=D)), ("D == target + 1", dict(target=D - 1)), ("target 0", dict()), ("target 1", dict(target=1)),
                         ("target 6", dict(target=6)), ("seed 1", dict(target=6, seed=1)), ("seed 1 again", dict(target=6, seed=1)),
                         ("seed 2^63", dict(target=6, seed=2 ** 63 + 5)), ("min_depth D", dict(min_depth=D)), ("min_depth D + 1", dict(min_depth=D + 1))):
            want, _ = check_device(torch, scfq, dtable, ctable, k, False, data, ctx=("rule", name), bins=D + 2, **kw)
            kept[name] = want["classes"]
            calls += 1
        assert sum(c == 0 for c in kept["D == target"]) == 300 == sum(c == 0 for c in kept["target 0"]) == sum(c == 0 for c in kept["min_depth D"])
        assert 0 < sum(c == 3 for c in kept["D == target + 1"]) < 60 and sum(c == 2 for c in kept["min_depth D + 1"]) == 300
        assert 110 < sum(c == 0 for c in kept["target 6"]) < 190 and kept["seed 1"] == kept["seed 1 again"]
        assert kept["seed 1"] != kept["target 6"] != kept["seed 2^63"] != kept["seed 1"]
        # pairs: the lower mate decides; one mate without k-mers; both without
        r1 = fastq([s, low, s, b"ACGT", b"ACGT", s, b"N" * 30])
        r2 = fastq([low, s, s, s, b"NNNN", b"", low])
        for kw in (dict(min_depth=6), dict(min_depth=6, keep_no_kmers=True), dict(target=4, seed=3)):
            want, _ = check_device(torch, scfq, dtable, ctable, k, False, r1, r2, ctx=("pairs", kw), bins=D + 2, **kw)
            il = b"".join(x for pair in zip(split_records(r1), split_records(r2)) for x in pair)
            wi, _ = check_device(torch, scfq, dtable, ctable, k, False, il, ctx=("interleaved", kw), bins=D + 2, interleaved=True, **kw)
            calls += 2
            if "min_depth" in kw:
                keep_no = kw.get("keep_no_kmers", False)
                assert want["classes"] == [2, 2, 0, 0, 1, 0, 2] and want["units_out"] == (4 if keep_no else 3) == wi["units_out"]
            # the outputs are in step: equal record counts and matching names
            n1, n2 = names(want["out1"]), names(want["out2"])
            assert n1 == n2 and len(n1) == want["units_out"] and names(wi["out1"]) == [n for n in n1 for _ in (0, 1)]
    return calls


def split_records(data):
    lines = data.split(b"\n")[:-1]
    return [b"".join(x + b"\n" for x in lines[i:i + 4]) for i in range(0, len(lines), 4)]


def names(data):
    return data.split(b"\n")[0:-1:4]


# ---- 8. partition ---------------------------------------------------------------------------------------------------------------
def partition(torch, scfq):
    """1, 4, 5 and a few thousand reads (the waves of a block, the blocks' strides, the groups of 32), unequal numbers of reads"""
    rng = np.random.default_rng(20261026)
    k = 15
    genome = dna(rng, 800)

    def reads(n):
        out = []
        for _ in range(n):
            at, ln = int(rng.integers(0, 700)), int(rng.integers(10, 100))
            s = genome[at:at + ln]
            out.append(revcomp(s) if rng.integers(2) else s)
        return out
    calls = 0
    for n in (1, 4, 5, 33, 3000):
        data = fastq(reads(n))
        ctable = table_of(data, k, True, big=True)
        with device_table(scfq, data, k, True) as dtable:
            check_device(torch, scfq, dtable, ctable, k, True, data, ctx=("partition", n), target=30, min_depth=2, bins=200)
            calls += 1
            if n >= 4:
                other = fastq(reads(n - 3 if n < 100 else n - 70))
                check_device(torch, scfq, dtable, ctable, k, True, data, other, ctx=("partition, two", n), target=30, min_depth=2, bins=200)
                check_device(torch, scfq, dtable, ctable, k, True, other, data, ctx=("partition, two, swapped", n), target=30, min_depth=2, bins=200)
                check_device(torch, scfq, dtable, ctable, k, True, data, ctx=("partition, interleaved", n), target=30, min_depth=2, bins=200, interleaved=True)
                calls += 3
    return calls


# ---- 9. every k -----------------------------------------------------------------------------------------------------------------
def every_k_one(torch, scfq, k, offsets=OFFSETS, two_pass_at=(OFFSETS[0], OFFSETS[-1])):
    """the case set of _every_k_cases.py at one k, plain and canonical, against a table counted from the set itself: as a handle with the
    device pointer at each of `offsets`, and in the two-pass form at each of `two_pass_at`"""
    data = cases(k).fastq
    calls = 0
    for canonical in (False, True):
        ctable = table_of(data, k, canonical, big=True)
        want = normalize_of(ctable, k, canonical, data, bins=12, **NORM_OPTS)
        assert set(want["classes"]) == {0, 1, 2, 3} and max(r[0] for r in want["recs"]) == 513
        with device_table(scfq, data, k, canonical) as dtable:
            for off in offsets:
                check_device(torch, scfq, dtable, ctable, k, canonical, data, ctx=("every k", k, canonical, off), want=want, bins=12, offs=(off, 0), **NORM_OPTS)
        for off in two_pass_at:
            check_device(torch, scfq, None, ctable, k, canonical, data, ctx=("every k, two-pass", k, canonical, off), want=want, bins=12, offs=(off, 0),
                         two_pass=dict(k=k, canonical=canonical), **NORM_OPTS)
        calls += len(offsets) + len(two_pass_at)
    return calls


def every_k(torch, scfq, c=BUILT_IN_C):
    """every k at one offset each: the run under SCFQ_NORM_LDS_WINDOWS=64, where the reads of 65 and more windows select from device memory"""
    return sum(every_k_one(torch, scfq, k, offsets=OFFSETS[1:2], two_pass_at=OFFSETS[:1]) for k in range(13, 33))


CASES = {"every_k": every_k, "lengths": lengths, "select": select, "special_keys": special_keys, "rule": rule, "partition": partition}

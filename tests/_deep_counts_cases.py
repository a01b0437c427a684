"""Counts past 32 bits, stated by arithmetic: one record whose sequence line is four homopolymer runs with an 'N' between them (RUNS,
about 10 GiB; test_gpu_deep_counts.py makes it on the device), the table fq-kcount has to return for it, and the small read set whose
per-read records against that table take every shape of fq-normalize's saturation at SCFQ_NORM_MAX_DEPTH = 2^32 - 2.  The host side
(test_every_k_cases_host.py) proves the shapes with the checker alone."""
from _every_k_cases import fastq_of, source
from _kmers_check import index_of

RUNS = ((b"A", 2 ** 32 + 4096), (b"T", 2 ** 32 + 8192), (b"C", 2 ** 31 + 5), (b"G", 2 ** 24 + 1))
HEAD, TAIL = b"@deep\n", b"\n+\n\n"
TABLES = ((13, False), (32, False), (21, True), (32, True))            # (k, canonical)
SAT = 2 ** 32 - 2
UNITS = 208                                                            # units of depth SAT for the keep rule
TARGETS = (20, 2 ** 31, 2 ** 32 - 1)                                   # (the last one: the largest the options accept)
MAX_BINS = 1 << 20                                                     # SCFQ_NORM_MAX_BINS
WEAK_BELOW_MAX = 2 ** 32 - 1
# the calls of fq-normalize per table: every target with the smallest histogram, the middle one with the largest too, the largest weak_below
CALLS = [dict(target=t, seed=s, bins=2) for t, s in zip(TARGETS, (0, 7, 0))] + [dict(target=TARGETS[1], seed=7, bins=MAX_BINS),
                                                                                dict(weak_below=WEAK_BELOW_MAX, bins=2)]
LINE = sum(n for _, n in RUNS) + len(RUNS) - 1
INPUT_BYTES = len(HEAD) + LINE + len(TAIL)


def run_offsets():
    """[(letter, first byte, length)] of the runs in the input"""
    out, at = [], len(HEAD)
    for letter, n in RUNS:
        out.append((letter, at, n))
        at += n + 1
    return out


def table_of(k, canonical, runs=RUNS):
    """{key: count}: L - k + 1 windows per run; in canonical mode A and T share key 0 and C and G the key of k x C"""
    table = {}
    for letter, n in runs:
        key = index_of(({b"T": b"A", b"G": b"C"}.get(letter, letter) if canonical else letter) * k)
        table[key] = table.get(key, 0) + n - k + 1
    return table


def summary_of(k, canonical):
    """the fields of scfq_kcount_summary that the arithmetic gives"""
    table = table_of(k, canonical)
    windows = LINE - k + 1
    return dict(reads=1, lines=4, input_bytes=INPUT_BYTES, k=k, flags=1 if canonical else 0, windows=windows, kmers=sum(table.values()),
                skipped=(len(RUNS) - 1) * k, short_lines=0, distinct=len(table), unique=0, max_count=max(table.values()))


def reads_of(k):
    """{name: sequence}: the shapes, then UNITS reads of one saturated window each"""
    other = source(k, 2 * k + 8, b"deep")                              # no homopolymer of k letters: every window of it is absent
    assert all(len(set(other[i:i + k])) > 1 for i in range(len(other) - k + 1))
    a, t, c, g = (x * (k + 10) for x in (b"A", b"T", b"C", b"G"))
    shapes = {
        "all saturated, A": a,
        "all saturated, T": t,                                         # (k = 32, plain: the key without a slot)
        "saturated beside markers": a[:k + 5] + b"N" + a[:k + 3] + b"n" + t[:k + 2],
        "median C, maximum saturated": a[:k + 3] + b"N" + c[:k + 6],
        "median G": g[:k + 6] + b"N" + a[:k + 3],
        "median 0, maximum saturated": a[:k + 2] + b"N" + other[:k + 8],
        "all absent": other,
        "long, median C": (b"A" * 300 + b"N" + b"C" * 400 + b"N") * 4,
        "long, median saturated": (b"T" * 500 + b"N" + b"C" * 250 + b"N") * 4 + b"A" * 40,
    }
    return shapes


def fastq_reads(k):
    shapes = reads_of(k)
    return fastq_of([(s, b"\n") for s in shapes.values()] + [((b"A" if i % 2 else b"T") * k, b"\n") for i in range(UNITS)], final=True)

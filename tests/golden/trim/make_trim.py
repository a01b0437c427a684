"""Writes the fixtures of fq-trim next to itself: the inputs r1.fq, r2.fq, interleaved.fq (the same pairs, mates alternating) and
r2.fq.gz, and what the checker tests/_trim_check.trim_of makes of them with the parameters PARAMS below: single.fq (r1.fq as
single-end reads), paired1.fq and paired2.fq (r1.fq with r2.fq) and interleaved_out.fq.  Seeded: every run writes the same bytes.
The mix: fragments whose mates overlap, fragments shorter than a read (both mates read through into the adapters), fragments too long
to overlap, poly-G tails, quality that falls along the read, and a few mates too short to keep.

    python tests/golden/trim/make_trim.py
"""
import gzip
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from _trim_check import trim_of      # noqa: E402

READ = 100
PARAMS = dict(poly_g=10, window_quality=20)
ADAPTER1 = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCACGATCTCGTATGCCGTCTTCTGCTTG" + "A" * 60      # what mate 1 reads behind a short fragment
ADAPTER2 = "AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGTAGATCTCGGTGGTCGCCGTATCATT" + "A" * 60
COMP = str.maketrans("ACGT", "TGCA")


def revcomp(s):
    return s.translate(COMP)[::-1]


def main():
    rng = random.Random(20261020)

    def dna(n):
        return "".join(rng.choice("ACGT") for _ in range(n))

    def quality(n, falls):
        """high all along, or falling to '#' over the last third"""
        q = [rng.randrange(30, 41) for _ in range(n)]
        if falls:
            start = rng.randrange(n // 2, n - 4)
            for i in range(start, n):
                q[i] = rng.randrange(2, 12)
        return "".join(chr(33 + v) for v in q)

    pairs = []
    for i in range(56):
        kind = i % 7
        la, lb = (READ, READ) if i % 4 else (rng.randrange(60, READ + 1), rng.randrange(60, READ + 1))
        if kind in (0, 1):                              # the mates overlap
            size = rng.randrange(max(la, lb), la + lb - 29)
        elif kind in (2, 3):                            # shorter than a read: read-through, the adapter follows
            size = rng.randrange(10 if i % 3 == 0 else 35, min(la, lb))
        else:                                           # too long to overlap
            size = rng.randrange(la + lb + 1, 400)
        frag = dna(size)
        m1 = (frag + ADAPTER1)[:la]
        m2 = (revcomp(frag) + ADAPTER2)[:lb]
        if kind == 4:                                   # the dark cycles at the end of mate 2
            g = rng.randrange(8, 30)
            m2 = m2[:lb - g] + "G" * g
        if kind == 5:                                   # a partial adapter at the very end of mate 1
            k = rng.randrange(4, 12)
            m1 = m1[:la - k] + ADAPTER1[:k]
        pairs.append((m1, quality(la, kind == 6 or i % 9 == 0), m2, quality(lb, kind == 6)))

    def record(name, seq, qual):
        return "@%s\n%s\n+\n%s\n" % (name, seq, qual)

    r1 = "".join(record("pair%d/1" % i, p[0], p[1]) for i, p in enumerate(pairs))
    r2 = "".join(record("pair%d/2" % i, p[2], p[3]) for i, p in enumerate(pairs))
    both = "".join(record("pair%d/1" % i, p[0], p[1]) + record("pair%d/2" % i, p[2], p[3]) for i, p in enumerate(pairs))
    r1, r2, both = r1.encode(), r2.encode(), both.encode()
    single = trim_of(r1, **PARAMS)
    two = trim_of(r1, r2, **PARAMS)
    one = trim_of(both, interleaved=True, **PARAMS)
    for name, data in (("r1.fq", r1), ("r2.fq", r2), ("interleaved.fq", both), ("single.fq", single["out1"]), ("paired1.fq", two["out1"]),
                       ("paired2.fq", two["out2"]), ("interleaved_out.fq", one["out1"])):
        with open(os.path.join(HERE, name), "wb") as f:
            f.write(data)
    with open(os.path.join(HERE, "r2.fq.gz"), "wb") as raw:
        with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
            f.write(r2)
    for what, w in (("single", single), ("paired", two), ("interleaved", one)):
        print(what, {k: w[k] for k in ("reads_in", "reads_out", "dropped_reads", "cut_overlap", "cut_adapter", "cut_polyg", "cut_quality", "adapter_reads")})


if __name__ == "__main__":
    main()

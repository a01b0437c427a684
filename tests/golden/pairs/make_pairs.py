"""Writes the paired-end fixtures of fq-insert-size next to itself: r1.fq, r2.fq, interleaved.fq (the same pairs, mates alternating)
and r2.fq.gz.  Seeded: every run writes the same bytes.  The mix: fragments of a planted length whose mates overlap, fragments shorter
than a read (both mates read through into the adapters), fragments too long to overlap, and mates of unrelated sequence; a few bases
of some mates are turned into sequencing errors or N.

    python tests/golden/pairs/make_pairs.py
"""
import gzip
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
READ = 150
ADAPTER1 = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCACGATCTCGTATGCCGTCTTCTGCTTG" + "A" * 120      # what mate 1 reads behind a short fragment
ADAPTER2 = "AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGTAGATCTCGGTGGTCGCCGTATCATT" + "A" * 120
COMP = str.maketrans("ACGT", "TGCA")


def revcomp(s):
    return s.translate(COMP)[::-1]


def main():
    rng = random.Random(20261019)

    def dna(n):
        return "".join(rng.choice("ACGT") for _ in range(n))

    def damage(s, k):
        s = list(s)
        for _ in range(k):
            i = rng.randrange(len(s))
            s[i] = rng.choice("ACGTN")
        return "".join(s)

    pairs = []
    for i in range(88):
        kind = i % 8
        la, lb = (READ, READ) if i % 5 else (rng.randrange(100, READ + 1), rng.randrange(100, READ + 1))
        if kind == 7:                                   # unrelated mates
            m1, m2 = dna(la), dna(lb)
        else:
            if kind in (0, 1, 2, 3):                    # the mates overlap
                size = rng.randrange(max(la, lb), la + lb - 29)
            elif kind in (4, 5):                        # shorter than a read: read-through
                size = rng.randrange(20, min(la, lb))
            else:                                       # too long to overlap
                size = rng.randrange(la + lb + 1, 600)
            frag = dna(size)
            m1 = (frag + ADAPTER1)[:la]
            m2 = (revcomp(frag) + ADAPTER2)[:lb]
            if kind in (1, 5):
                m1, m2 = damage(m1, rng.randrange(0, 4)), damage(m2, rng.randrange(0, 4))
        pairs.append((m1, m2))

    def record(name, seq):
        return "@%s\n%s\n+\n%s\n" % (name, seq, "I" * len(seq))

    r1 = "".join(record("pair%d/1" % i, m1) for i, (m1, _) in enumerate(pairs))
    r2 = "".join(record("pair%d/2" % i, m2) for i, (_, m2) in enumerate(pairs))
    both = "".join(record("pair%d/1" % i, m1) + record("pair%d/2" % i, m2) for i, (m1, m2) in enumerate(pairs))
    for name, text in (("r1.fq", r1), ("r2.fq", r2), ("interleaved.fq", both)):
        with open(os.path.join(HERE, name), "wb") as f:
            f.write(text.encode())
    with open(os.path.join(HERE, "r2.fq.gz"), "wb") as raw:
        with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
            f.write(r2.encode())


if __name__ == "__main__":
    main()

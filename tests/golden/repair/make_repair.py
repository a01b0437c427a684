"""Writes the fq-repair fixture of this directory: two files that are out of step and what `sc fq-repair` has to make of them.

    python tests/golden/repair/make_repair.py

160 fragments of random sequence, 30 .. 90 bases a mate, named frag<p>.  The header of mate m is "@frag<p> <m>:N:0:ACGT", so the comments
of two mates differ; by the fragment's number p:
  p % 10 == 1           "@frag<p>/1" and "@frag<p>/2" instead: the suffix form
  p == TAB              "@frag<p>\\tlane=3" in both files: the name ends at a tab
  p in REPEATED         the name "twice": three records in R1 (33, 34, 35), two in R2 (33, 34); R2's third is dropped
  p == ONLY_SUFFIX      "@/1" and "@/2": a name that is only the suffix, the empty name
  p % 13 == 5           dropped from R1
  p % 11 == 7           dropped from R2
  p in BLOCK            R2's records of that stretch stand in a shuffled order
The last record of every file has no final newline; no line ends in CR LF.
Files: r1.fq, r2.fq, r2.fq.gz, and from the plain checker (tests/_repair_check.py, never from the library) out1.fq, out2.fq, singles1.fq,
singles2.fq, report.tsv (the header and the row) and per_read.tsv (with its header).  Deterministic: a linear congruential generator of
its own."""
import gzip
import io
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from _repair_check import STATS_HEADER, per_read_text, repair_of, stats_text      # noqa: E402

FRAGMENTS = 160
TAB = 20
REPEATED = (33, 34, 35)
ONLY_SUFFIX = 42
BLOCK = range(100, 120)


class Lcg:
    def __init__(self, seed):
        self.x = seed

    def below(self, n):
        self.x = (self.x * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        return (self.x >> 33) % n


def header_of(p, m):
    if p in REPEATED:
        return b"@twice %d:N:0:ACGT" % m
    if p == ONLY_SUFFIX:
        return b"@/%d" % m
    if p == TAB:
        return b"@frag%d\tlane=3" % p
    if p % 10 == 1:
        return b"@frag%d/%d" % (p, m)
    return b"@frag%d %d:N:0:ACGT" % (p, m)


def in_r1(p):
    return p % 13 != 5


def in_r2(p):
    return p % 11 != 7 and p != REPEATED[2]


def make_records():
    """per fragment the two records, and R2's order"""
    rng = Lcg(20261101)
    recs = []
    for p in range(FRAGMENTS):
        mates = []
        for m in (1, 2):
            n = 30 + rng.below(61)
            seq = bytes(b"ACGT"[rng.below(4)] for _ in range(n))
            qual = bytes(33 + 2 + rng.below(39) for _ in range(n))
            mates.append(header_of(p, m) + b"\n" + seq + b"\n+\n" + qual + b"\n")
        recs.append(tuple(mates))
    order = list(range(FRAGMENTS))
    block = list(BLOCK)
    for k in range(len(block) - 1, 0, -1):
        j = rng.below(k + 1)
        block[k], block[j] = block[j], block[k]
    order[BLOCK.start:BLOCK.stop] = block
    return recs, order


def make_files():
    """{name: bytes} of everything this directory holds, and the checker's result"""
    recs, order = make_records()
    r1 = b"".join(recs[p][0] for p in range(FRAGMENTS) if in_r1(p))[:-1]
    r2 = b"".join(recs[p][1] for p in order if in_r2(p))[:-1]
    files = {"r1.fq": r1, "r2.fq": r2}
    raw = io.BytesIO()
    with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
        f.write(r2)
    files["r2.fq.gz"] = raw.getvalue()
    w = repair_of(r1, r2)
    files.update({"out1.fq": w["out1"], "out2.fq": w["out2"], "singles1.fq": w["singles1_out"], "singles2.fq": w["singles2_out"],
                  "report.tsv": (STATS_HEADER + "\n" + stats_text(w) + "\n").encode(), "per_read.tsv": per_read_text(w, header=True).encode()})
    return files, w


def main():
    files, w = make_files()
    for name, data in files.items():
        with open(os.path.join(HERE, name), "wb") as f:
            f.write(data)
    print({k: w[k] for k in ("reads1", "reads2", "pairs", "singles1", "singles2", "moved", "in_step", "repeated1", "repeated2")})
    return 0


if __name__ == "__main__":
    sys.exit(main())

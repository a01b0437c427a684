"""Writes the fq-rmdup fixture of this directory: the reads and what `sc fq-rmdup --prefix=50 --swapped` has to make of them.

    python tests/golden/rmdup/make_rmdup.py

150 pairs of random sequence, 40 .. 120 bases a mate.  By the pair's number p (q is the pair the plant refers to, one with p % 7 == 0 and
mates of 60 bases or more); the plants by p % 14 stand among the first 60 pairs:
  p = 61, 63 .. 139     the forty pairs of one class: copies of pair 61, every second pair of that stretch
  p in ALL_G            both mates 100 G: the reads a two-colour instrument writes without signal
  p % 14 == 2           an exact duplicate of q = p - 2 under another name and with other qualities
  p % 14 == 9           q = p - 2 with its mates exchanged: a duplicate with --swapped only
  p % 14 == 3 / 10      mate 1 / mate 2 of q = p - 3, the other mate its own: equal in one mate only, never a duplicate
  p % 14 == 4           the first 50 bases of both mates of q = p - 4, then tails of its own: a duplicate with --prefix=50 and below
  p % 14 == 11          mate 1 is the first 30 bases of q = p - 4's, a proper prefix; mate 2 is q's: never a duplicate
The last record of every file has no final newline; no line ends in CR LF.
Files: r1.fq, r2.fq, r2.fq.gz, interleaved.fq (the same pairs, mates alternating), and from the plain checker (tests/_rmdup_check.py, never
from the library) out1.fq, out2.fq, report.tsv (the header and the row), hist.tsv (--hist, with its header) and per_read.tsv (with its
header).  Deterministic: a linear congruential generator of its own."""
import gzip
import io
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from _rmdup_check import STATS_HEADER, hist_text, per_read_text, rmdup_of, stats_text      # noqa: E402

PAIRS = 150
PREFIX = 50
RULES_BELOW = 60                                   # the plants by p % 14
BIG = list(range(61, 140, 2))
ALL_G = [60, 80, 100, 120, 140, 148]


class Lcg:
    def __init__(self, seed):
        self.x = seed

    def below(self, n):
        self.x = (self.x * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        return (self.x >> 33) % n


def make_seqs():
    rng = Lcg(20261023)

    def random_seq(n):
        return bytes(b"ACGT"[rng.below(4)] for _ in range(n))

    seqs = []
    for p in range(PAIRS):
        low = 60 if p % 7 == 0 else 40
        seqs.append([random_seq(low + rng.below(121 - low)) for _ in range(2)])
    for p in range(PAIRS):
        r = p % 14 if p < RULES_BELOW else -1
        if p in BIG:
            seqs[p] = list(seqs[BIG[0]])
        elif p in ALL_G:
            seqs[p] = [b"G" * 100, b"G" * 100]
        elif r == 2:
            seqs[p] = list(seqs[p - 2])
        elif r == 9:
            seqs[p] = [seqs[p - 2][1], seqs[p - 2][0]]
        elif r == 3:
            seqs[p][0] = seqs[p - 3][0]
        elif r == 10:
            seqs[p][1] = seqs[p - 3][1]
        elif r == 4:
            for m in range(2):
                own = seqs[p][m][PREFIX:] or b"A"
                other = seqs[p - 4][m][PREFIX:PREFIX + 1]
                if own[:1] == other:                      # the first base behind the prefix differs for certain
                    own = bytes([b"ACGT"[(b"ACGT".index(own[:1]) + 1) % 4]]) + own[1:]
                seqs[p][m] = seqs[p - 4][m][:PREFIX] + own
        elif r == 11:
            seqs[p] = [seqs[p - 4][0][:30], seqs[p - 4][1]]
    return seqs, rng


def make_pairs():
    seqs, rng = make_seqs()
    pairs = []
    for p, mates in enumerate(seqs):
        texts = []
        for m, seq in enumerate(mates):
            qual = bytes(33 + 2 + rng.below(39) for _ in range(len(seq)))
            texts.append(b"@pair%d/%d\n%s\n+\n%s\n" % (p, m + 1, seq, qual))
        pairs.append(tuple(texts))
    return pairs


def make_files():
    """{name: bytes} of everything this directory holds, and the checker's result"""
    pairs = make_pairs()
    r1, r2 = b"".join(p[0] for p in pairs)[:-1], b"".join(p[1] for p in pairs)[:-1]
    files = {"r1.fq": r1, "r2.fq": r2, "interleaved.fq": b"".join(p[0] + p[1] for p in pairs)[:-1]}
    raw = io.BytesIO()
    with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
        f.write(r2)
    files["r2.fq.gz"] = raw.getvalue()
    w = rmdup_of(r1, r2, prefix=PREFIX, swapped=True)
    files.update({"out1.fq": w["out1"], "out2.fq": w["out2"], "report.tsv": (STATS_HEADER + "\n" + stats_text(w) + "\n").encode(),
                  "hist.tsv": hist_text(w, header=True).encode(), "per_read.tsv": per_read_text(w, header=True).encode()})
    return files, w


def main():
    files, w = make_files()
    for name, data in files.items():
        with open(os.path.join(HERE, name), "wb") as f:
            f.write(data)
    print({k: w[k] for k in ("units_in", "units_out", "duplicate_units", "duplicated_classes", "max_copies", "bases_in", "bases_out")})
    return 0


if __name__ == "__main__":
    sys.exit(main())

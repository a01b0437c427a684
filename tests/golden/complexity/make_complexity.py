"""Writes the fq-complexity fixture of this directory: the reads and what `sc fq-complexity --max-masked-pct=30` has to make of them.

    python tests/golden/complexity/make_complexity.py

150 pairs of 40 .. 120 bases of random sequence.  Every third read carries a planted unit of period 1 .. 6 repeated over 5 .. 60 bases at a
place of its own, every seventeenth an N, every nineteenth a stretch of lower case, pair 40 has a mate of 3 bases, pair 41 an empty one,
pair 42 a mate of 600 bases (too long: echoed), pair 43 a quality line shorter than its sequence.
Files: r1.fq, r2.fq, r2.fq.gz, interleaved.fq (the same pairs, mates alternating), and from the plain checker
(tests/_complexity_check.py, never from the library) out1.fq, out2.fq, report.tsv (the header and the row), hist.tsv (--hist, with its
header) and per_read.tsv (with its header).  Deterministic: a linear congruential generator of its own."""
import gzip
import io
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from _complexity_check import STATS_HEADER, complexity_of, hist_text, lengths_of, per_read_text, stats_text      # noqa: E402

PAIRS = 150
MAX_MASKED_PCT = 30


class Lcg:
    def __init__(self, seed):
        self.x = seed

    def below(self, n):
        self.x = (self.x * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        return (self.x >> 33) % n


def make_pairs():
    rng = Lcg(20261022)
    pairs, n = [], 0
    for p in range(PAIRS):
        mates = []
        for m in range(2):
            L = 40 + rng.below(81)
            seq = bytearray(b"ACGT"[rng.below(4)] for _ in range(L))
            if n % 3 == 0:
                unit = bytes(b"ACGT"[rng.below(4)] for _ in range(1 + rng.below(6)))
                run, at = 5 + rng.below(56), rng.below(L)
                seq[at:at + run] = (unit * 60)[:min(run, L - at)]
            if n % 17 == 5:
                seq[rng.below(L)] = ord("N")
            if n % 19 == 7:
                at = rng.below(L)
                seq[at:at + 9] = bytes(seq[at:at + 9]).lower()
            if (p, m) == (40, 1):
                seq = seq[:3]
            if (p, m) == (41, 0):
                seq = seq[:0]
            if (p, m) == (42, 1):
                seq = bytearray(b"ACGT"[rng.below(4)] for _ in range(600))
            qual = bytes(33 + 2 + rng.below(39) for _ in range(len(seq)))
            if (p, m) == (43, 0):
                qual = qual[:10]
            mates.append(b"@pair%d/%d\n%s\n+\n%s\n" % (p, m + 1, bytes(seq), qual))
            n += 1
        pairs.append(tuple(mates))
    return pairs


def make_files():
    """{name: bytes} of everything this directory holds, and the checker's result"""
    pairs = make_pairs()
    r1, r2 = b"".join(p[0] for p in pairs), b"".join(p[1] for p in pairs)
    files = {"r1.fq": r1, "r2.fq": r2, "interleaved.fq": b"".join(p[0] + p[1] for p in pairs)}
    raw = io.BytesIO()
    with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
        f.write(r2)
    files["r2.fq.gz"] = raw.getvalue()
    w = complexity_of(r1, r2, max_masked_pct=MAX_MASKED_PCT)
    assert w["too_long"] == 1 and 0 < w["low_reads"] < w["dropped_reads"] < w["reads_in"] // 2 and w["masked_bases_out"] > 0
    files.update({"out1.fq": w["out1"], "out2.fq": w["out2"], "report.tsv": (STATS_HEADER + "\n" + stats_text(w) + "\n").encode(),
                  "hist.tsv": hist_text(w, header=True).encode(), "per_read.tsv": per_read_text(w, lengths_of(r1, r2), header=True).encode()})
    return files, w


def main():
    files, w = make_files()
    for name, data in files.items():
        with open(os.path.join(HERE, name), "wb") as f:
            f.write(data)
    print({k: w[k] for k in ("reads_in", "reads_out", "low_reads", "dropped_reads", "masked_reads", "masked_bases", "max_score")})
    return 0


if __name__ == "__main__":
    sys.exit(main())

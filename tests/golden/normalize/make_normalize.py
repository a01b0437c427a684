"""Writes the fq-normalize fixture of this directory: the reads and what `sc fq-normalize --k=21 --target=20 --min-depth=3` has to make
of them.

    python tests/golden/normalize/make_normalize.py

Two "genomes" of 600 random bases, the first sampled at about 40 x and the second at about 6 x with pairs of 2 x 75 bases from
fragments of 180 .. 260 bases of either strand, 1 % substitution errors, an N in a few reads, and one pair that is shorter than k.
Files: r1.fq, r2.fq, r2.fq.gz, interleaved.fq (the same pairs, mates alternating), and from the plain checker
(tests/_normalize_check.py over _kcount_check.kcount_of, never from the library) out1.fq, out2.fq, report.tsv (the header and the row),
hist.tsv (--hist, 1002 bins, with its header) and per_read.tsv.  Deterministic: a linear congruential generator of its own."""
import gzip
import io
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from _kcount_check import kcount_of                                                                            # noqa: E402
from _normalize_check import HIGH, HIST_HEADER, KEPT, LOW, NO_KMERS, ROW_HEADER, hist_rows, normalize_of, per_read_rows, report_row      # noqa: E402

K, TARGET, MIN_DEPTH, BINS = 21, 20, 3, 1002
REGION, READ_LEN = 600, 75
PAIRS = (160, 24)              # per region: 2 * 75 * pairs / 600 = 40 x and 6 x


class Lcg:
    def __init__(self, seed):
        self.x = seed

    def below(self, n):
        self.x = (self.x * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        return (self.x >> 33) % n


COMP = bytes.maketrans(b"ACGT", b"TGCA")


def make_pairs():
    """[(region, r1 record, r2 record)] in the order of the files: the regions are shuffled into each other"""
    rng = Lcg(20261021)
    genomes = [bytes(b"ACGT"[rng.below(4)] for _ in range(REGION)) for _ in PAIRS]
    plan = [0] * PAIRS[0] + [1] * PAIRS[1]
    for i in range(len(plan) - 1, 0, -1):
        j = rng.below(i + 1)
        plan[i], plan[j] = plan[j], plan[i]
    pairs = []
    for p, region in enumerate(plan):
        frag_len = 180 + rng.below(81)
        at = rng.below(REGION - frag_len + 1)
        frag = genomes[region][at:at + frag_len]
        if rng.below(2):
            frag = frag.translate(COMP)[::-1]
        mates = []
        for seq in (bytearray(frag[:READ_LEN]), bytearray(frag[-READ_LEN:].translate(COMP)[::-1])):
            for q in range(READ_LEN):
                if rng.below(100) == 0:
                    seq[q] = b"ACGT"[(b"ACGT".index(seq[q]) + 1 + rng.below(3)) & 3]
                elif rng.below(1500) == 0:
                    seq[q] = ord("N")
            qual = bytes(33 + 2 + rng.below(39) for _ in range(READ_LEN))
            mates.append((bytes(seq), qual))
        if p == 100:                          # the pair that is shorter than k
            mates = [(s[:K - 1 - m], q[:K - 1 - m]) for m, (s, q) in enumerate(mates)]
        pairs.append((region,) + tuple(b"@pair%d/%d\n%s\n+\n%s\n" % (p, m + 1, s, q) for m, (s, q) in enumerate(mates)))
    return pairs


def make_files():
    """{name: bytes} of everything this directory holds, and the checker's result"""
    pairs = make_pairs()
    r1, r2 = b"".join(p[1] for p in pairs), b"".join(p[2] for p in pairs)
    files = {"r1.fq": r1, "r2.fq": r2, "interleaved.fq": b"".join(p[1] + p[2] for p in pairs)}
    raw = io.BytesIO()
    with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
        f.write(r2)
    files["r2.fq.gz"] = raw.getvalue()
    table = kcount_of([r1, r2], K, True).table
    w = normalize_of(table, K, True, r1, r2, target=TARGET, min_depth=MIN_DEPTH, bins=BINS)
    # all three drop classes, and kept units of both regions
    classes = w["classes"]
    assert {NO_KMERS, LOW, HIGH, KEPT} <= set(classes), sorted(set(classes))
    for region in (0, 1):
        assert any(c == KEPT for c, p in zip(classes, pairs) if p[0] == region), region
    assert sum(c == HIGH for c, p in zip(classes, pairs) if p[0] == 0) >= 5 and classes[100] == NO_KMERS
    assert sum(c == LOW for c, p in zip(classes, pairs) if p[0] == 1) >= 3
    assert any(r[0] < READ_LEN - K + 1 and r[0] > 0 for r in w["recs"])                       # a read with an N
    files.update({"out1.fq": w["out1"], "out2.fq": w["out2"], "report.tsv": (ROW_HEADER + "\n" + report_row(w) + "\n").encode(),
                  "hist.tsv": ("\n".join([HIST_HEADER] + hist_rows(w["hist"])) + "\n").encode(),
                  "per_read.tsv": ("\n".join(per_read_rows(w)) + "\n").encode()})
    return files, w


def main():
    files, w = make_files()
    for name, data in files.items():
        with open(os.path.join(HERE, name), "wb") as f:
            f.write(data)
    print({k: w[k] for k in ("units_in", "units_out", "dropped_no_kmers", "dropped_low", "dropped_high")})
    return 0


if __name__ == "__main__":
    sys.exit(main())

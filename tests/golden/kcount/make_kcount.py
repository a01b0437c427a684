"""Writes the fq-kcount fixture of this directory: reads.fq and the texts `sc fq-kcount` has to print for it.

    python tests/golden/kcount/make_kcount.py

A "genome" of 2000 random bases, sampled with 400 reads of 100 bases from either strand (about 20 x) with 1 % substitution errors
and an N now and then, so that the histogram at k = 21 has an error peak at 1 and a coverage peak in the teens.  The expected texts
come from the plain checker (tests/_kcount_check.py), never from the library: hist.txt (the default output), dump_min5.txt
(--dump --min-count=5), top10.txt (--top=10, with a tie across the cut) and totals.txt (--totals), all with --k=21 --canonical.
Deterministic: a linear congruential generator of its own."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from _kcount_check import dump_of, hist_text, kcount_of, rows_text, top_of, totals_text      # noqa: E402

K = 21
GENOME, READS, READ_LEN = 2000, 400, 100


class Lcg:
    def __init__(self, seed):
        self.x = seed

    def below(self, n):
        self.x = (self.x * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        return (self.x >> 33) % n


def make_reads():
    rng = Lcg(20261020)
    genome = bytes(b"ACGT"[rng.below(4)] for _ in range(GENOME))
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    parts = []
    for r in range(READS):
        at = rng.below(GENOME - READ_LEN + 1)
        seq = bytearray(genome[at:at + READ_LEN])
        if rng.below(2):
            seq = bytearray(bytes(seq).translate(comp)[::-1])
        for p in range(READ_LEN):
            if rng.below(100) == 0:
                seq[p] = b"ACGT"[(b"ACGT".index(seq[p]) + 1 + rng.below(3)) & 3]
            elif rng.below(1000) == 0:
                seq[p] = ord("N")
        qual = bytes(33 + 2 + rng.below(39) for _ in range(READ_LEN))
        parts.append(b"@read%d\n%s\n+\n%s\n" % (r, bytes(seq), qual))
    return b"".join(parts)


def expected(data):
    want = kcount_of(data, K, True)
    top = top_of(want.table, 11)
    assert top[9][1] == top[10][1], "the tenth and the eleventh count differ: no tie across the cut"
    return {"hist.txt": hist_text(want.table), "dump_min5.txt": rows_text(dump_of(want.table, 5), K), "top10.txt": rows_text(top[:10], K),
            "totals.txt": totals_text(want, K)}


def main():
    data = make_reads()
    with open(os.path.join(HERE, "reads.fq"), "wb") as f:
        f.write(data)
    for name, text in expected(data).items():
        with open(os.path.join(HERE, name), "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

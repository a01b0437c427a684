"""Writes the fixtures of fq-demux next to itself.  Seeded, and made of random letters only: every run writes the same bytes.
sheet.tsv: four samples with two barcodes each (a comment line and a blank line among them); `alpha` and `beta` are at Hamming distance 2 in
barcode1 and share barcode2, `delta` has a barcode1 of 6 letters whose first 4 are not `gamma`'s.  Reads: r1.fq, r2.fq, interleaved.fq
(the same pairs, mates alternating), r2.fq.gz; 48 bases behind the barcode.  The barcodes are inline: barcode1 opens mate 1, barcode2
mate 2.  Planted among perfect pairs: one substitution in either barcode, one in each, two in one (unmatched with the default of one
mismatch), an N and a lower-case letter in a barcode, the barcode half way between alpha and beta (ambiguous), random barcodes, a mate
shorter than every barcode (no_barcode) and one exactly as long as its barcode (an empty sequence line).  What
tests/_demux_check.demux_of makes of them with the defaults: <sample>_R1.fq / <sample>_R2.fq, undetermined_R1.fq / _R2.fq and report.tsv
(the rows of the command for r1.fq with r2.fq, with its header).

    python tests/golden/demux/make_demux.py
"""
import gzip
import io
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from _demux_check import REPORT_HEADER, demux_of, report_text      # noqa: E402

READ = 48
PAIRS = 120
SAMPLES = (("alpha", "ACGTACGT", "TTGACCAG"), ("beta", "ACGAACGA", "TTGACCAG"), ("gamma", "GGATCCTA", "CATGGTCA"), ("delta", "TCAGGA", "AGCTTGCA"))
SHEET = "# sample\tbarcode1\tbarcode2\n" + "".join("%s\t%s\t%s\n" % s for s in SAMPLES[:2]) + "\n" + "".join("%s\t%s\t%s\n" % s for s in SAMPLES[2:])


def build():
    """file name -> bytes, and the checker's result for r1.fq with r2.fq"""
    rng = random.Random(20261020)

    def dna(n):
        return "".join(rng.choice("ACGT") for _ in range(n))

    def sub(bc, k=1):
        bc = list(bc)
        for i in rng.sample(range(len(bc)), k):
            bc[i] = rng.choice([b for b in "ACGT" if b != bc[i]])
        return "".join(bc)

    def quality(n):
        return "".join(chr(33 + rng.randrange(25, 41)) for _ in range(n))

    pairs = []
    for i in range(PAIRS):
        _, b1, b2 = SAMPLES[rng.randrange(4)]
        kind = i % 20
        m1, m2 = b1 + dna(READ), b2 + dna(READ)
        if kind == 3:
            m1 = sub(b1) + m1[len(b1):]
        elif kind == 5:
            m2 = sub(b2) + m2[len(b2):]
        elif kind == 7:
            m1, m2 = sub(b1) + m1[len(b1):], sub(b2) + m2[len(b2):]
        elif kind == 9:
            m1 = sub(b1, 2) + m1[len(b1):]
        elif kind == 11:
            m1 = b1[:2] + "N" + b1[3:] + m1[len(b1):]
        elif kind == 13:
            m2 = b2[:4] + b2[4].lower() + b2[5:] + m2[len(b2):]
        elif kind == 15:
            m1, m2 = "ACGTACGA" + dna(READ), "TTGACCAG" + dna(READ)      # one letter from alpha, one from beta
        elif kind == 17:
            m1, m2 = dna(8 + READ), dna(8 + READ)
        elif kind == 19 and i % 40 == 19:
            m1 = dna(5)
        elif kind == 19:
            m1 = b1
        pairs.append((m1, quality(len(m1)), m2, quality(len(m2))))

    def record(name, seq, qual):
        return "@%s\n%s\n+\n%s\n" % (name, seq, qual)

    r1 = "".join(record("pair%d/1" % i, p[0], p[1]) for i, p in enumerate(pairs)).encode()
    r2 = "".join(record("pair%d/2" % i, p[2], p[3]) for i, p in enumerate(pairs)).encode()
    both = "".join(record("pair%d/1" % i, p[0], p[1]) + record("pair%d/2" % i, p[2], p[3]) for i, p in enumerate(pairs)).encode()
    files = {"sheet.tsv": SHEET.encode(), "r1.fq": r1, "r2.fq": r2, "interleaved.fq": both}
    two = demux_of(r1, r2, SAMPLES)
    for d, row in enumerate(two["rows"]):
        name = SAMPLES[d][0] if d < len(SAMPLES) else "undetermined"
        files[name + "_R1.fq"] = two["out1"][row["off1"]:row["off1"] + row["bytes1"]]
        files[name + "_R2.fq"] = two["out2"][row["off2"]:row["off2"] + row["bytes2"]]
    files["report.tsv"] = ("\n".join([REPORT_HEADER] + report_text(two, SAMPLES)) + "\n").encode()
    raw = io.BytesIO()
    with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
        f.write(r2)
    files["r2.fq.gz"] = raw.getvalue()
    return files, two


def main():
    files, two = build()
    for name, data in files.items():
        with open(os.path.join(HERE, name), "wb") as f:
            f.write(data)
    print({k: two[k] for k in ("units_in", "assigned", "perfect", "mismatched", "no_barcode", "unmatched", "ambiguous", "bases_clipped")})
    print([r["units"] for r in two["rows"]], {n: len(d) for n, d in files.items()})


if __name__ == "__main__":
    main()

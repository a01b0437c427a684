"""Writes the fixtures of fq-screen next to itself.  Seeded, and made of random letters only: every run writes the same bytes.
References: spike.fa (three contigs, lower-case stretches, runs of N, "\\r\\n" line ends), vector.fa and rrna.fa (one contig each, the two
share a stretch of 200 bases).  Reads: r1.fq, r2.fq, interleaved.fq (the same pairs, mates alternating), r2.fq.gz; 100 bases a read.
Planted among random pairs: stretches of a reference forward and reverse-complemented, in one mate only, a read across two contigs of
spike.fa (no window crosses), reads with one N in the middle, a read from the shared stretch (two references match), and reads with
exactly min_hits - 1 and min_hits k-mers of a reference.  What tests/_screen_check.screen_of makes of them with PARAMS: out1.fq / out2.fq,
interleaved_out.fq and report.tsv (the rows of the command for r1.fq with r2.fq).

    python tests/golden/screen/make_screen.py
"""
import gzip
import io
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from _screen_check import REPORT_HEADER, index_of, report_rows, screen_of      # noqa: E402

READ = 100
K = 31
PARAMS = dict(min_hits=3)
NAMES = ("spike", "vector", "rrna")
COMP = str.maketrans("ACGT", "TGCA")


def revcomp(s):
    return s.translate(COMP)[::-1]


def build():
    """file name -> bytes"""
    rng = random.Random(20261019)

    def dna(n):
        return "".join(rng.choice("ACGT") for _ in range(n))

    def other(base):
        return rng.choice([b for b in "ACGT" if b != base])

    def fasta(contigs, width, eol):
        return "".join(">%s some text\n".replace("\n", eol) % name + "".join(seq[i:i + width] + eol for i in range(0, len(seq), width)) for name, seq in contigs)

    # spike: soft-masked stretches, runs of N, three contigs (the last one exactly K bases), CRLF
    c1, c2, c3 = dna(1500), dna(900), dna(K)
    spike_clean = [c1, c2, c3]
    c1m = c1[:300] + c1[300:420].lower() + c1[420:700] + "N" * 25 + c1[725:]
    c2m = c2[:100].lower() + c2[100:500] + "NNN" + c2[503:]
    spike = fasta((("spike_1", c1m), ("spike_2", c2m), ("spike_3", c3)), 60, "\r\n")
    shared = dna(200)
    vec, rrna = dna(800) + shared + dna(1000), dna(1200) + shared + dna(1100)
    vector = fasta((("vector", vec),), 70, "\n")
    rrna_fa = fasta((("rrna", rrna),), 80, "\n")[:-1]      # (no final newline)

    def quality(n):
        return "".join(chr(33 + rng.randrange(25, 41)) for _ in range(n))

    def with_hits(ref, at, hits):
        """a read with exactly `hits` k-mers of ref: K + hits - 1 of its bases from `at`, between letters that differ from the reference's"""
        core = ref[at:at + K + hits - 1]
        left = (READ - len(core)) // 2
        read = dna(left - 1) + other(ref[at - 1]) + core + other(ref[at + len(core)])
        return read + dna(READ - len(read))

    pairs = []
    for i in range(32):
        kind = i % 16
        m1, m2 = dna(READ), dna(READ)
        if kind == 1:                                   # both mates from the spike-in, as a fragment: forward and reverse complement
            at = rng.randrange(0, 150)
            m1, m2 = c1[at:at + READ], revcomp(c1[at + 80:at + 180])
        elif kind == 2:                                 # mate 1 only, the soft-masked stretch
            m1 = c1[310:410]
        elif kind == 3:                                 # mate 2 only, reverse complement, the vector
            at = rng.randrange(0, 600)
            m2 = revcomp(vec[at:at + READ])
        elif kind == 4:                                 # across two contigs: the end of spike_1 and the start of spike_2
            m1 = c1[-50:] + c2[:50]
        elif kind == 5:                                 # one N in the middle of a read from rrna
            at = rng.randrange(0, 1000)
            m1 = rrna[at:at + 50] + "N" + rrna[at + 51:at + READ]
        elif kind == 6:                                 # the shared stretch: vector and rrna both match
            m2 = shared[40:140]
        elif kind == 7:                                 # exactly min_hits - 1 k-mers: no match
            m1 = with_hits(vec, rng.randrange(10, 700), PARAMS["min_hits"] - 1)
        elif kind == 8:                                 # exactly min_hits
            m1 = with_hits(vec, rng.randrange(10, 700), PARAMS["min_hits"])
        elif kind == 9:                                 # the third contig, all of it and nothing more
            m2 = dna(30) + other(c3[0]) + c3 + dna(READ - 32 - K)
        elif kind == 10 and i % 32 == 10:               # a short pair and a lower-case read
            m1, m2 = dna(K - 1), c1[500:600].lower()
        elif kind == 11:                                # across the run of N of spike_1: the reference has no k-mer there
            m1 = c1[660:760]
        pairs.append((m1, quality(len(m1)), m2, quality(len(m2))))

    def record(name, seq, qual):
        return "@%s\n%s\n+\n%s\n" % (name, seq, qual)

    r1 = "".join(record("pair%d/1" % i, p[0], p[1]) for i, p in enumerate(pairs)).encode()
    r2 = "".join(record("pair%d/2" % i, p[2], p[3]) for i, p in enumerate(pairs)).encode()
    both = "".join(record("pair%d/1" % i, p[0], p[1]) + record("pair%d/2" % i, p[2], p[3]) for i, p in enumerate(pairs)).encode()
    files = {"spike.fa": spike.encode(), "vector.fa": vector.encode(), "rrna.fa": rrna_fa.encode(), "r1.fq": r1, "r2.fq": r2, "interleaved.fq": both}
    index = index_of([(n, files[n + ".fa"]) for n in NAMES], K)
    two, one = screen_of(index, r1, r2, **PARAMS), screen_of(index, both, interleaved=True, **PARAMS)
    files.update({"out1.fq": two["out1"], "out2.fq": two["out2"], "interleaved_out.fq": one["out1"],
                  "report.tsv": ("\n".join([REPORT_HEADER] + report_rows(two, index)) + "\n").encode()})
    raw = io.BytesIO()
    with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
        f.write(r2)
    files["r2.fq.gz"] = raw.getvalue()
    return files, index, two


def main():
    files, index, two = build()
    for name, data in files.items():
        with open(os.path.join(HERE, name), "wb") as f:
            f.write(data)
    print({k: index[k] for k in ("distinct", "slots")}, index["refs"])
    print({k: two[k] for k in ("reads_in", "reads_out", "matched_reads", "matched_pairs", "multi_reads", "short_reads", "ref_reads", "ref_only_reads", "skipped")})


if __name__ == "__main__":
    main()

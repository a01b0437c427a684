"""The case set of the sweep over every k (test_gpu_every_k.py) and its proof on the host (test_every_k_cases_host.py): cases(k) is
one small FASTQ, deterministic from k, that holds what the k-dependent shifts, masks and loop shapes of fq-kmers, fq-kcount, fq-screen
and fq-normalize can get wrong, and two references cut from the same source for fq-screen.  The parts, each a list of (sequence, line
end) in the order of the records:

    invalid   a read of 2k + 1 letters with one invalid letter at position p, one read per p = 0 .. 2k, 'N' and lower case in turn
    edges     T x (k + 20), A x (k + 20); a reverse-complement palindrome (even k) or a k-mer and its reverse complement in two reads
              (odd k); a read whose consecutive windows are in turn smaller forwards and smaller as reverse complement; k-mers that
              begin with T and end with A (k >= 2); C x 300
    lengths   sequence lines of every length of line_lengths(k), each once with "\\n" and once with "\\r\\n", cut from the source one
              behind the other, so the two copies of a length are the same text

The last record lacks its final newline."""
import hashlib

COMP = bytes.maketrans(b"ACGT", b"TGCA")
SOURCE = 6144
OFFSETS = (0, 5, 11)                      # of the device pointer from a 16-byte boundary
NORM_OPTS = dict(target=3, min_depth=2)   # fq-normalize against the set's own table: kept, low, high and no_kmers all occur


def revcomp(s):
    return s.translate(COMP)[::-1]


def source(k, n=SOURCE, salt=b""):
    """n letters of A C G T from SHA-256 over (k, salt, counter): two bits a letter"""
    out = bytearray()
    i = 0
    while len(out) < n:
        for byte in hashlib.sha256(b"every k %d %s %d" % (k, salt, i)).digest():
            out += bytes(b"ACGT"[(byte >> s) & 3] for s in (0, 2, 4, 6))
        i += 1
    return bytes(out[:n])


def line_lengths(k):
    out = []
    for n in (0, k - 1, k, k + 1, 2 * k - 1, 2 * k, 15, 16, 17, 27, 28, 29, 46, 47, 48, 49, 63, 64, 65, 127, 128, 129, 510 + k, 511 + k, 512 + k):
        if n not in out:
            out.append(n)
    return out


def forward_is_smaller(w):
    """True / False, None for a palindrome"""
    r = revcomp(w)
    return None if r == w else w < r              # (A < C < G < T as bytes and as codes)


def alternating(k):
    """k + m - 1 letters whose m windows are in turn smaller forwards and smaller as reverse complement; m = 6, but 3 at k = 2, where
    forwards is smaller iff the two codes sum to less than 3 and no run is longer (A G G A)"""
    s = source(k, 1 << 15, b"alternating")
    m = 6 if k != 2 else 3
    for at in range(len(s) - k - m):
        kinds = [forward_is_smaller(s[at + i:at + i + k]) for i in range(m)]
        if None not in kinds and all(kinds[i] != kinds[i + 1] for i in range(m - 1)):
            return s[at:at + k + m - 1]
    raise AssertionError("no alternating read at k = %d" % k)


class Cases:
    def __init__(self, k):
        g = source(k)
        self.k, self.source = k, g
        # ---- one invalid letter at every position
        base = g[3000:3000 + 2 * k + 1]
        invalid = []
        for p in range(2 * k + 1):
            r = bytearray(base)
            r[p] = ord("N") if p % 2 == 0 else r[p] | 0x20
            invalid.append((bytes(r), b"\n"))
        # ---- key edges
        self.t_run, self.a_run, self.c_run = b"T" * (k + 20), b"A" * (k + 20), b"C" * 300
        if k % 2 == 0:
            half = g[3200:3200 + k // 2]
            self.palindrome = [half + revcomp(half)]
        else:
            w = g[3200:3200 + k]
            if revcomp(w) == w:                   # (k = 1 has no palindrome; nor has any odd k)
                raise AssertionError(w)
            self.palindrome = [w, revcomp(w)]
        self.alternating = alternating(k)
        self.t_to_a = [b"T" + g[3300 + 40 * i:3300 + 40 * i + k - 2] + b"A" for i in range(3)] if k >= 2 else []
        edges = [(s, b"\n") for s in [self.t_run, self.a_run] + self.palindrome + [self.alternating] + self.t_to_a + [self.c_run]]
        # ---- lengths: the reads lie one behind the other in the source's first half
        lengths, at = [], 0
        for n in line_lengths(k):
            assert at + n <= 3000
            lengths += [(g[at:at + n], b"\n"), (g[at:at + n], b"\r\n")]
            at += n
        self.lengths_end = at
        self.parts = dict(invalid=invalid, edges=edges, lengths=lengths)
        self.fastq = fastq_of([r for part in self.parts.values() for r in part])
        # ---- fq-screen: `one` holds the source's letters 400 .. 1600 wrapped at 70 columns, the palindrome, the T run and the read
        # under the invalid letters, `two` the source's first 800 letters and the A run: the short reads at the source's start hit
        # `two`, the reads of the invalid part `one`, those over 400 .. 800 and the runs both, the edges' single k-mers none
        one = b">g wrapped\n" + b"\n".join(g[i:min(i + 70, 1600)] for i in range(400, 1600, 70)) + b"\n>palindrome\n" + b"".join(self.palindrome[:1]) + \
            b"\n>t\n" + self.t_run + b"\n>under the invalid letters\n" + base + b"\n"
        two = b">g\n" + g[:800] + b"\n>a\n" + self.a_run + b"\n"
        self.refs = [("one", one), ("two", two)]


def fastq_of(reads, final=False):
    """records "@<i>" of (sequence, line end); final: the last line has its line end"""
    data = b"".join(b"@%d" % i + eol + s + eol + b"+" + eol + b"I" * len(s) + eol for i, (s, eol) in enumerate(reads))
    return data if final or not reads else data[:len(data) - len(reads[-1][1])]


_cases = {}


def cases(k):
    if k not in _cases:
        _cases[k] = Cases(k)
    return _cases[k]

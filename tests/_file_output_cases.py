"""Inputs whose outputs pass one, and two, chunks of the writer every read-producing command shares (csrc/scfq_fdwrite.hpp: two
pinned buffers of kChunk bytes, picked by k & 1), and what the commands owe for them.

The layout and the expectations are tests/_big_offset_cases.py's: an input is block x R + tail, the expectation is the checker's result
on the block and on the tail, composed.  Here R is small.  For every command it is the smallest R with
  - every output the command writes longer than kChunk (a second issue(), the buffer with k & 1 == 1), and
  - at least one output longer than 2 * kChunk (a third chunk, which uses buffer 0 again),
computed from the checker's output lengths on the block and on the tail, never from the library.  kChunk is read from the header.
No command needs an input above MAX_INPUT bytes for this, so "every output" holds for all six without exception: fq-demux, whose
twelve files each get between an eighth and a fifth of the input, needs the largest one.

fq-trim with every step off echoes a well-formed LF input: `echo_input` pads the header of the last record so that the output has
one of EXACT_SIZES bytes.  tests/test_file_output_cases_host.py pins all of this without a GPU."""
import os
import re

import numpy as np

import _big_offset_cases as C
from conftest import GOLDEN, PKG
from _screen_check import contigs_of, index_of_np

NAMES = ("spike", "vector", "rrna")
FA = [os.path.join(GOLDEN, "screen", n + ".fa") for n in NAMES]
MAX_INPUT = 400 * 10 ** 6
TRIM_OFF = dict(no_adapters=True, no_overlap=True, min_length=0)      # (test_gpu_trim.py's OFF)
K, CANONICAL = 21, True                                               # of fq-normalize's given table
SEEDS = dict(single=20261101, paired=20261102, echo=20261103)


def chunk_bytes():
    """kChunk of csrc/scfq_fdwrite.hpp (a literal shifted by a literal)"""
    text = open(os.path.join(PKG, "csrc", "scfq_fdwrite.hpp")).read()
    m = re.search(r"static constexpr uint64_t kChunk = (\d+)ull << (\d+);", text)
    assert m, "kChunk is no longer a shifted literal in scfq_fdwrite.hpp"
    return int(m.group(1)) << int(m.group(2))


CHUNK = chunk_bytes()
EXACT_SIZES = (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1)
PIPE_SIZE = 2 * CHUNK + 1


def meets(lengths):
    """the two chunk conditions for the lengths of a command's outputs"""
    return all(n > CHUNK for n in lengths) and any(n > 2 * CHUNK for n in lengths)


def smallest_R(lengths_at, lo=1):
    """the smallest R >= lo whose output lengths lengths_at(R) meet both conditions"""
    R = lo
    while not meets(lengths_at(R)):
        R += 1
        assert R < 100_000
    return R


class Case:
    """a command's case.  inputs: [(block, tail)] per input file; R; want: the composed expectation; outputs: {name: pieces} with
    pieces(): the expected bytes of that output as uint8 arrays, one per repetition and one for the tail; lengths_at(R): the output
    lengths for any R (what R was found with)"""

    def __init__(self, name, inputs, R, want, outputs, lengths_at):
        self.name, self.inputs, self.R, self.want, self.outputs, self.lengths_at = name, inputs, R, want, outputs, lengths_at
        self.input_bytes = [R * b.size + t.size for b, t in inputs]
        assert max(self.input_bytes) <= MAX_INPUT, (name, self.input_bytes)

    def lengths(self):
        return {k: sum(p.size for p in pieces()) for k, pieces in self.outputs.items()}

    def input_pieces(self, j):
        block, tail = self.inputs[j]
        return [block] * self.R + [tail]


def tiled_pieces(t):
    block, tail = C.as_u8(t.block), C.as_u8(t.tail)
    return lambda: [block] * t.R + [tail]


def tiled_lengths(block, tail, names):
    return lambda R: [R * len(block[k]) + len(tail[k]) for k in names]


def ref_texts():
    return [c for p in FA for c in contigs_of(open(p, "rb").read()) if len(c) > 400]


def screen_cindex():
    return index_of_np([(n, open(p, "rb").read()) for n, p in zip(NAMES, FA)], 31)


# ---- fq-dedup -------------------------------------------------------------------------------------------------------------------

def dedup_reps(R):
    return (0, R // 3, 2 * R // 3, R - 1)


def dedup_case(probes):
    """the filler's headers carry the repetition number (C.numbered), so the filler comes out verbatim; the tail borrows headers of
    four repetitions.  Which repetitions it borrows from does not change a length, so R is found with a tail that borrows from 0"""
    def make(reps):
        rng = np.random.default_rng(SEEDS["single"])
        block, fields = C.single_block(rng, probes)
        return block, fields, C.single_tail(rng, probes, block, fields, reps)

    block, fields, tail0 = make((0,))
    kept0, _ = C.dedup_of(block, fields, 1, tail0)
    lengths_at = lambda R: [R * block.size + len(kept0)]
    R = smallest_R(lengths_at)
    block, fields, tail = make(dedup_reps(R))
    kept, want = C.dedup_of(block, fields, R, tail)
    assert len(kept) == len(kept0) and tail.size == tail0.size and want["bytes_out"] == lengths_at(R)[0]
    filler = C.numbered(block, fields, R).reshape(R, block.size)
    case = Case("dedup", [(block, tail)], R, want, dict(out=lambda: list(filler) + [C.as_u8(kept)]), lengths_at)
    case.input_pieces = lambda j: list(filler) + [tail]
    case.fields = fields
    return case


# ---- fq-merge, fq-trim, fq-screen: one paired input, each its own R -------------------------------------------------------------

def paired_data(refs):
    rng = np.random.default_rng(SEEDS["paired"])
    return C.paired_blocks(rng, refs), C.paired_tails(rng, refs)


def _paired_case(name, data, checker, composer, names):
    (b1, b2, _), (t1, t2, _) = data
    block, tail = checker(b1, b2), checker(t1, t2)
    lengths_at = tiled_lengths(block, tail, names)
    R = smallest_R(lengths_at)
    want = composer(block, tail, R)
    return Case(name, [(b1, t1), (b2, t2)], R, want, {k: tiled_pieces(want[k]) for k in names}, lengths_at)


def merge_case(data):
    return _paired_case("merge", data, C.merge_of, C.compose_merge, C.MERGE_OUTPUTS)


def trim_case(data):
    return _paired_case("trim", data, lambda a, b: C.trim_of(a, b, **C.TRIM_ALL), C.compose_trim, ("out1", "out2"))


def screen_case(data, cindex):
    return _paired_case("screen", data, lambda a, b: C.screen_of(cindex, a, b, **C.SCREEN_KW), C.compose_screen, ("out1", "out2"))


# ---- fq-demux -------------------------------------------------------------------------------------------------------------------

def demux_names():
    """the file of every destination and mate, in the order they are written (scfq_demux_host::out_path)"""
    return [(d, w, "%s_R%s.fq" % (C.DEMUX_SAMPLES[d][0] if d < len(C.DEMUX_SAMPLES) else "undetermined", w))
            for d in range(len(C.DEMUX_SAMPLES) + 1) for w in "12"]


def demux_case(refs):
    (b1, b2, _), (t1, t2, _) = C.barcoded_data(refs)
    block, tail = C.demux_of(b1, b2, **C.DEMUX_KW), C.demux_of(t1, t2, **C.DEMUX_KW)
    lengths_at = lambda R: [R * rb["bytes" + w] + rt["bytes" + w] for rb, rt in zip(block["rows"], tail["rows"]) for w in "12"]
    R = smallest_R(lengths_at)
    want = C.compose_demux(block, tail, R)
    return Case("demux", [(b1, t1), (b2, t2)], R, want, {f: tiled_pieces(want["out" + w][d]) for d, w, f in demux_names()}, lengths_at)


def unaligned_long_samples(rows):
    """the samples (not "undetermined") both of whose files start at an offset that is no multiple of 16 and are longer than a chunk"""
    return [d for d, r in enumerate(rows[:-1]) if all(r["off" + w] % 16 and r["bytes" + w] > CHUNK for w in "12")]


# ---- fq-normalize ---------------------------------------------------------------------------------------------------------------

def normalize_counted(refs):
    """(the input whose k-mers the given table counts, the paired data): C.normalize_counted of test_gpu_big_offsets_tables.py's pair"""
    data = C.tables_pair_data(refs)
    (b1, b2, _), (t1, t2, _) = data
    return C.normalize_counted(b1, b2, t1, t2), data


def _kept_pieces(kept, Ub, R, ln, block, tail):
    """the bytes of the kept units of one output: per repetition the block's bytes under that repetition's units, then the tail's"""
    def pieces():
        out = [block[np.repeat(kept[r * Ub:(r + 1) * Ub].astype(bool), ln.block)] for r in range(R)]
        return out + [tail[np.repeat(kept[R * Ub:].astype(bool), ln.tail)]]
    return pieces


def normalize_case(refs):
    """the sampled rule: the class of a unit depends on its number in the whole input.  A unit of the filler has the same number
    for every R, so the filler's kept bytes per repetition are found once (for the most repetitions MAX_INPUT allows); the tail's
    units are classified again for every R"""
    counted, ((b1, b2, _), (t1, t2, _)) = normalize_counted(refs)
    table = C.kcount_of(counted, None, K, CANONICAL)["table"]
    block = C.normalize_of(table, K, CANONICAL, b1, b2, **C.NORM_SAMPLED)
    tail = C.normalize_of(table, K, CANONICAL, t1, t2, **C.NORM_SAMPLED)
    Ub, Ut = len(block["classes"]), len(tail["classes"])
    top = (MAX_INPUT - max(t1.size, t2.size)) // max(b1.size, b2.size)
    most = C.compose_normalize_sampled(block, tail, top, **C.NORM_SAMPLED)
    kept = most["kept"][:top * Ub].reshape(top, Ub).astype(np.int64)
    filler = [np.concatenate([[0], np.cumsum(kept @ block["len%d" % j])]) for j in (1, 2)]      # kept bytes of the first R repetitions
    mates = [tail["recs"][m::2, j] for m in (0, 1) for j in (0, 1)]

    def lengths_at(R):
        cls, _ = C.classify_np(*mates, R * Ub + np.arange(Ut, dtype=np.uint64), **C.NORM_SAMPLED)
        return [int(filler[j][R]) + int(tail["len%d" % (j + 1)][cls == C.NORM_KEPT].sum()) for j in (0, 1)]

    R = smallest_R(lengths_at)
    assert R <= top
    want = C.compose_normalize_sampled(block, tail, R, **C.NORM_SAMPLED)
    assert [want["out1_bytes"], want["out2_bytes"]] == lengths_at(R)
    outputs = {"out%d" % j: _kept_pieces(want["kept"], Ub, R, want["len%d" % j], b, t) for j, b, t in ((1, b1, t1), (2, b2, t2))}
    case = Case("normalize", [(b1, t1), (b2, t2)], R, want, outputs, lengths_at)
    case.counted, case.table = counted, table
    return case


# ---- exact sizes: fq-trim with every step off -----------------------------------------------------------------------------------

def echo_block(probes):
    rng = np.random.default_rng(SEEDS["echo"])
    return C.single_block(rng, probes)[0]


def echo_input(block, size):
    """(block, R, tail) with R * block.size + tail.size == size: whole repetitions, then a tail of the block's first records and one
    last record "@x...x\\nACGT\\n+\\nIIII\\n" whose header is as long as it takes (shorter than one record of the block)"""
    last = b"@x\nACGT\n+\nIIII\n"
    starts = C.index_of(block)["off"][::4]                    # where a record of the block starts, and its end
    R, rest = divmod(size, block.size)
    if rest < len(last):
        R, rest = R - 1, rest + block.size
    assert R >= 0
    cut = int(starts[np.searchsorted(starts, rest - len(last), side="right") - 1])
    pad = rest - len(last) - cut
    assert 0 <= pad < 2000
    tail = np.concatenate([block[:cut], C.as_u8(b"@x" + b"x" * pad + last[2:])])
    assert R * block.size + tail.size == size
    return block, R, tail

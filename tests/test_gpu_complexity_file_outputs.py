"""scfq_cplx_files behind the writer every read-producing command shares (csrc/scfq_fdwrite.hpp), in the style of
tests/test_gpu_file_outputs.py: one input whose out1 passes two chunks of the writer, compared by a streaming hash with the checker's
output; a reader that goes away early (SCFQ_EPIPE); /dev/full (SCFQ_EIO).  The input is a block of 2 000 reads of 150 bases, every third
with a planted repeat, written R times: a record's output depends on the record alone, so the checker's result on the block, R times, is
the expectation."""
import hashlib
import os

import numpy as np
import pytest

from _complexity_check import FIELDS, SCORE_BINS, assert_stats, complexity_of
from _file_output_cases import CHUNK
from test_gpu_file_outputs import GONE_AFTER, eio_to_dev_full, epipe_call, sigpipe_ignored, through_a_pipe

pytestmark = pytest.mark.gpu

OPTS = dict(max_masked_pct=40, mask="lower")
ADDITIVE = ("reads1", "lines1", "input_bytes1", "reads_in", "reads_out", "low_reads", "dropped_reads", "masked_reads", "perfect_intervals", "bases_in",
            "bases_out", "masked_bases", "masked_bases_out", "out1_bytes")


def block_of():
    rng = np.random.default_rng(20261023)
    letters = np.frombuffer(b"ACGT", np.uint8)
    recs = []
    for i in range(2000):
        s = bytearray(letters[rng.integers(0, 4, 150)].tobytes())
        if i % 3 == 0:
            unit, run, at = letters[rng.integers(0, 4, 1 + i % 6)].tobytes(), int(rng.integers(8, 120)), int(rng.integers(0, 150))
            s[at:at + run] = (unit * 120)[:min(run, 150 - at)]
        recs.append(b"@block read %d\n%s\n+\n%s\n" % (i, bytes(s), bytes(33 + rng.integers(2, 41, 150).astype(np.uint8))))
    return b"".join(recs)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    block = block_of()
    w = complexity_of(block, **OPTS)
    assert 0 < w["dropped_reads"] < 400 and w["masked_bases_out"] > 0
    R = 2 * CHUNK // len(w["out1"]) + 2                   # out1 passes two chunks: a third one uses the first pinned buffer again
    want = dict(w, hist=[R * v for v in w["hist"]])
    want.update({k: R * w[k] for k in ADDITIVE})
    assert want["out1_bytes"] > 2 * CHUNK and R * len(block) < 80 * 10 ** 6
    path = str(tmp_path_factory.mktemp("cplx_files") / "in.fq")
    with open(path, "wb") as f:
        for _ in range(R):
            f.write(block)
    digest = hashlib.sha256()
    for _ in range(R):
        digest.update(w["out1"])
    yield dict(path=path, want=want, R=R, out1=w["out1"], digest=digest.hexdigest())
    os.remove(path)


def test_out1_past_two_chunks_a_reader_that_goes_away_and_a_full_device(gpu, scfq, case):
    want, opts = case["want"], scfq.cplx_opts(**OPTS)
    # through a pipe that is read to the end: the whole output, by its hash
    got = {}
    reader = through_a_pipe(lambda w: got.update(r=scfq.cplx_files(case["path"], None, opts, w)))
    s, h = got["r"]
    assert_stats(s, want, "to a pipe")
    assert h.tolist() == want["hist"] and sum(want["hist"]) == want["reads_in"] and len(want["hist"]) == SCORE_BINS
    assert reader.length == want["out1_bytes"] and reader.hash.hexdigest() == case["digest"]
    # a reader that goes away inside the second chunk
    sigpipe_ignored()
    err = {}
    reader = through_a_pipe(lambda w: err.update(e=epipe_call(scfq, lambda: scfq.cplx_files(case["path"], None, opts, w))), take=GONE_AFTER)
    kept = b"".join(reader.kept)
    whole = case["out1"] * (GONE_AFTER // len(case["out1"]) + 1)
    assert len(kept) == reader.length == GONE_AFTER and kept == whole[:GONE_AFTER], "what the reader got is no prefix of the output"
    assert scfq.lib().scfq_cplx_error_detail().decode().startswith("write:")
    assert_stats(err["e"].stats, want, "reader gone")                      # complete, as the header promises
    # a device that is full
    e = eio_to_dev_full(scfq, lambda fd: scfq.cplx_files(case["path"], None, opts, fd), scfq.lib().scfq_cplx_error_detail)
    assert_stats(e.stats, want, "/dev/full")
    # and the per-read table's descriptor fails the same way, before any read is written
    e = eio_to_dev_full(scfq, lambda fd: scfq.cplx_files(case["path"], None, opts, -1, -1, fd), scfq.lib().scfq_cplx_error_detail)
    assert_stats(e.stats, want, "/dev/full, per read")
    assert {k: want[k] for k in FIELDS} == {k: int(getattr(s, k)) for k in FIELDS}

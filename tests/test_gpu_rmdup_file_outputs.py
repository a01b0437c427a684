"""scfq_rmdup_files behind the writer every read-producing command shares (csrc/scfq_fdwrite.hpp), in the style of
tests/test_gpu_file_outputs.py: one single-end input whose out1 passes two chunks of the writer, compared by a streaming hash with the
checker's output; a reader that goes away early (SCFQ_EPIPE); /dev/full (SCFQ_EIO) on the output and on the per-unit table.  The input is
272 000 random reads of 150 bases, every fifth the sequence of an earlier read under its own name and with its own qualities.  A block
cannot be repeated here, since the repeats would all be duplicates: the checker runs over the whole input, once."""
import hashlib
import os

import numpy as np
import pytest

from _rmdup_check import FIELDS, HIST_BINS, assert_stats, rmdup_of
from _file_output_cases import CHUNK
from test_gpu_file_outputs import GONE_AFTER, eio_to_dev_full, epipe_call, sigpipe_ignored, through_a_pipe

pytestmark = pytest.mark.gpu

READS, LENGTH = 272_000, 150


def input_of():
    """records of one width: "@r%07d\\n", 150 bases, "\\n+\\n", 150 qualities, "\\n" """
    rng = np.random.default_rng(20261024)
    head = 10
    width = head + LENGTH + 3 + LENGTH + 1
    a = np.empty((READS, width), np.uint8)
    a[:, :head] = np.frombuffer(b"".join(b"@r%07d\n" % i for i in range(READS)), np.uint8).reshape(READS, head)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (READS, LENGTH))]
    copies = np.arange(9, READS, 5)                       # every fifth read: the sequence of an earlier read that is no copy itself
    source = (rng.random(copies.size) * copies).astype(np.int64)
    source -= source % 5 == 4
    seq[copies] = seq[source]
    a[:, head:head + LENGTH] = seq
    a[:, head + LENGTH:head + 3 + LENGTH] = np.frombuffer(b"\n+\n", np.uint8)
    a[:, head + 3 + LENGTH:head + 3 + 2 * LENGTH] = 33 + rng.integers(2, 41, (READS, LENGTH), dtype=np.uint8)
    a[:, -1] = 10
    return a.tobytes(), copies.size


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    data, planted = input_of()
    want = rmdup_of(data)
    assert want["duplicate_units"] == planted and want["units_in"] == READS and want["max_copies"] >= 2
    assert want["out1_bytes"] > 2 * CHUNK and len(data) < 100 * 10 ** 6      # out1 passes two chunks: a third one uses the first pinned buffer again
    path = str(tmp_path_factory.mktemp("rmdup_files") / "in.fq")
    with open(path, "wb") as f:
        f.write(data)
    yield dict(path=path, want=want, digest=hashlib.sha256(want["out1"]).hexdigest())
    os.remove(path)


def test_out1_past_two_chunks_a_reader_that_goes_away_and_a_full_device(gpu, scfq, case):
    want, opts = case["want"], scfq.rmdup_opts()
    # through a pipe that is read to the end: the whole output, by its length and its hash
    got = {}
    reader = through_a_pipe(lambda w: got.update(r=scfq.rmdup_files(case["path"], None, opts, w)))
    s, h = got["r"]
    assert_stats(s, want, "to a pipe")
    assert h.tolist() == want["hist"] and sum(want["hist"]) == want["units_out"] and len(want["hist"]) == HIST_BINS
    assert reader.length == want["out1_bytes"] and reader.hash.hexdigest() == case["digest"]
    assert int(s.collisions) == 0 and int(s.rounds) == 1
    # a reader that goes away inside the second chunk
    sigpipe_ignored()
    err = {}
    reader = through_a_pipe(lambda w: err.update(e=epipe_call(scfq, lambda: scfq.rmdup_files(case["path"], None, opts, w))), take=GONE_AFTER)
    kept = b"".join(reader.kept)
    assert len(kept) == reader.length == GONE_AFTER and kept == want["out1"][:GONE_AFTER], "what the reader got is no prefix of the output"
    assert scfq.lib().scfq_rmdup_error_detail().decode().startswith("write:")
    assert_stats(err["e"].stats, want, "reader gone")                      # complete, as the header promises
    # a device that is full
    e = eio_to_dev_full(scfq, lambda fd: scfq.rmdup_files(case["path"], None, opts, fd), scfq.lib().scfq_rmdup_error_detail)
    assert_stats(e.stats, want, "/dev/full")
    # and the per-unit table's descriptor fails the same way, before any read is written
    e = eio_to_dev_full(scfq, lambda fd: scfq.rmdup_files(case["path"], None, opts, -1, -1, fd), scfq.lib().scfq_rmdup_error_detail)
    assert_stats(e.stats, want, "/dev/full, per read")
    assert {k: want[k] for k in FIELDS} == {k: int(getattr(s, k)) for k in FIELDS}

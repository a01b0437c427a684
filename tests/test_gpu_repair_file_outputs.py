"""scfq_repair_files behind the writer every read-producing command shares (csrc/scfq_fdwrite.hpp), in the style of
tests/test_gpu_file_outputs.py: two inputs whose out2, the GATHERED output, passes two chunks of the writer, compared by a streaming hash
with the checker's output; a reader that goes away early (SCFQ_EPIPE); /dev/full (SCFQ_EIO) on an output and on the per-record table, and
the command that leaves no file behind then.  The inputs are 272 000 pairs of 150 bases; R2 holds its records in a random order, and
every 1000th record of R1 has a name that R2 does not have."""
import hashlib
import os
import subprocess
import threading

import numpy as np
import pytest

from conftest import GOLDEN, PKG
from _repair_check import FIELDS, assert_stats, repair_of
from _file_output_cases import CHUNK
from test_gpu_file_outputs import GONE_AFTER, eio_to_dev_full, epipe_call, sigpipe_ignored, through_a_pipe

pytestmark = pytest.mark.gpu

READS, LENGTH = 272_000, 150
SC = os.path.join(PKG, "sc")


def inputs_of():
    """records of one width: "@r%07d/m\\n", 150 bases, "\\n+\\n", 150 qualities, "\\n" """
    rng = np.random.default_rng(20261105)
    head = 12
    width = head + LENGTH + 3 + LENGTH + 1
    files = []
    for mate in (1, 2):
        a = np.empty((READS, width), np.uint8)
        names = [b"@r%07d/%d\n" % (i, mate) for i in range(READS)]
        if mate == 1:
            names[::1000] = [b"@x%07d/1\n" % i for i in range(0, READS, 1000)]
        a[:, :head] = np.frombuffer(b"".join(names), np.uint8).reshape(READS, head)
        a[:, head:head + LENGTH] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (READS, LENGTH))]
        a[:, head + LENGTH:head + 3 + LENGTH] = np.frombuffer(b"\n+\n", np.uint8)
        a[:, head + 3 + LENGTH:head + 3 + 2 * LENGTH] = 33 + rng.integers(2, 41, (READS, LENGTH), dtype=np.uint8)
        a[:, -1] = 10
        files.append(a if mate == 1 else a[rng.permutation(READS)])
    return files[0].tobytes(), files[1].tobytes()


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d1, d2 = inputs_of()
    want = repair_of(d1, d2)
    assert want["pairs"] == READS - READS // 1000 and want["singles1"] == want["singles2"] == READS // 1000 and want["moved"] > READS // 2
    assert want["out2_bytes"] > 2 * CHUNK and len(d2) < 100 * 10 ** 6      # out2 passes two chunks: a third one uses the first pinned buffer again
    where = tmp_path_factory.mktemp("repair_files")
    paths = [str(where / "in1.fq"), str(where / "in2.fq")]
    for p, d in zip(paths, (d1, d2)):
        with open(p, "wb") as f:
            f.write(d)
    yield dict(paths=paths, want=want, digest=hashlib.sha256(want["out2"]).hexdigest())
    for p in paths:
        os.remove(p)


def test_out2_past_two_chunks_a_reader_that_goes_away_and_a_full_device(gpu, scfq, case):
    want, (p1, p2) = case["want"], case["paths"]
    detail = scfq.lib().scfq_repair_error_detail
    # through a pipe that is read to the end: the whole gathered output, by its length and its hash
    got = {}
    reader = through_a_pipe(lambda w: got.update(s=scfq.repair_files(p1, p2, None, -1, w)))
    s = got["s"]
    assert_stats(s, want, "to a pipe", path=1)
    assert reader.length == want["out2_bytes"] and reader.hash.hexdigest() == case["digest"]
    # a reader that goes away inside the second chunk
    sigpipe_ignored()
    err = {}
    reader = through_a_pipe(lambda w: err.update(e=epipe_call(scfq, lambda: scfq.repair_files(p1, p2, None, -1, w))), take=GONE_AFTER)
    kept = b"".join(reader.kept)
    assert len(kept) == reader.length == GONE_AFTER and kept == want["out2"][:GONE_AFTER], "what the reader got is no prefix of the output"
    assert detail().decode().startswith("write:")
    assert_stats(err["e"].stats, want, "reader gone")                      # complete, as the header promises
    # a device that is full, under the gathered output and under a sequential one
    e = eio_to_dev_full(scfq, lambda fd: scfq.repair_files(p1, p2, None, -1, fd), detail)
    assert_stats(e.stats, want, "/dev/full, out2")
    e = eio_to_dev_full(scfq, lambda fd: scfq.repair_files(p1, p2, None, -1, -1, fd), detail)
    assert_stats(e.stats, want, "/dev/full, singles1")
    # and the per-record table's descriptor fails the same way, before any read is written
    e = eio_to_dev_full(scfq, lambda fd: scfq.repair_files(p1, p2, None, -1, -1, -1, -1, fd), detail)
    assert_stats(e.stats, want, "/dev/full, per read")
    assert {k: want[k] for k in FIELDS} == {k: int(getattr(s, k)) for k in FIELDS}


def test_the_command_goes_quiet_or_leaves_no_file_behind(gpu, tmp_path):
    r1, r2 = (os.path.join(GOLDEN, "repair", f) for f in ("r1.fq", "r2.fq"))
    # /dev/full under out1: status 1, and the files this call created are gone again
    r = subprocess.run([SC, "fq-repair", "--out1=/dev/full", "--out2=o2.fq", "--singles1=s1.fq", "--per-read=t.tsv", r1, r2], capture_output=True,
                       stdin=subprocess.DEVNULL, cwd=str(tmp_path))
    assert r.returncode == 1 and b"Error" in r.stderr and r.stdout == b"" and os.listdir(str(tmp_path)) == [], (r, os.listdir(str(tmp_path)))
    # a reader that is gone: quiet, status 0.  The reader opens the FIFO, which lets the command's open return, and closes it at once
    fifo = str(tmp_path / "gone.fifo")
    os.mkfifo(fifo)
    th = threading.Thread(target=lambda: os.close(os.open(fifo, os.O_RDONLY)), daemon=True)
    th.start()
    r = subprocess.run([SC, "fq-repair", "--out1=gone.fifo", "--out2=o2.fq", r1, r2], capture_output=True, stdin=subprocess.DEVNULL, cwd=str(tmp_path), timeout=120)
    th.join(30)
    assert (r.returncode, r.stderr, r.stdout) == (0, b"", b"") and not th.is_alive(), r

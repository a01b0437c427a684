"""The last metre of the six commands that write reads — fq-dedup, fq-merge, fq-trim, fq-screen, fq-demux, fq-normalize — from device
memory to a file descriptor (csrc/scfq_fdwrite.hpp: Pinned::device_to_fd), on outputs of more than one and more than two of its
chunks: regular files compared with == to the composed checkers' results (tests/_file_output_cases.py, pinned without a GPU in
tests/test_file_output_cases_host.py), outputs of exactly kChunk - 1 .. 2 kChunk + 1 bytes, a pipe that is drained slowly and one
whose reader goes away, /dev/full, a directory that takes no file, and `sc` on top of each.  Every failing call runs once; after it
the pool memory and the descriptors of the process are what they were and the next call is byte-exact.

A wrong buffer parity shows as a second or third chunk that differs (the message names the chunk), a last chunk cut wrong as a file
length, bytes dropped after a short write() as a hash of the pipe's bytes."""
import hashlib
import os
import signal
import stat
import subprocess
import threading

import numpy as np
import pytest

import _big_offset_cases as C
import _file_output_cases as F
from conftest import PKG
from _demux_check import assert_stats as assert_demux
from _kcount_check import CANONICAL
from _merge_check import assert_stats as assert_merge
from _normalize_check import assert_stats as assert_norm
from _screen_check import assert_stats as assert_screen
from _trim_check import assert_stats as assert_trim, trim_of_np

pytestmark = pytest.mark.gpu

SC = os.path.join(PKG, "sc")
CHUNK = F.CHUNK
READ = 4093                      # bytes a draining reader asks for: no divisor of a pipe's buffer or of a chunk
GONE_AFTER = CHUNK + 5           # bytes a reader takes before it goes away: inside the second chunk


# ---- files ----------------------------------------------------------------------------------------------------------------------

def write_pieces(path, pieces):
    with open(path, "wb") as f:
        for p in pieces:
            f.write(p)
    return str(path)


def assert_bytes(got, pieces, ctx):
    """got: a uint8 array; pieces: the expected arrays, one per repetition and one for the tail.  Compared piece by piece"""
    at = 0
    for i, p in enumerate(pieces):
        have = got[at:at + p.size]
        if have.size != p.size or not np.array_equal(have, p):
            n = min(have.size, p.size)
            j = at + (int(np.flatnonzero(have[:n] != p[:n])[0]) if (have[:n] != p[:n]).any() else n)
            raise AssertionError((ctx, "piece %d of %d differs at byte %d of %d (%d owed): chunk %d of the writer, byte %d of it" %
                                  (i, len(pieces), j, got.size, sum(q.size for q in pieces), j // CHUNK, j % CHUNK),
                                  bytes(got[j:j + 40]), bytes(p[j - at:j - at + 40])))
        at += p.size
    assert got.size == at, (ctx, "the output has %d bytes, %d are owed" % (got.size, at))


def assert_file(path, pieces, ctx):
    assert_bytes(np.fromfile(str(path), np.uint8), pieces, ctx)


class Outputs:
    """regular files in a directory, opened for writing; closed and removed at the end of the `with`"""

    def __init__(self, where, names):
        self.paths = [os.path.join(str(where), n) for n in names]

    def __enter__(self):
        self.fds = [os.open(p, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644) for p in self.paths]
        return self

    def close(self):
        for fd in self.fds:
            os.close(fd)
        self.fds = []

    def __exit__(self, *exc):
        self.close()
        for p in self.paths:
            os.remove(p)


class Staged:
    """a case of tests/_file_output_cases.py with its inputs as files"""

    def __init__(self, case, where):
        self.case, self.want, self.R = case, case.want, case.R
        self.paths = [write_pieces(os.path.join(str(where), "%s_in%d.fq" % (case.name, j + 1)), case.input_pieces(j)) for j in range(len(case.inputs))]
        assert [os.path.getsize(p) for p in self.paths] == case.input_bytes

    def remove(self):
        for p in self.paths:
            os.remove(p)


@pytest.fixture(scope="module")
def where(tmp_path_factory):
    return tmp_path_factory.mktemp("file_outputs")


def staged(make):
    @pytest.fixture(scope="module")
    def fixture(request, where):
        s = Staged(make(request), where)
        yield s
        s.remove()
    return fixture


@pytest.fixture(scope="module")
def probes(scfq):
    return [seq.encode() for _, seq in scfq.adapters_default()]


@pytest.fixture(scope="module")
def refs():
    return F.ref_texts()


@pytest.fixture(scope="module")
def paired(refs):
    return F.paired_data(refs)


dedup_in = staged(lambda r: F.dedup_case(r.getfixturevalue("probes")))
merge_in = staged(lambda r: F.merge_case(r.getfixturevalue("paired")))
trim_in = staged(lambda r: F.trim_case(r.getfixturevalue("paired")))
screen_in = staged(lambda r: F.screen_case(r.getfixturevalue("paired"), F.screen_cindex()))
demux_in = staged(lambda r: F.demux_case(r.getfixturevalue("refs")))
norm_in = staged(lambda r: F.normalize_case(r.getfixturevalue("refs")))


@pytest.fixture(scope="module")
def norm_table(gpu, scfq, norm_in):
    """the library's table of the counted input (host memory only)"""
    distinct = len(norm_in.case.table)
    bits = max(10, (4 * distinct - 1).bit_length())
    s, table = scfq.kcount_host(norm_in.case.counted, k=F.K, flags=CANONICAL, table_bits=bits)
    assert int(s.distinct) == distinct
    with table:
        yield table


class Echo:
    """the input that fq-trim with every step off echoes, of exactly `size` bytes, as a file"""

    def __init__(self, block, size, where, name="echo"):
        blk, R, tail = F.echo_input(block, size)
        self.size, self.pieces = size, [blk] * R + [tail]
        self.path = write_pieces(os.path.join(str(where), "%s_%d.fq" % (name, size)), self.pieces)
        self.want = C.compose_trim(trim_of_np(blk, None, **F.TRIM_OFF), trim_of_np(tail, None, **F.TRIM_OFF), R)
        assert os.path.getsize(self.path) == size == self.want["out1_bytes"]

    def whole(self):
        return np.concatenate(self.pieces)


@pytest.fixture(scope="module")
def echo_block(probes):
    return F.echo_block(probes)


@pytest.fixture(scope="module")
def echo(echo_block, where):
    """the echo input of 2 kChunk + 1 bytes: three chunks, the last one byte long"""
    e = Echo(echo_block, F.PIPE_SIZE, where)
    yield e
    os.remove(e.path)


def stats_of(st, want):
    return {k: int(getattr(st, k)) for k in want}


# ---- what the process holds -------------------------------------------------------------------------------------------------------

def trim_off(scfq):
    return scfq.trim_opts(**F.TRIM_OFF)


def echo_call(scfq, echo, where, ctx):
    """fq-trim of the echo input into a regular file: byte-exact, with complete statistics"""
    with Outputs(where, ["echo_out.fq"]) as o:
        s = scfq.trim_file(echo.path, None, trim_off(scfq), o.fds[0])
        o.close()
        assert_trim(s, echo.want, ctx)
        assert_file(o.paths[0], echo.pieces, ctx)
    return s


@pytest.fixture(scope="module")
def warmed(gpu, scfq, echo, where):
    """one file call behind which what the process holds stays what it is: a process's first call opens device nodes, and its first
    file call makes the staging memory that the library keeps.  (What it wrote is not looked at: the tests do that.)"""
    with Outputs(where, ["warm_up.fq"]) as o:
        scfq.trim_file(echo.path, None, trim_off(scfq), o.fds[0])


@pytest.fixture(autouse=True)
def pool_memory(scfq, gpu, warmed):
    before = scfq.lib().scfq_device_bytes_now()
    yield
    assert scfq.lib().scfq_device_bytes_now() == before


def held(scfq):
    return int(scfq.lib().scfq_device_bytes_now()), len(os.listdir("/proc/self/fd"))


class Unchanged:
    """around one failing call: pool memory and descriptors afterwards as before, and the next call to a regular file byte-exact"""

    def __init__(self, scfq, echo, where, ctx):
        self.scfq, self.echo, self.where, self.ctx = scfq, echo, where, ctx

    def __enter__(self):
        self.before = held(self.scfq)
        return self

    def __exit__(self, kind, value, tb):
        if kind is None:
            assert held(self.scfq) == self.before, (self.ctx, "pool bytes and descriptors", held(self.scfq), self.before)
            echo_call(self.scfq, self.echo, self.where, (self.ctx, "the next call"))


def sigpipe_ignored():
    if signal.getsignal(signal.SIGPIPE) != signal.SIG_IGN:
        pytest.skip("SIGPIPE is not ignored in this interpreter: a write to a closed pipe would kill pytest")


class Reader(threading.Thread):
    """reads the read end of a pipe in pieces of READ bytes into a hash and a length; take: the bytes after which it closes the
    pipe and ends (None: at the end of the data).  What it read is kept when it goes away early"""

    def __init__(self, fd, take=None, keep=False):
        super().__init__()
        self.fd, self.take, self.keep = fd, take, keep
        self.length, self.hash, self.kept, self.error = 0, hashlib.sha256(), [], None

    def run(self):
        try:
            while self.take is None or self.length < self.take:
                b = os.read(self.fd, READ if self.take is None else min(READ, self.take - self.length))
                if not b:
                    break
                self.length += len(b)
                self.hash.update(b)
                if self.keep:
                    self.kept.append(b)
        except BaseException as e:         # (reported by the test, which joins)
            self.error = e
        finally:
            os.close(self.fd)


def through_a_pipe(call, take=None):
    """call(write_fd) with a Reader on the other end; the write end is closed here whatever the call does.  Returns the reader"""
    r, w = os.pipe()
    reader = Reader(r, take, keep=take is not None)
    reader.start()
    try:
        call(w)
    finally:
        os.close(w)
        reader.join()
    assert reader.error is None, reader.error
    return reader


def assert_prefix(reader, pieces, ctx):
    got = np.frombuffer(b"".join(reader.kept), np.uint8)
    assert got.size == reader.length == GONE_AFTER, (ctx, got.size)
    whole = np.concatenate(pieces)
    assert whole.size > got.size and np.array_equal(got, whole[:got.size]), (ctx, "what the reader got is no prefix of the output")


# ---- 2. every command into regular files ------------------------------------------------------------------------------------------

def test_dedup_to_a_file(gpu, scfq, dedup_in, where):
    case = dedup_in.case
    with Outputs(where, ["dedup.fq"]) as o:
        st = scfq.dedup_file(dedup_in.paths[0], o.fds[0])
        o.close()
        assert stats_of(st, case.want) == case.want
        assert os.path.getsize(o.paths[0]) == int(st.bytes_out)
        assert_file(o.paths[0], case.outputs["out"](), "dedup")


def test_merge_to_files(gpu, scfq, merge_in, where):
    case = merge_in.case
    with Outputs(where, ["%s.fq" % k for k in C.MERGE_OUTPUTS]) as o:
        s = scfq.merge_file(*merge_in.paths, merged_fd=o.fds[0], un1_fd=o.fds[1], un2_fd=o.fds[2])
        o.close()
        assert_merge(s, case.want, "merge")
        for k, p in zip(C.MERGE_OUTPUTS, o.paths):
            assert os.path.getsize(p) == int(getattr(s, k + "_bytes")), k
            assert_file(p, case.outputs[k](), ("merge", k))
    assert s.merged > case.R and s.too_long > 20


def two_outputs(where, call, check, case, ctx):
    with Outputs(where, [ctx + "_out1.fq", ctx + "_out2.fq"]) as o:
        s = call(*o.fds)
        o.close()
        check(s, case.want, ctx)
        for k, p in zip(("out1", "out2"), o.paths):
            assert os.path.getsize(p) == int(getattr(s, k + "_bytes")), (ctx, k)
            assert_file(p, case.outputs[k](), (ctx, k))
    return s


def test_trim_to_files(gpu, scfq, trim_in, where):
    opts = scfq.trim_opts(**C.TRIM_ALL)
    s = two_outputs(where, lambda fd1, fd2: scfq.trim_file(*trim_in.paths, opts, fd1, fd2), assert_trim, trim_in.case, "trim")
    assert min(s.cut_overlap, s.cut_adapter, s.cut_polyg, s.cut_quality, s.dropped_reads) > trim_in.R


def test_screen_to_files(gpu, scfq, screen_in, where):
    opts = scfq.screen_opts(**C.SCREEN_KW)
    with scfq.screen_index_files(F.FA) as index:
        s = two_outputs(where, lambda fd1, fd2: scfq.screen_file(index, *screen_in.paths, opts, fd1, fd2), assert_screen, screen_in.case, "screen")
    assert s.matched_pairs > screen_in.R and 0 < s.reads_out < s.reads_in


def test_demux_to_a_directory(gpu, scfq, demux_in, where):
    case = demux_in.case
    out_dir = os.path.join(str(where), "demux_out")
    os.mkdir(out_dir)
    try:
        with scfq.demux_sheet(list(C.DEMUX_SAMPLES)) as sheet:
            s, rows = scfq.demux_file(sheet, *demux_in.paths, scfq.demux_opts(**C.DEMUX_KW), out_dir=out_dir)
        assert_demux(s, rows, case.want, "demux")
        # from the rows the library gave: two samples or more whose files start at offsets that are no multiple of 16 inside the
        # device buffer and are longer than a chunk
        unaligned = [d for d, r in enumerate(rows[:-1]) if all(int(getattr(r, "off" + w)) % 16 and int(getattr(r, "bytes" + w)) > CHUNK for w in "12")]
        assert len(unaligned) >= 2, [(int(r.off1), int(r.off2), int(r.bytes1), int(r.bytes2)) for r in rows]
        names = F.demux_names()
        assert sorted(os.listdir(out_dir)) == sorted(f for _, _, f in names)
        for d, w, f in names:
            p = os.path.join(out_dir, f)
            assert os.path.getsize(p) == int(getattr(rows[d], "bytes" + w)), f
            assert_file(p, case.outputs[f](), ("demux", f, "starts at byte %d of out%s" % (int(getattr(rows[d], "off" + w)), w)))
    finally:
        for f in os.listdir(out_dir):
            os.remove(os.path.join(out_dir, f))
        os.rmdir(out_dir)


def norm_opts(scfq):
    return scfq.norm_opts(**C.NORM_SAMPLED)


def test_normalize_to_files(gpu, scfq, norm_in, norm_table, where):
    opts = norm_opts(scfq)
    s = two_outputs(where, lambda fd1, fd2: scfq.norm_file(norm_table, *norm_in.paths, opts, fd1, fd2)[0], assert_norm, norm_in.case, "normalize")
    assert 0 < s.units_out < s.units_in and min(s.dropped_low, s.dropped_high) > norm_in.R


# ---- 3. exact sizes ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", F.EXACT_SIZES, ids=["chunk-1", "chunk", "chunk+1", "2chunk", "2chunk+1"])
def test_output_of_exactly(gpu, scfq, echo_block, where, size):
    """an output that ends one byte before, on and one byte behind the end of the first and of the second chunk"""
    e = Echo(echo_block, size, where, "exactly")
    try:
        s = echo_call(scfq, e, where, ("exactly", size))
        assert int(s.out1_bytes) == size and int(s.reads_out) == int(s.reads_in)
    finally:
        os.remove(e.path)


# ---- 4. pipes ---------------------------------------------------------------------------------------------------------------------

def test_trim_into_a_pipe_that_is_drained_slowly(gpu, scfq, echo):
    """write() to a pipe takes what fits: write_all's loop over short writes, three chunks long"""
    sigpipe_ignored()
    got = {}
    reader = through_a_pipe(lambda w: got.update(s=scfq.trim_file(echo.path, None, trim_off(scfq), w)))
    assert_trim(got["s"], echo.want, "pipe, drained")
    assert reader.length == echo.size
    assert reader.hash.hexdigest() == hashlib.sha256(echo.whole()).hexdigest()


def epipe_call(scfq, call):
    with pytest.raises(scfq.ScfqError) as e:
        call()
    assert e.value.rc == scfq.SCFQ_EPIPE, str(e.value)
    return e.value


def test_trim_into_a_pipe_whose_reader_goes_away(gpu, scfq, echo, warmed, where):
    sigpipe_ignored()
    ok = echo_call(scfq, echo, where, "before")
    with Unchanged(scfq, echo, where, "trim, reader gone"):
        err = {}
        reader = through_a_pipe(lambda w: err.update(e=epipe_call(scfq, lambda: scfq.trim_file(echo.path, None, trim_off(scfq), w))), take=GONE_AFTER)
        assert_prefix(reader, echo.pieces, "trim")
        assert scfq.lib().scfq_trim_error_detail().decode().startswith("write:")
        s = err["e"].stats                                      # complete, as the header promises
        assert_trim(s, echo.want, "trim, reader gone")
        assert (int(s.reads_out), int(s.out1_bytes)) == (int(ok.reads_out), int(ok.out1_bytes))


def test_dedup_into_a_pipe_whose_reader_goes_away(gpu, scfq, dedup_in, echo, warmed, where):
    sigpipe_ignored()
    with Unchanged(scfq, echo, where, "dedup, reader gone"):
        reader = through_a_pipe(lambda w: epipe_call(scfq, lambda: scfq.dedup_file(dedup_in.paths[0], w)), take=GONE_AFTER)
        assert_prefix(reader, dedup_in.case.outputs["out"](), "dedup")
        assert scfq.lib().scfq_dedup_error_detail().decode().startswith("write:")


def test_merge_with_unmerged1_into_a_pipe_whose_reader_goes_away(gpu, scfq, merge_in, echo, warmed, where):
    """`merged` is written first: it is complete and exact when the second output's reader goes away"""
    sigpipe_ignored()
    case = merge_in.case
    with Unchanged(scfq, echo, where, "merge, reader gone"):
        with Outputs(where, ["merged.fq", "unmerged2.fq"]) as o:
            err = {}
            reader = through_a_pipe(lambda w: err.update(e=epipe_call(scfq, lambda: scfq.merge_file(*merge_in.paths, merged_fd=o.fds[0], un1_fd=w, un2_fd=o.fds[1]))),
                                    take=GONE_AFTER)
            o.close()
            assert_prefix(reader, case.outputs["unmerged1"](), "merge, unmerged1")
            assert_file(o.paths[0], case.outputs["merged"](), "merge, merged, written before the failure")
            assert os.path.getsize(o.paths[1]) == 0, "unmerged2 comes after the output that failed"
            assert scfq.lib().scfq_merge_error_detail().decode().startswith("write:")
            assert_merge(err["e"].stats, case.want, "merge, reader gone")


def test_normalize_with_out2_into_a_pipe_whose_reader_goes_away(gpu, scfq, norm_in, norm_table, echo, warmed, where):
    sigpipe_ignored()
    case = norm_in.case
    with Unchanged(scfq, echo, where, "normalize, reader gone"):
        with Outputs(where, ["norm_out1.fq"]) as o:
            err = {}
            reader = through_a_pipe(lambda w: err.update(e=epipe_call(scfq, lambda: scfq.norm_file(norm_table, *norm_in.paths, norm_opts(scfq), o.fds[0], w))),
                                    take=GONE_AFTER)
            o.close()
            assert_prefix(reader, case.outputs["out2"](), "normalize, out2")
            assert_file(o.paths[0], case.outputs["out1"](), "normalize, out1, written before the failure")
            assert scfq.lib().scfq_norm_error_detail().decode().startswith("write:")
            assert_norm(err["e"].stats, case.want, "normalize, reader gone")


# ---- 5. a device that is full, a directory that takes no file -------------------------------------------------------------------

def eio_to_dev_full(scfq, call, detail):
    fd = os.open("/dev/full", os.O_WRONLY)
    try:
        with pytest.raises(scfq.ScfqError) as e:
            call(fd)
    finally:
        os.close(fd)
    assert e.value.rc == scfq.SCFQ_EIO, str(e.value)
    assert detail().decode().startswith("write:"), detail()
    return e.value


def test_trim_to_a_full_device(gpu, scfq, echo, warmed, where):
    """the write of chunk 0 fails while the copy of chunk 1 is on its way into the other pinned buffer"""
    with Unchanged(scfq, echo, where, "trim, /dev/full"):
        e = eio_to_dev_full(scfq, lambda fd: scfq.trim_file(echo.path, None, trim_off(scfq), fd), scfq.lib().scfq_trim_error_detail)
        assert_trim(e.stats, echo.want, "trim, /dev/full")


def test_screen_to_a_full_device(gpu, scfq, screen_in, echo, warmed, where):
    opts = scfq.screen_opts(**C.SCREEN_KW)
    with scfq.screen_index_files(F.FA) as index:
        with Unchanged(scfq, echo, where, "screen, /dev/full"):
            e = eio_to_dev_full(scfq, lambda fd: scfq.screen_file(index, *screen_in.paths, opts, fd, -1), scfq.lib().scfq_screen_error_detail)
            assert_screen(e.stats, screen_in.want, "screen, /dev/full")


def test_demux_into_a_directory_that_takes_no_file(gpu, scfq, refs, echo, warmed, where):
    """(the tails of the demux case alone: the first open() fails, whatever the outputs' sizes)"""
    if os.geteuid() == 0:
        pytest.skip("root creates files in a directory without write permission")
    (_, _, _), (t1, t2, _) = C.barcoded_data(refs)
    want = C.demux_of(t1, t2, **C.DEMUX_KW)
    paths = [write_pieces(os.path.join(str(where), "demux_tail%d.fq" % j), [t]) for j, t in ((1, t1), (2, t2))]
    closed = os.path.join(str(where), "closed")
    os.mkdir(closed)
    os.chmod(closed, 0o555)
    try:
        with scfq.demux_sheet(list(C.DEMUX_SAMPLES)) as sheet:
            with Unchanged(scfq, echo, where, "demux, read-only directory"):
                with pytest.raises(scfq.ScfqError) as e:
                    scfq.demux_file(sheet, *paths, scfq.demux_opts(**C.DEMUX_KW), out_dir=closed)
                assert e.value.rc == scfq.SCFQ_EIO, str(e.value)
                assert os.path.join(closed, F.demux_names()[0][2]) in scfq.lib().scfq_demux_error_detail().decode()
                assert_demux(e.value.stats, e.value.rows, want, "demux, read-only directory")
        assert os.listdir(closed) == []
    finally:
        os.chmod(closed, 0o755)
        os.rmdir(closed)
        for p in paths:
            os.remove(p)


# ---- 6. sc ------------------------------------------------------------------------------------------------------------------------

def test_sc_trim_is_quiet_when_its_reader_goes_away(gpu, echo):
    p = subprocess.Popen([SC, "fq-trim", echo.path], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    try:
        got = b""
        while len(got) < GONE_AFTER:
            b = p.stdout.read(GONE_AFTER - len(got))
            assert b, "sc wrote %d bytes only" % len(got)
            got += b
        p.stdout.close()
        err = p.stderr.read()
        assert p.wait(timeout=120) == 0 and err == b"", (p.returncode, err)
    finally:
        if p.poll() is None:
            p.kill()
            p.wait()
        p.stderr.close()
    assert got[:1] == b"@" and got.count(b"\n") > 1000


def sc_merge_to_dev_full(merge_in, un1, un2):
    with open("/dev/full", "wb") as full:
        return subprocess.run([SC, "fq-merge", "--unmerged1=" + un1, "--unmerged2=" + un2] + merge_in.paths, stdin=subprocess.DEVNULL, stdout=full,
                              stderr=subprocess.PIPE, timeout=300)


def test_sc_merge_discards_its_files_when_stdout_is_full(gpu, merge_in, where):
    un1, un2 = (os.path.join(str(where), n) for n in ("sc_un1.fq", "sc_un2.fq"))
    r = sc_merge_to_dev_full(merge_in, un1, un2)
    assert r.returncode == 1 and len(r.stderr.decode().splitlines()) == 1 and b"write:" in r.stderr, (r.returncode, r.stderr)
    assert not os.path.exists(un1) and not os.path.exists(un2)


def test_sc_merge_leaves_a_fifo_when_stdout_is_full(gpu, merge_in, where):
    un1, un2 = (os.path.join(str(where), n) for n in ("sc_un1.fifo", "sc_un2.fq"))
    os.mkfifo(un1)
    drained = []

    def drain():
        with open(un1, "rb") as f:                              # (returns once sc has opened the other end)
            while True:
                b = f.read(1 << 16)
                if not b:
                    break
                drained.append(len(b))

    t = threading.Thread(target=drain)
    t.start()
    try:
        r = sc_merge_to_dev_full(merge_in, un1, un2)
    finally:
        if t.is_alive() and not drained:                        # sc never opened it: open it here, so that the thread's open returns
            fd = os.open(un1, os.O_WRONLY | os.O_NONBLOCK) if os.path.exists(un1) else -1
            if fd >= 0:
                os.close(fd)
        t.join()
    try:
        assert r.returncode == 1 and len(r.stderr.decode().splitlines()) == 1, (r.returncode, r.stderr)
        assert stat.S_ISFIFO(os.stat(un1).st_mode), "the FIFO the caller made is the caller's"
        assert not os.path.exists(un2) and sum(drained) == 0
    finally:
        if os.path.exists(un1):
            os.remove(un1)


def test_sc_dedup_to_stdout(gpu, dedup_in, where):
    out = os.path.join(str(where), "sc_dedup.fq")
    try:
        with open(out, "wb") as f:
            r = subprocess.run([SC, "fq-dedup", dedup_in.paths[0]], stdin=subprocess.DEVNULL, stdout=f, stderr=subprocess.PIPE, timeout=300)
        want = dedup_in.want
        assert r.returncode == 0 and r.stderr.decode().splitlines()[:2] == ["total_reads: %d" % want["total_reads"], "duplicates %d" % want["duplicates"]], r.stderr
        assert_file(out, dedup_in.case.outputs["out"](), "sc fq-dedup > out")
    finally:
        os.remove(out)

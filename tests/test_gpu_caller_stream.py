"""The caller-stream contract of include/sc_fqcount.h (scfq_opts.wait_stream, scfq_set_wait_stream), asserted for every `*_device`
wrapper of tests/_caller_cases.py: device-pointer arguments, inputs and outputs, are ordered after the work already queued on the
caller's stream, and the results are visible to any stream when the call returns.

The input side.  The input buffers hold a DECOY, another valid input of the same byte length.  On the caller's stream, with no host
synchronisation, a delay is queued, then the copies of the real input over the decoy (the second input last), then the sentinel
fill of every output buffer, then the event `ready`.  The entry condition: `ready` is still pending immediately before the call (a
delay that was too short is doubled and the sequence repeated, a few times; then the test FAILS, it never passes without the
condition).  On return `ready` has happened, every part of the result is the real input's, the outputs hold the wanted bytes with
the sentinel intact behind their reported sizes, read back on a third stream without a device-wide synchronisation.  A call that
did not wait returns the decoy's result (tests/test_caller_cases_host.py: it differs in every part) or has its output overwritten by
the sentinel."""
import ctypes

import numpy as np
import pytest

import _caller_cases as T

pytestmark = pytest.mark.gpu

ATTEMPTS = 4
STREAMS = ("fresh", "legacy")                         # a fresh non-blocking stream of the caller; the legacy default stream
PLACES = ((0, 0), (T.SHORT_LINES, 17), (T.CRLF, 0), (T.SINGLE, 4095))      # (seed, bytes past a 4 KiB boundary)
WITH_OUTPUTS = [j for j in T.JOBS if j.outs and j.name != "index_lines_device"]      # (scfq_index_lines takes device input only)


class Delay:
    """element-wise passes over 256 MiB on the current stream: about 0.15 ms each"""

    def __init__(self, torch):
        self.x = torch.zeros(64 << 20, dtype=torch.float32, device="cuda")
        self.passes = 32

    def queue(self):
        for _ in range(self.passes):
            self.x.add_(1.0)


@pytest.fixture(scope="module")
def delay(gpu):
    d = Delay(gpu)
    first = d.passes
    yield d
    print("\ncaller-stream tests: %d passes of the delay kernel at the end (%d at the start)" % (d.passes, first))


@pytest.fixture
def restore_wait_stream(scfq, gpu):
    """whatever a test does to the thread's wait stream, it ends as the `gpu` fixture had set it"""
    on = ctypes.c_int(0)
    before = scfq.lib().scfq_get_wait_stream(ctypes.byref(on))
    assert on.value == 1, "the gpu fixture sets the wait stream"
    try:
        yield
    finally:
        scfq.set_wait_stream(before or 0)


def ordered_call(torch, scfq, delay, job, seed, which, offset, host_input=False, via_opts=False, control=False):
    """the sequence of the module docstring for one job; returns (got, want, the decoy's wanted result).  control: the wait stream is
    cleared — what a library that does not wait would do; the caller gets the result back instead of an assertion"""
    real, decoy = job.make(seed), job.decoy(seed)
    want, other = T.wanted(job, seed), T.wanted(job, seed, decoy=True)
    ctx = job.context(scfq, real)
    try:
        stream = torch.cuda.Stream() if which == "fresh" else torch.cuda.default_stream()
        assert (stream.cuda_stream == 0) == (which == "legacy")
        reals = [] if host_input else [torch.from_numpy(r.copy()).cuda() for r in real]
        for attempt in range(ATTEMPTS):
            placed = [] if host_input else [T.place(torch, d, offset) for d in decoy]
            rooms = T.rooms_of(torch, job, want, fill=T.BLANK)
            torch.cuda.synchronize()
            ready = torch.cuda.Event()
            if control:
                scfq.set_wait_stream(None)
            elif via_opts:
                scfq.set_wait_stream(None)                 # the thread default is cleared: only scfq_opts.wait_stream names the stream
            else:
                scfq.set_wait_stream(stream.cuda_stream)
            kw = dict(wait_stream=stream.cuda_stream) if via_opts else {}
            with torch.cuda.stream(stream):
                delay.queue()
                for (_, _, view), r in zip(placed, reals):
                    view.copy_(r)
                for room in rooms.values():
                    room.t.fill_(T.SENTINEL)
                ready.record()
            if not ready.query():                          # the entry condition, immediately before the call
                break
            torch.cuda.synchronize()
            delay.passes *= 2
        else:
            pytest.fail("ordering was not exercised: the queued work had finished before the call, with %d passes of the delay" % delay.passes)
        label = (job.name, "seed %d" % seed, which, "offset %d" % offset, "host input" if host_input else "device input")
        try:
            got, used = job.run(torch, scfq, [(p, d.size) for (_, p, _), d in zip(placed, decoy)], {n: r.arg() for n, r in rooms.items()}, want, ctx,
                                host=real if host_input else None, **kw)
        except scfq.ScfqError as e:
            if control:
                return dict(error=repr(e)), want, other
            raise AssertionError((label, "the call failed: outputs sized for the real input do not hold another input's result", repr(e)))
        returned_after = ready.query()
        if control:
            torch.cuda.synchronize()
            return got, want, other
        assert returned_after, (label, "the call returned while the caller's stream was still busy: it did not wait")
        T.compare(job, got, want, label, other)
        assert set(used) == set(rooms), (label, used)
        third = torch.cuda.Stream()                        # visible to any stream: no device-wide synchronisation before this
        with torch.cuda.stream(third):
            back = {name: room.t.cpu().numpy() for name, room in rooms.items()}
        for name, room in rooms.items():
            room.check(back[name], used[name], want[name], (label, name))
        for (t, p, view), r in zip(placed, real):         # and the input is what the caller wrote, between intact guards
            host = t.cpu().numpy()
            start = p - t.data_ptr()
            assert np.array_equal(host[start:start + r.size], r) and bool((host[:start] == 0x47).all()) and bool((host[start + r.size:] == 0x47).all()), label
        return got, want, other
    finally:
        torch.cuda.synchronize()
        if ctx is not None:
            ctx.close()


@pytest.mark.parametrize("which", STREAMS)
@pytest.mark.parametrize("job", T.JOBS, ids=repr)
def test_device_input_waits_for_the_callers_stream(gpu, scfq, delay, restore_wait_stream, job, which):
    for seed, offset in PLACES:
        ordered_call(gpu, scfq, delay, job, seed, which, offset)


@pytest.mark.parametrize("which", STREAMS)
@pytest.mark.parametrize("job", WITH_OUTPUTS, ids=repr)
def test_device_outputs_of_host_input_wait_for_the_callers_stream(gpu, scfq, delay, restore_wait_stream, job, which):
    """the `direct` / `recs_device` term of a pipeline's after_caller flag: nothing but the outputs is the caller's device memory"""
    for seed in (0, T.SHORT_LINES):
        ordered_call(gpu, scfq, delay, job, seed, which, 0, host_input=True)


@pytest.mark.parametrize("which", STREAMS)
@pytest.mark.parametrize("name", ["count_device", "partial_device", "partial_device+hist"])
def test_wait_stream_in_the_options(gpu, scfq, delay, restore_wait_stream, name, which):
    """SCFQ_WAIT_STREAM and scfq_opts.wait_stream, with the thread's default cleared"""
    for seed, offset in PLACES[:2]:
        ordered_call(gpu, scfq, delay, T.BY_NAME[name], seed, which, offset, via_opts=True)


def test_the_wait_stream_is_the_fixtures_again(gpu, scfq):
    on = ctypes.c_int(0)
    stream = scfq.lib().scfq_get_wait_stream(ctypes.byref(on))
    assert on.value == 1 and (stream or 0) == gpu.cuda.default_stream().cuda_stream

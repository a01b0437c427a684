"""fq-repair between a caller and its kernels: the caller-stream rule (the sequence of tests/test_gpu_caller_stream.py, imported, with its
entry condition: the test fails, and never passes, when the caller's stream was already idle, so the input is still the decoy when the
call is made) and twelve host threads on the twelve worker seeds (tests/test_gpu_threads.py's run_threads).  The job is one more row for
the table of tests/_caller_cases.py, kept in tests/_repair_cases.py; what its inputs hold is asserted without a device in
tests/test_repair_host.py."""
import pytest

import _caller_cases as T
from _repair_cases import JOB
from test_gpu_caller_stream import PLACES, STREAMS, delay, ordered_call, restore_wait_stream      # noqa: F401  (the two fixtures)
from test_gpu_threads import ROUNDS, run_threads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def placed(gpu):
    """the job's inputs of every worker seed in device memory, at a pointer offset of its own"""
    held = {}
    for seed in T.WORKER_SEEDS:
        off = (0, 1, 17, 64, 4095, 33)[seed % 6]
        r1, r2 = JOB.make(seed)
        held[seed] = (T.place(gpu, r1, off), T.place(gpu, r2, (off + 7) % 4096), (r1.size, r2.size))
    return held


def test_the_inputs_tell_a_call_that_did_not_wait():
    """the real input and its decoy differ in every part that is compared"""
    for seed, _ in PLACES:
        want, other = T.wanted(JOB, seed), T.wanted(JOB, seed, decoy=True)
        assert all(want[p] != other[p] for p in JOB.parts), (seed, [p for p in JOB.parts if want[p] == other[p]])


@pytest.mark.parametrize("which", STREAMS)
def test_device_input_waits_for_the_callers_stream(gpu, scfq, delay, restore_wait_stream, which):      # noqa: F811
    for seed, offset in PLACES:
        ordered_call(gpu, scfq, delay, JOB, seed, which, offset)


@pytest.mark.parametrize("which", STREAMS)
def test_device_outputs_of_host_input_wait_for_the_callers_stream(gpu, scfq, delay, restore_wait_stream, which):      # noqa: F811
    """nothing but the outputs and the per-record table is the caller's device memory"""
    for seed in (0, T.SHORT_LINES):
        ordered_call(gpu, scfq, delay, JOB, seed, which, 0, host_input=True)


def test_twelve_threads(gpu, scfq, placed):
    """twelve threads, the same command, twelve different inputs"""
    torch = gpu
    for seed in T.WORKER_SEEDS:
        T.wanted(JOB, seed)
    assert len({T.wanted(JOB, seed)["out2"] for seed in T.WORKER_SEEDS}) == len(T.WORKER_SEEDS)

    def work(i, r):
        seed = T.WORKER_SEEDS[i]
        p1, p2, sizes = placed[seed]
        T.call(torch, scfq, JOB, [(p1[1], sizes[0]), (p2[1], sizes[1])], T.wanted(JOB, seed), None, (JOB.name, "thread %d" % i, "round %d" % r))

    before = scfq.lib().scfq_device_bytes_now()
    run_threads(torch, scfq, work, rounds=ROUNDS)
    assert scfq.lib().scfq_device_bytes_now() == before

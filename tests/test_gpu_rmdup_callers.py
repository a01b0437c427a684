"""fq-rmdup between a caller and its kernels: the caller-stream rule (the sequence of tests/test_gpu_caller_stream.py, imported, with its
entry condition: the test fails, and never passes, when the caller's stream was already idle) and twelve host threads on the twelve worker
seeds (tests/test_gpu_threads.py's run_threads).  The job is one more row for the table of tests/_caller_cases.py, kept here; what its
inputs hold is asserted without a device in tests/test_rmdup_host.py."""
import numpy as np
import pytest

import _caller_cases as T
from _rmdup_check import FIELDS, rmdup_of
from test_gpu_caller_stream import PLACES, STREAMS, delay, ordered_call, restore_wait_stream      # noqa: F401  (the two fixtures)
from test_gpu_threads import ROUNDS, inputs, run_threads                                           # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

RMDUP_REC = np.dtype([("rep", "<u4"), ("copies", "<u4")])


class Rmdup(T.TwoOutputs):
    rec = (8, "units_in")
    more = ("hist",)
    opts = dict(prefix=10, swapped=True)           # (the first ten bases: the inputs' reads share starts, and mates change places)

    def wanted(self, inputs, base=None):
        a1, a2 = self.texts(inputs)
        w = rmdup_of(a1.tobytes(), None if a2 is None else a2.tobytes(), interleaved=self.interleaved, **self.opts)
        return dict(stats=T.pick(w, FIELDS), hist=w["hist"], recs=T.packed(w["recs"], RMDUP_REC, 2), out1=w["out1"], out2=w["out2"])

    def run(self, torch, scfq, ptrs, outs, want, ctx=None, host=None):
        opts, two, recs = scfq.rmdup_opts(interleaved=self.interleaved, **self.opts), (T._out(outs, "out1"), T._out(outs, "out2")), T._out(outs, "recs")
        if host is None:
            s, hist = scfq.rmdup_resident(*T._args(ptrs), opts, *two, recs=recs)
        else:
            s, hist = scfq._rmdup_call(scfq.lib().scfq_rmdup_buffers, "scfq_rmdup_buffers", T._host_head(scfq, host) + [scfq._opts_ref(opts)],
                                       lambda h: self.table_args(recs) + [h] + scfq._trim_outputs(two) + [1])
        return dict(stats=T.fields_of(s, FIELDS), hist=hist.tolist()), self.used(s, outs)


JOBS = (Rmdup("rmdup_resident"), Rmdup("rmdup_resident interleaved", kind="interleaved"))


def test_the_inputs_tell_a_call_that_did_not_wait():
    """the real input and its decoy differ in every part that is compared, and units are removed"""
    for job in JOBS:
        for seed, _ in PLACES:
            want, other = T.wanted(job, seed), T.wanted(job, seed, decoy=True)
            assert all(want[p] != other[p] for p in job.parts), (job, seed)
        w = T.wanted(job, 0)["stats"]
        assert 0 < w["duplicate_units"] < w["units_in"] // 2 and w["duplicated_classes"] > 0, w


@pytest.mark.parametrize("which", STREAMS)
@pytest.mark.parametrize("job", JOBS, ids=repr)
def test_device_input_waits_for_the_callers_stream(gpu, scfq, delay, restore_wait_stream, job, which):      # noqa: F811
    for seed, offset in PLACES:
        ordered_call(gpu, scfq, delay, job, seed, which, offset)


@pytest.mark.parametrize("which", STREAMS)
@pytest.mark.parametrize("job", JOBS, ids=repr)
def test_device_outputs_of_host_input_wait_for_the_callers_stream(gpu, scfq, delay, restore_wait_stream, job, which):      # noqa: F811
    """nothing but the outputs and the per-unit table is the caller's device memory"""
    for seed in (0, T.SHORT_LINES):
        ordered_call(gpu, scfq, delay, job, seed, which, 0, host_input=True)


@pytest.mark.parametrize("job", JOBS, ids=repr)
def test_twelve_threads(gpu, scfq, inputs, job):      # noqa: F811
    """twelve threads, the same command, twelve different inputs"""
    torch = gpu
    for seed in T.WORKER_SEEDS:
        T.wanted(job, seed)
    assert len({T.wanted(job, seed)["out1"] for seed in T.WORKER_SEEDS}) == len(T.WORKER_SEEDS)

    def work(i, r):
        seed = T.WORKER_SEEDS[i]
        T.call(torch, scfq, job, inputs[seed].ptrs(job), T.wanted(job, seed), None, (job.name, "thread %d" % i, "round %d" % r))

    before = scfq.lib().scfq_device_bytes_now()
    run_threads(torch, scfq, work, rounds=ROUNDS)
    assert scfq.lib().scfq_device_bytes_now() == before

"""fq-repair's row for the table of tests/_caller_cases.py, kept outside it: the job that tests/test_gpu_repair_callers.py runs behind a
busy caller stream and from twelve threads, and whose inputs tests/test_repair_host.py looks at without a device.

The pairs of tests/_caller_cases.py are in step, which would leave both singles outputs empty and the table the identity.  make() takes
them out of step without changing a file's length (a decoy has the byte lengths of the real input, file by file): every seventh record
of R1 from the second on gets the second byte of its header in upper case — another name, so the record and its mate are singles — and
R2's records are rotated by 1 + seed % 5."""
import numpy as np

import _caller_cases as T
from _repair_check import FIELDS, OUTPUTS, repair_of


def records_of(data):
    lines = bytes(data).split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    return [b"\n".join(lines[k:k + 4]) + b"\n" for k in range(0, len(lines) - 1, 4)]


def out_of_step(r1, r2, seed):
    a, b = records_of(r1), records_of(r2)
    for i in range(1, len(a), 7):
        if a[i][1:2].isalpha():
            a[i] = a[i][:1] + a[i][1:2].upper() + a[i][2:]
    k = (1 + seed % 5) % max(len(b), 1)
    b = b[k:] + b[:k]
    out = np.frombuffer(b"".join(a), np.uint8), np.frombuffer(b"".join(b), np.uint8)
    assert out[0].size == len(r1) and out[1].size == len(r2)
    return out


class Repair(T.Paired):
    primary = "out1"
    parts = ("stats", "table") + OUTPUTS
    outs = (("table", 4),) + tuple((n, 1) for n in OUTPUTS)

    def make(self, seed, decoy=False):
        f = T.fastq(seed, decoy)
        return list(out_of_step(f[0].tobytes(), f[1].tobytes(), seed))

    def wanted(self, inputs, base=None):
        w = repair_of(inputs[0].tobytes(), inputs[1].tobytes())
        return dict(stats=T.pick(w, FIELDS), table=np.asarray(w["table"], "<u4").tobytes(), **dict(zip(OUTPUTS, w["outs"])))

    def run(self, torch, scfq, ptrs, outs, want, ctx=None, host=None):
        four, table = [T._out(outs, n) for n in OUTPUTS], T._out(outs, "table")
        if host is None:
            s = scfq.repair_resident(*T._args(ptrs), None, four, table=table)
        else:
            s = scfq._repair_call(scfq.lib().scfq_repair_buffers, "scfq_repair_buffers",
                                  T._host_head(scfq, host) + [None] + T.TwoOutputs.table_args(table) + scfq._repair_outputs(four) + [1])
        used = dict(table=int(s.reads1 + s.reads2), **{n: int(getattr(s, n + "_bytes")) for n in OUTPUTS})
        return dict(stats=T.fields_of(s, FIELDS)), ({n: used[n] for n in outs} if outs else {})


JOB = Repair("repair_resident")

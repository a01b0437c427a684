"""What the seven commands that write reads share (scfq_reads_device.hpp, scfq_reads_host.hpp), through all seven doors: the units of
the inputs, a record echoed as it stands, the groups' lengths and their scans, where the outputs go, the too-small output and the two
ways out (host memory, the caller's device memory).

Every command runs with settings that change no read, on five records of 20 to 70 bases per file: a group of 32 is partly filled, and
wave_copy's head, body and tail all occur.  The inputs come with LF, with CRLF, with CRLF and no final newline, and with a last record
cut behind its second line; as one file, as two files of five and four records, and interleaved with nine.  The outputs are host and
device memory of exactly the result's size between 0xA5 bytes, and then one byte short, one output at a time: SCFQ_EARG, complete
statistics, and not a byte written anywhere.  The wanted bytes are each command's own plain model's (tests/_*_check.py): the commands
need not agree on a record that is cut."""
import numpy as np
import pytest

import _complexity_check as CX
import _demux_check as DX
import _merge_check as MG
import _normalize_check as NM
import _rmdup_check as RU
import _screen_check as SC
import _trim_check as TR
from _kcount_check import kcount_of

pytestmark = pytest.mark.gpu

FILL, GUARD = 0xA5, 19                     # (19: the outputs begin off every alignment wave_copy looks at)
FORMS = ("lf", "crlf", "crlf no final newline", "cut behind line 2")
MODES = ("single", "two", "interleaved")
LENGTHS = ((20, 33, 47, 64, 70), (21, 38, 52, 69))
SAMPLES = [("s1", "ACGTAC"), ("s2", "TTGGCA")]
K_SCREEN, K_NORM = 15, 15


def _dna(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def _records(which):
    """the records of file `which`: distinct random reads; three of the headers end in a sample's barcode, one with a wrong letter"""
    rng = np.random.default_rng([20261201, which])
    tails = (b"ACGTAC", b"", b"TTGGCA", b"ACGTAA", b"")
    return [[b"@r%d.%d 1:N:0:%s" % (which, i, tails[i]), _dna(rng, n), b"+", bytes(33 + (7 * i + j) % 40 for j in range(n))]
            for i, n in enumerate(LENGTHS[which])]


def _text(records, form):
    eol = b"\n" if form in ("lf", "cut behind line 2") else b"\r\n"
    if form == "cut behind line 2":
        records = records[:-1] + [records[-1][:2]]
    text = b"".join(line + eol for rec in records for line in rec)
    return text[:-len(eol)] if form == "crlf no final newline" else text


def inputs_of(mode, form):
    a, b = _records(0), _records(1)
    if mode == "single":
        return [_text(a, form)]
    if mode == "two":
        return [_text(a, form), _text(b, form)]
    return [_text([a[0], b[0], a[1], b[1], a[2], b[2], a[3], b[3], a[4]], form)]


REFERENCE = b">other\n" + _dna(np.random.default_rng(20261202), 300) + b"\n"


class Command:
    names = ("out1", "out2")

    def outputs(self, mode):
        return self.names if mode == "two" else self.names[:1]

    def sizes(self, s):
        return (int(s.out1_bytes), int(s.out2_bytes))

    def check_stats(self, got, want, ctx):
        self.model.assert_stats(got, want, ctx)


class Trim(Command):
    model, kw = TR, dict(no_overlap=True, no_adapters=True, min_length=0)

    def want(self, data, mode):
        w = TR.trim_of(*data, interleaved=mode == "interleaved", **self.kw)
        assert w["dropped_reads"] == 0 and w["bases_out"] == w["bases_in"]
        return w

    def call(self, scfq, head, outs, on_dev, mode, ctx):
        return scfq._trim_call(scfq.lib().scfq_trim_buffers, "scfq_trim_buffers", scfq.trim_opts(interleaved=mode == "interleaved", **self.kw), head, outs + [on_dev])


class Merge(Command):
    model, names = MG, ("merged", "unmerged1", "unmerged2")

    def outputs(self, mode):
        return self.names if mode == "two" else self.names[:2]

    def sizes(self, s):
        return (int(s.merged_bytes), int(s.unmerged1_bytes), int(s.unmerged2_bytes))

    def want(self, data, mode):
        w = MG.merge_of(*data)
        assert MG.stat(w, "merged") == 0 and w["merged"] == b"" and w["unmerged1"]
        return {**w, **{n: bytes(w[n]) for n in self.names}}

    def call(self, scfq, head, outs, on_dev, mode, ctx):
        return scfq._merge_call(scfq.lib().scfq_merge_buffers, "scfq_merge_buffers", None, 33, mode == "interleaved", head, outs + [on_dev])


class Screen(Command):
    model = SC

    def want(self, data, mode):
        w = SC.screen_of(SC.index_of([("other", REFERENCE)], K_SCREEN), *data, interleaved=mode == "interleaved")
        assert w["matched_reads"] == 0 and w["dropped_reads"] == 0
        return w

    def call(self, scfq, head, outs, on_dev, mode, ctx):
        return scfq._screen_call(scfq.lib().scfq_screen_buffers, "scfq_screen_buffers", ctx, scfq.screen_opts(interleaved=mode == "interleaved"), head,
                                 [None, 0] + outs + [on_dev])

    def context(self, scfq):
        return scfq.screen_index_host([("other", REFERENCE)], K_SCREEN)


class Demux(Command):
    model, kw = DX, dict(header=True, keep_barcode=True)

    def want(self, data, mode):
        w = DX.demux_of(data[0], data[1] if len(data) > 1 else None, SAMPLES, interleaved=mode == "interleaved", **self.kw)
        assert w["bases_clipped"] == 0 and 0 < w["assigned"] < w["units_in"]
        return w

    def call(self, scfq, head, outs, on_dev, mode, ctx):
        s, rows = scfq._demux_call(scfq.lib().scfq_demux_buffers, "scfq_demux_buffers", ctx, scfq.demux_opts(interleaved=mode == "interleaved", **self.kw), head,
                                   [None, 0], outs + [on_dev])
        s.rows = rows
        return s

    def context(self, scfq):
        return scfq.demux_sheet(SAMPLES)

    def check_stats(self, got, want, ctx):
        DX.assert_stats(got, got.rows, want, ctx)


class Normalize(Command):
    model, kw = NM, dict(target=1000)

    def want(self, data, mode):
        w = NM.normalize_of(kcount_of(list(data), K_NORM, True).table, K_NORM, True, *data, interleaved=mode == "interleaved", **self.kw)
        assert w["units_out"] == w["units_in"] > 0
        return w

    def call(self, scfq, head, outs, on_dev, mode, ctx):
        opts = scfq.norm_opts(interleaved=mode == "interleaved", k=K_NORM, canonical=True, **self.kw)
        return scfq._norm_call(scfq.lib().scfq_norm_buffers, "scfq_norm_buffers", None, opts, head, [None, 0] + outs + [on_dev], 0)[0]


class Complexity(Command):
    model = CX

    def want(self, data, mode):
        w = CX.complexity_of(*data, interleaved=mode == "interleaved", mask=CX.MASK_NONE, max_masked_pct=100)
        assert w["dropped_reads"] == 0
        return w

    def call(self, scfq, head, outs, on_dev, mode, ctx):
        opts = scfq.cplx_opts(interleaved=mode == "interleaved", mask="none", max_masked_pct=100)
        return scfq._cplx_call(scfq.lib().scfq_cplx_buffers, "scfq_cplx_buffers", opts, head, lambda h: [None, 0, h] + outs + [on_dev], False)[0]


class Rmdup(Command):
    model = RU

    def want(self, data, mode):
        w = RU.rmdup_of(*data, interleaved=mode == "interleaved")
        assert w["duplicate_units"] == 0 and w["units_in"] > 0
        return w

    def call(self, scfq, head, outs, on_dev, mode, ctx):
        return scfq._rmdup_call(scfq.lib().scfq_rmdup_buffers, "scfq_rmdup_buffers", head + [scfq._opts_ref(scfq.rmdup_opts(interleaved=mode == "interleaved"))],
                                lambda h: [None, 0, h] + outs + [on_dev], False)[0]


COMMANDS = dict(trim=Trim(), merge=Merge(), screen=Screen(), demux=Demux(), normalize=Normalize(), complexity=Complexity(), rmdup=Rmdup())
CASES = [(c, m) for c in COMMANDS for m in MODES if not (c == "merge" and m == "single")]


class Room:
    """`cap` bytes of host or device memory between GUARD bytes, all of them FILL"""

    def __init__(self, torch, cap, on_dev):
        self.cap = cap
        if on_dev:
            self.t = torch.full((cap + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
            self.ptr = self.t.data_ptr() + GUARD
        else:
            self.t = np.full(cap + 2 * GUARD, FILL, np.uint8)
            self.ptr = self.t.ctypes.data + GUARD

    def bytes(self):
        return (self.t if isinstance(self.t, np.ndarray) else self.t.cpu().numpy()).tobytes()

    def holds(self, want):
        """`want` and nothing else"""
        return self.bytes() == bytes([FILL]) * GUARD + want + bytes([FILL]) * (self.cap - len(want) + GUARD)


def _head(scfq, torch, data, on_dev):
    """(ptr1, n1, ptr2, n2, is_device) and what keeps the memory alive"""
    import ctypes
    keep, head = [], []
    for d in data:
        a = np.frombuffer(d, np.uint8)
        t = torch.from_numpy(a.copy()).cuda() if on_dev else a
        keep.append(t)
        head += [ctypes.c_void_p(t.data_ptr() if on_dev else a.ctypes.data), a.size]
    return head + ([None, 0] if len(data) == 1 else []) + [1 if on_dev else 0], keep


@pytest.fixture(scope="module")
def contexts(gpu, scfq):
    made = {name: cmd.context(scfq) for name, cmd in COMMANDS.items() if hasattr(cmd, "context")}
    yield made
    for c in made.values():
        c.close()


@pytest.mark.parametrize("name,mode", CASES, ids=["%s %s" % c for c in CASES])
def test_outputs_that_fit_and_outputs_one_byte_short(gpu, scfq, contexts, name, mode):
    torch, cmd, ctx = gpu, COMMANDS[name], contexts.get(name)
    names = cmd.outputs(mode)
    for form in FORMS:
        data = inputs_of(mode, form)
        want = cmd.want(data, mode)
        sizes = [len(want[n]) for n in names]
        assert sum(sizes) > 200, (name, mode, form, sizes)
        for on_dev in (0, 1):
            label = (name, mode, form, "device" if on_dev else "host")
            head, keep = _head(scfq, torch, data, on_dev)
            # every output of exactly its size
            rooms = [Room(torch, n, on_dev) for n in sizes]
            outs = scfq._merge_outputs([(r.ptr, r.cap) for r in rooms] + [None] * (len(cmd.names) - len(names)))
            s = cmd.call(scfq, head, outs, on_dev, mode, ctx)
            cmd.check_stats(s, want, label)
            assert list(cmd.sizes(s)[:len(names)]) == sizes, label
            for n, r in zip(names, rooms):
                assert r.holds(want[n]), label + (n, r.bytes()[GUARD:GUARD + 80], want[n][:80])
            # one output a byte short: nothing is written to any, the statistics are complete
            for k, n in enumerate(names):
                if sizes[k] == 0:
                    continue
                rooms = [Room(torch, size - (j == k), on_dev) for j, size in enumerate(sizes)]
                outs = scfq._merge_outputs([(r.ptr, r.cap) for r in rooms] + [None] * (len(cmd.names) - len(names)))
                with pytest.raises(scfq.ScfqError) as e:
                    cmd.call(scfq, head, outs, on_dev, mode, ctx)
                text = "the %s output holds %d bytes, the result has %d" % (n, sizes[k] - 1, sizes[k])
                assert e.value.rc == scfq.SCFQ_EARG and text in str(e.value), label + (str(e.value),)
                if name == "demux":
                    e.value.stats.rows = e.value.rows
                cmd.check_stats(e.value.stats, want, label + ("short", n))
                assert all(r.holds(b"") for r in rooms), label + ("short", n)
            del keep

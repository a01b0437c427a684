"""fq-dedup on the device at the edges of its kernels (the inputs of tests/_dedup_cases.py; tests/test_dedup_cases_host.py pins
them on the CPU): everything is == against oracle.dedup — the bytes, total_reads, duplicates, records_out, bytes_out.

Two ways in.  (1) Families a-f through scfq.dedup_host in a fresh child process per setting of SCFQ_DEDUP_HASH_BITS and
SCFQ_DEDUP_FUSED_HASH (read once per process): with 4 bits of hash the exact compare decides nearly every pair.  (2) In this
process, scfq.dedup_device on caller's memory: the input at base + 0 .. 15, the output at an aligned address + 0 .. 15 inside a
buffer of sentinel bytes, sized, gathered directly (capacity above the input's size) and gathered after the size is known
(capacity == bytes_out); one byte less is SCFQ_EARG, and no byte around the output changes in any of them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _dedup_cases as dc
from test_gpu_parity import to_dev

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

SETTINGS = {
    "default": {},
    "bits4": {"SCFQ_DEDUP_HASH_BITS": "4"},
    "bits40": {"SCFQ_DEDUP_HASH_BITS": "40"},
    "unfused": {"SCFQ_DEDUP_FUSED_HASH": "0"},
    "bits4_unfused": {"SCFQ_DEDUP_HASH_BITS": "4", "SCFQ_DEDUP_FUSED_HASH": "0"},
}
# seconds a child may take: a new process, the library loaded, every case of the family once.  Measured on an MI355X, the slowest of the
# five settings beside each; the limit is there to end a child that hangs, so it is wide
CHILD_TIMEOUT = {
    "tail_compare": 30,      # measured 1.6 s
    "length_only": 30,       # measured 0.6 s
    "input_ends": 30,        # measured 1.2 s
    "mixed_eol": 30,         # measured 0.7 s
    "groups": 30,            # measured 1.2 s
    "copy_lengths": 30,      # measured 1.0 s
    "saturated": 120,        # measured 7.4 s (4.8 s of it in the library: two calls, 117 MB from host memory each)
}
_failed_child = []           # the first child that failed: no further one is started behind it


def run_child(family, setting):
    if _failed_child:
        pytest.fail("not started: the child %s failed before" % (_failed_child[0],))
    env = {k: v for k, v in os.environ.items() if k not in ("SCFQ_DEDUP_HASH_BITS", "SCFQ_DEDUP_FUSED_HASH")}
    env.update(SETTINGS[setting])
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "_dedup_cases.py"), "--run", family], env=env, capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT[family], cwd=os.path.dirname(HERE))
    except subprocess.TimeoutExpired as e:
        _failed_child.append((family, setting))
        pytest.fail("%s / %s: no answer within %d s; %r" % (family, setting, CHILD_TIMEOUT[family], (e.stdout or b"")[-2000:]))
    if r.returncode != 0:
        _failed_child.append((family, setting))
        pytest.fail("%s / %s: exit status %d\n%s\n%s" % (family, setting, r.returncode, r.stdout[-3000:], r.stderr[-3000:]))
    print(r.stdout.strip())
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("family", dc.FAMILIES[:-1])
def test_family_in_a_child_per_setting(gpu, family, setting):
    res = run_child(family, setting)
    assert res["family"] == family and res["cases"] == sum(1 for _ in dc.cases(family))
    if setting.startswith("bits4") and not setting.startswith("bits40") and family in ("tail_compare", "length_only"):
        # more headers than 4 bits have values: equal hashes of different headers in EVERY case, told apart by the compare alone
        assert res["min_hash_collisions"] > 0, res


def test_saturated(gpu):
    """Headers of 0xFFFFFF bytes and more (header_span looks them up again through the line index), each twice, and a sibling that
    differs at byte 64: two threads walk 16 MiB byte by byte.  On its own, under its own limit, default settings.
    Measured on an MI355X: 4.8 s in the library for the sizing call and the call that returns the bytes, 5.7 s for the test."""
    res = run_child("saturated", "default")
    assert res["cases"] == 1


# ------------------------------------------------------------------------------------------------------------ caller's device memory
SENTINEL = 0xA5
_cache = {}


def family_cases(oracle, family, subset):
    """(name, input as numpy, the oracle's bytes, the oracle's statistics) — computed once, shared by every offset"""
    key = (family, subset)
    if key not in _cache:
        if family not in _cache:
            _cache[family] = []
            for name, data, exp in dc.cases(family):
                a = np.frombuffer(data, dtype=np.uint8)
                want, ost = oracle.dedup(a)
                _cache[family].append((name, a, want, (ost.total_reads, ost.duplicates, ost.records_out, ost.bytes_out)))
        every = _cache[family]
        if subset == "all":
            picked = every
        elif subset == "ends":
            picked = [every[0], every[-1]]
        elif subset == "ends_and_small":          # input_ends: every n <= 40, and the first and last case of the family
            picked = [c for i, c in enumerate(every) if c[0].startswith("input_ends/n=") or i in (0, len(every) - 1)]
        else:                                     # copy_lengths: each body length at residue 0 (the output's offset gives the residues)
            assert subset == "residue0"
            picked = [c for c in every if c[0].endswith(",residue=0") or "100000" in c[0]]
        _cache[key] = picked
    return _cache[key]


def stats_of(st):
    return (st.total_reads, st.duplicates, st.records_out, st.bytes_out)


class OutBuffer:
    """cap bytes at `offset` past a 256-byte aligned address, sentinel bytes before, inside and behind"""

    def __init__(self, torch, cap, offset, guard=512):
        self.t = torch.empty(guard + 256 + offset + cap + guard, dtype=torch.uint8, device="cuda")
        base = self.t.data_ptr()
        self.start = (base + guard + 255) // 256 * 256 - base + offset
        self.ptr = base + self.start
        assert self.ptr % 256 == offset and self.start + cap + guard <= self.t.numel()

    def reset(self):
        self.t.fill_(SENTINEL)

    def check(self, n_written, want, ctx):
        host = self.t.cpu().numpy()
        assert (host[:self.start] == SENTINEL).all(), ("bytes before out", ctx)
        assert (host[self.start + n_written:] == SENTINEL).all(), ("bytes behind the result", ctx)
        assert host[self.start:self.start + n_written].tobytes() == want, ("bytes", ctx)


def three_calls(torch, scfq, case, in_off, out_off):
    name, a, want, ostats = case
    ctx = (name, in_off, out_off)
    n = a.size
    keep, ptr = to_dev(torch, a, in_off)
    assert ptr % 16 == in_off
    nb, st = scfq.dedup_device(ptr, n)                                      # sizing
    assert nb == len(want) and stats_of(st) == ostats, ("sizing", ctx, nb, stats_of(st), ostats)
    stats = stats_of(st) + (st.hash_collisions,)
    out = OutBuffer(torch, n + 64, out_off)
    out.reset()
    nb, st = scfq.dedup_device(ptr, n, out.ptr, n + 64)                     # direct gather: enqueued before the size is known
    assert nb == len(want) and stats_of(st) + (st.hash_collisions,) == stats, ("direct", ctx)
    out.check(nb, want, ("direct", ctx))
    if len(want) < n:
        out.reset()
        nb, st = scfq.dedup_device(ptr, n, out.ptr, len(want))              # exact capacity: gathered once the size is back
        assert nb == len(want) and stats_of(st) + (st.hash_collisions,) == stats, ("exact", ctx)
        out.check(nb, want, ("exact", ctx))
    if len(want) >= 1:
        out.reset()
        with pytest.raises(scfq.ScfqError) as e:
            scfq.dedup_device(ptr, n, out.ptr, len(want) - 1)               # (== n for an input without a final newline that drops nothing)
        assert e.value.rc == scfq.SCFQ_EARG, ctx
        host = out.t.cpu().numpy()                                          # nothing before out, nothing behind its len(want) - 1 bytes
        assert (host[:out.start] == SENTINEL).all() and (host[out.start + len(want) - 1:] == SENTINEL).all(), ("one byte short", ctx)
    del keep


DIAGONAL = [("tail_compare", "ends"), ("length_only", "ends"), ("mixed_eol", "ends"), ("input_ends", "ends_and_small"), ("groups", "all"),
            ("copy_lengths", "all")]


@pytest.mark.parametrize("offset", range(16))
@pytest.mark.parametrize("family,subset", DIAGONAL, ids=[f for f, s in DIAGONAL])
def test_device_pointers_on_the_diagonal(gpu, scfq, oracle, family, subset, offset):
    """input at base + offset, output at an aligned address + offset"""
    for case in family_cases(oracle, family, subset):
        three_calls(gpu, scfq, case, offset, offset)


@pytest.mark.parametrize("in_off", range(16))
def test_copy_lengths_every_pair_of_offsets(gpu, scfq, oracle, in_off):
    """wave_copy reads at any alignment and stores 16 bytes at a time from the first aligned byte of its destination: every
    pair (input offset, output offset) for every body length"""
    for out_off in range(16):
        for case in family_cases(oracle, "copy_lengths", "residue0"):
            three_calls(gpu, scfq, case, in_off, out_off)

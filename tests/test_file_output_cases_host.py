"""tests/_file_output_cases.py without a GPU: the R every case picked puts the command's outputs on the stated sides of kChunk and
2 * kChunk and R - 1 does not (from checker lengths alone), the five exact-size inputs have exactly their sizes and are echoed by the
checker, the demux case has its unaligned multi-chunk files — and a model of the two-buffer schedule of
csrc/scfq_fdwrite.hpp: device_to_fd, which states the invariant the GPU tests of tests/test_gpu_file_outputs.py rely on."""
import numpy as np
import pytest

import _big_offset_cases as C
import _file_output_cases as F
from _trim_check import trim_of_np


@pytest.fixture(scope="module")
def probes(scfq):
    return [seq.encode() for _, seq in scfq.adapters_default()]


@pytest.fixture(scope="module")
def refs():
    return F.ref_texts()


@pytest.fixture(scope="module")
def paired(refs):
    return F.paired_data(refs)


def check_case(case, byte_fields):
    """byte_fields: {output: the field of the composed statistics that holds its length}"""
    lengths = case.lengths()
    assert list(lengths.values()) == case.lengths_at(case.R), case.name
    for name, field in byte_fields.items():
        assert lengths[name] == case.want[field], (case.name, name)
    assert all(n > F.CHUNK for n in lengths.values()), (case.name, "an output of at most one chunk", lengths)
    assert any(n > 2 * F.CHUNK for n in lengths.values()), (case.name, "no output of three chunks", lengths)
    assert not F.meets(case.lengths_at(case.R - 1)), (case.name, "R - 1 would do")
    assert max(case.input_bytes) <= F.MAX_INPUT
    for block, tail in case.inputs:                       # whole records, LF only: a repetition starts a record
        assert block[-1] == 10 and tail[-1] == 10 and 13 not in block and 13 not in tail
    return lengths


def test_chunk_is_the_header_s():
    assert F.CHUNK == 32 << 20, "kChunk changed: the cases follow it, look at their sizes and times"
    assert F.EXACT_SIZES == (F.CHUNK - 1, F.CHUNK, F.CHUNK + 1, 2 * F.CHUNK, 2 * F.CHUNK + 1) and F.PIPE_SIZE == 2 * F.CHUNK + 1
    assert F.meets([F.CHUNK + 1, 2 * F.CHUNK + 1]) and not F.meets([F.CHUNK, 2 * F.CHUNK + 1]) and not F.meets([2 * F.CHUNK, 2 * F.CHUNK])


def test_dedup_case(probes, oracle):
    case = F.dedup_case(probes)
    check_case(case, dict(out="bytes_out"))
    assert case.want["duplicates"] == 61 and sorted(set(F.dedup_reps(case.R))) == sorted(F.dedup_reps(case.R))
    # the law on this very block and tail, three repetitions: the oracle on the numbered input
    block, tail = case.inputs[0]
    small = F.dedup_reps(3)
    rng = np.random.default_rng(F.SEEDS["single"])
    b3, f3 = C.single_block(rng, probes)
    t3 = C.single_tail(rng, probes, b3, f3, small)
    assert np.array_equal(b3, block) and t3.size == tail.size
    out, _ = oracle.dedup(np.concatenate([C.numbered(b3, f3, 3), t3]))
    assert out == C.numbered(b3, f3, 3).tobytes() + C.dedup_of(b3, f3, 3, t3)[0]
    pieces = case.input_pieces(0)
    assert len(pieces) == case.R + 1 and bytes(pieces[1][case.fields[0]:case.fields[0] + C.FIELD]) == b"%08x" % 1


def test_merge_case(paired):
    lengths = check_case(F.merge_case(paired), dict(merged="merged_bytes", unmerged1="unmerged1_bytes", unmerged2="unmerged2_bytes"))
    assert len(lengths) == 3


def test_trim_case(paired):
    case = F.trim_case(paired)
    check_case(case, dict(out1="out1_bytes", out2="out2_bytes"))
    assert min(case.want[k] for k in ("cut_overlap", "cut_adapter", "cut_polyg", "cut_quality", "dropped_reads")) > case.R


def test_screen_case(paired):
    case = F.screen_case(paired, F.screen_cindex())
    check_case(case, dict(out1="out1_bytes", out2="out2_bytes"))
    assert case.want["matched_pairs"] > case.R and 0 < case.want["reads_out"] < case.want["reads_in"]


def test_demux_case(refs):
    case = F.demux_case(refs)
    lengths = check_case(case, {})
    rows = case.want["rows"]
    assert len(lengths) == 2 * len(rows) == 12
    for d, w, f in F.demux_names():
        assert lengths[f] == rows[d]["bytes" + w]
    assert sum(r["bytes1"] for r in rows) == case.want["out1_bytes"] and sum(r["bytes2"] for r in rows) == case.want["out2_bytes"]
    # at least two samples whose files start at offsets that are no multiple of 16 inside the device buffer, each longer than a chunk
    assert len(F.unaligned_long_samples(rows)) >= 2, [(r["off1"], r["off2"]) for r in rows]


def test_normalize_case(refs):
    case = F.normalize_case(refs)
    check_case(case, dict(out1="out1_bytes", out2="out2_bytes"))
    w = case.want
    assert min(w["dropped_low"], w["dropped_high"], w["units_out"]) > case.R and len(set(w["classes"].tolist())) == 4
    # the pieces are the kept units' bytes: on the first repetition and the tail, against the rule "a unit's bytes, when kept"
    (b1, t1), Ub = case.inputs[0], (len(w["kept"]) - len(w["len1"].tail))
    Ub //= case.R
    pieces = case.outputs["out1"]()
    at = np.cumsum(w["len1"].block) - w["len1"].block
    first = b"".join(b1[a:a + n].tobytes() for a, n, k in zip(at.tolist(), w["len1"].block.tolist(), w["kept"][:Ub].tolist()) if k)
    assert pieces[0].tobytes() == first and len(pieces) == case.R + 1
    at = np.cumsum(w["len1"].tail) - w["len1"].tail
    last = b"".join(t1[a:a + n].tobytes() for a, n, k in zip(at.tolist(), w["len1"].tail.tolist(), w["kept"][case.R * Ub:].tolist()) if k)
    assert pieces[-1].tobytes() == last
    assert not np.array_equal(w["kept"][:Ub], w["kept"][Ub:2 * Ub]), "the repetitions keep different units"


@pytest.mark.parametrize("size", F.EXACT_SIZES)
def test_exact_size_inputs_are_echoed(probes, size):
    block, R, tail = F.echo_input(F.echo_block(probes), size)
    assert R * block.size + tail.size == size and R >= 1
    assert block[-1] == 10 and tail[-1] == 10 and 13 not in block and 13 not in tail
    wb, wt = trim_of_np(block, None, **F.TRIM_OFF), trim_of_np(tail, None, **F.TRIM_OFF)
    assert wb["out1"] == block.tobytes() and wt["out1"] == tail.tobytes()
    want = C.compose_trim(wb, wt, R)
    assert len(want["out1"]) == want["out1_bytes"] == size and want["reads_out"] == want["reads_in"] and want["out2_bytes"] == 0
    lines = tail.tobytes().split(b"\n")
    assert lines[-5].startswith(b"@x") and lines[-4:] == [b"ACGT", b"+", b"IIII", b""] and len(lines) % 4 == 1


# ---- the two-buffer schedule of device_to_fd --------------------------------------------------------------------------------------

def schedule(n_chunks, buffer_of=lambda k: k & 1, fail_at=None, wait_on_error=True):
    """device_to_fd's host calls for n_chunks, in order: ("issue", k, b) a copy of chunk k into buffer b and a record of ev[b];
    ("wait", b) on ev[b]; ("write", k, b) of buffer b as chunk k, which fails at chunk fail_at; then the return"""
    ops = []
    if not n_chunks:
        return ops
    ops.append(("issue", 0, buffer_of(0)))
    for k in range(n_chunks):
        ops.append(("wait", buffer_of(k)))
        if k + 1 < n_chunks:
            ops.append(("issue", k + 1, buffer_of(k + 1)))
        ops.append(("write", k, buffer_of(k)))
        if k == fail_at:
            if wait_on_error and k + 1 < n_chunks:
                ops.append(("wait", buffer_of(k + 1)))
            break
    return ops


def run(ops):
    """walks a schedule.  A copy may touch its buffer at any moment between its issue and the wait for that buffer's event (copies
    of one stream complete in order, and an event is recorded once per issue).  Returns (the chunks as write() saw them, the
    violations: a write() of a buffer with a copy in flight, the copies still in flight at the return)"""
    flying, holds, seen, bad = {}, {}, [], []
    for op in ops:
        if op[0] == "issue":
            _, k, b = op
            if b in flying:
                bad.append(("two copies into buffer %d" % b, k))
            flying[b] = k
        elif op[0] == "wait":
            b = op[1]
            if b in flying:
                holds[b] = flying.pop(b)
        else:
            _, k, b = op
            if b in flying:
                bad.append(("write() of buffer %d while chunk %d is copied into it" % (b, flying[b]), k))
            seen.append(holds.get(b))
    return seen, bad, flying


@pytest.mark.parametrize("n_chunks", [0, 1, 2, 3, 4, 5])
def test_schedule_never_writes_a_buffer_in_flight(n_chunks):
    ops = schedule(n_chunks)
    seen, bad, flying = run(ops)
    assert seen == list(range(n_chunks)) and not bad and not flying
    # between the wait for a chunk's buffer and the end of its write() no copy is issued into that buffer
    for k in range(n_chunks):
        lo, hi = ops.index(("wait", k & 1), 0 if k == 0 else ops.index(("write", k - 1, (k - 1) & 1))), ops.index(("write", k, k & 1))
        assert not [op for op in ops[lo:hi + 1] if op[0] == "issue" and op[2] == k & 1], (n_chunks, k)
    assert sum(op[0] == "issue" for op in ops) == n_chunks and len({op[2] for op in ops if op[0] == "issue"}) == min(n_chunks, 2)
    # the model can fail: one buffer for every chunk is a write() under a copy from two chunks on
    seen, bad, _ = run(schedule(n_chunks, buffer_of=lambda k: 0))
    assert bool(bad) == (n_chunks >= 2)


@pytest.mark.parametrize("n_chunks", [1, 2, 3, 4, 5])
def test_schedule_leaves_no_copy_in_flight_when_a_write_fails(n_chunks):
    """the caller frees both buffers right after the return (~Pinned): a copy still in flight then would land in freed memory"""
    for k in range(n_chunks):
        seen, bad, flying = run(schedule(n_chunks, fail_at=k))
        assert seen == list(range(k + 1)) and not bad and not flying, (n_chunks, k)
        _, _, flying = run(schedule(n_chunks, fail_at=k, wait_on_error=False))
        assert (len(flying) == 1) == (k + 1 < n_chunks), "without the wait on the error path the next chunk is still on its way"

"""The one path fq-dedup, fq-readstats and fq-cycles share and that only short lines reach: the line index's guess of n / 24 + 1024
lines is too small, its buffers go back to the pool and the index runs a second time at the exact size."""
import threading

import numpy as np
import pytest

from _cycles_check import assert_result, table_of_np
from _readstats_check import assert_summary, per_read_np
from test_gpu_parity import to_dev

pytestmark = pytest.mark.gpu

RECORDS = b"@\nA\n+\nI\n" * 2000
INPUTS = {
    "newlines": b"\n" * 5000,                          # 5000 lines, the guess is 5000 / 24 + 1024 = 1232
    "short_records": RECORDS,                          # 16000 bytes: 8000 lines, the guess is 1690
    "short_records_crlf": RECORDS.replace(b"\n", b"\r\n"),
}
PLACES = ("host", "device", "device_unaligned")       # the host-buffer entry point; a device pointer at offset 0 and at offset 1


def _guess_is_too_small(data):
    return data.count(b"\n") + 1 > len(data) // 24 + 1024


_wanted = {}


def wanted(oracle, name):
    """what the three commands owe for an input, computed once"""
    if name not in _wanted:
        a = np.frombuffer(INPUTS[name], dtype=np.uint8)
        _wanted[name] = dict(a=a, dedup=oracle.dedup(a), readstats=per_read_np(a), cycles=table_of_np(a))
    return _wanted[name]


def run_dedup(torch, scfq, w, place, ptr):
    want, ost = w["dedup"]
    a = w["a"]
    if place == "host":
        got, st = scfq.dedup_host(a)
    else:
        out = torch.zeros(a.size + 16, dtype=torch.uint8, device="cuda")
        nb, st = scfq.dedup_device(ptr, a.size, out.data_ptr(), a.size)
        got = out[:nb].cpu().numpy().tobytes()
    for f in ("total_reads", "duplicates", "records_out", "bytes_out"):
        assert getattr(st, f) == getattr(ost, f), (place, f, getattr(st, f), getattr(ost, f))
    assert got == want, place
    return got, [getattr(st, f) for f in ("total_reads", "duplicates", "records_out", "bytes_out")]


def run_readstats(torch, scfq, w, place, ptr):
    rows, lines = w["readstats"]
    a = w["a"]
    want = np.asarray(rows, dtype=np.int64).reshape(-1, 5)
    if place == "host":
        s = scfq.read_stats_host(a)
        assert_summary(s, want, a.size, lines, place)
        return bytes(s), b""
    tab = torch.full((max(want.shape[0], 1), 5), -1, dtype=torch.int64, device="cuda")
    s = scfq.read_stats_device(ptr, a.size, tab.data_ptr(), want.shape[0])
    got = tab[:want.shape[0]].cpu().numpy()
    assert np.array_equal(got, want), (place, "records differ")
    assert_summary(s, want, a.size, lines, place)
    return bytes(s), got.tobytes()


def run_cycles(torch, scfq, w, place, ptr):
    want = w["cycles"]
    a = w["a"]
    cap = max(want[2], want[3]) + 1
    got = scfq.cycles_host(a, cap) if place == "host" else scfq.cycles_device(ptr, a.size, cap)
    assert_result(got, *want, a.size, cap, place)
    return bytes(got[0]), got[1].tobytes()


RUN = {"dedup": run_dedup, "readstats": run_readstats, "cycles": run_cycles}


@pytest.mark.parametrize("command", sorted(RUN))
@pytest.mark.parametrize("name", sorted(INPUTS))
def test_second_round_of_the_index(gpu, scfq, oracle, command, name):
    torch = gpu
    assert _guess_is_too_small(INPUTS[name])
    w = wanted(oracle, name)
    for place in PLACES:
        t, ptr = (None, 0) if place == "host" else to_dev(torch, w["a"], 1 if place == "device_unaligned" else 0)
        assert place == "host" or ptr % 16 == (1 if place == "device_unaligned" else 0)
        # twice in a row: the second call takes the stream the first one returned, and nothing of the first is left
        before = scfq.lib().scfq_device_bytes_now()
        first = RUN[command](torch, scfq, w, place, ptr)
        assert scfq.lib().scfq_device_bytes_now() == before, (place, "first call")
        again = RUN[command](torch, scfq, w, place, ptr)
        assert again == first, (place, "the second call differs")
        assert scfq.lib().scfq_device_bytes_now() == before, (place, "second call")


def test_three_pipelines_from_four_threads(gpu, scfq, oracle):
    """the pool and the list of idle streams under more than one pipeline at once: four host threads, twenty calls each"""
    torch = gpu
    w = wanted(oracle, "short_records")
    t, ptr = to_dev(torch, w["a"])
    commands = ("readstats", "cycles", "dedup", "readstats")
    single = {c: RUN[c](torch, scfq, w, "device", ptr) for c in set(commands)}
    torch.cuda.synchronize()
    failures = []

    def worker(c):
        try:
            torch.cuda.set_device(0)
            scfq.set_wait_stream(torch.cuda.current_stream().cuda_stream)      # (per host thread)
            for k in range(20):
                if RUN[c](torch, scfq, w, "device", ptr) != single[c]:
                    failures.append((c, k, "differs from the single-threaded result"))
        except BaseException as e:      # (an assertion in a thread is otherwise lost)
            failures.append((c, repr(e)))

    threads = [threading.Thread(target=worker, args=(c,)) for c in commands]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not failures, failures[:4]

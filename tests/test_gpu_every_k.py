"""Every k a k-mer pipeline accepts, on the device: fq-kmers (k = 1 .. 12), fq-kcount (13 .. 32), fq-screen (8 .. 32) and fq-normalize
(13 .. 32) on the case set of tests/_every_k_cases.py, plain and canonical where the pipeline has the choice, the device pointer at
offsets 0, 5 and 11 from a 16-byte boundary, against the Python checkers with ==.  test_every_k_cases_host.py shows that the case set
tells a right key, mask or shift from a wrong one at each k."""
import numpy as np
import pytest

from _every_k_cases import OFFSETS, cases, fastq_of
from _kcount_check import CANONICAL, kcount_of_np
from _kmers_check import kmers_of_np
from _normalize_cases import every_k_one
from _screen_check import assert_summary, index_of, screen_of_np
from test_gpu_kcount import check_device as kcount_check_device
from test_gpu_kmers import check_call
from test_gpu_normalize import child
from test_gpu_parity import to_dev
from test_gpu_screen import check_device as screen_check_device

pytestmark = pytest.mark.gpu

MODES = (0, CANONICAL)


@pytest.mark.parametrize("k", range(1, 13))
def test_kmers(gpu, scfq, k):
    """the whole table and every field of the summary; k = 5 and k = 6 are the two layouts with fewer than 64 copies of the LDS counters"""
    a = np.frombuffer(cases(k).fastq, dtype=np.uint8)
    for flags in MODES:
        want = kmers_of_np(a, k, flags != 0)
        for offset in OFFSETS:
            t, ptr = to_dev(gpu, a, offset)
            check_call(scfq, lambda tb: scfq.kmers_device(ptr, a.size, k, flags, tb), want, k, flags, a.size, ("every k, device", offset))
        check_call(scfq, lambda tb: scfq.kmers_host(a, k, flags, tb), want, k, flags, a.size, "every k, host")


@pytest.mark.parametrize("k", range(13, 33))
def test_kcount(gpu, scfq, k):
    """the summary and the dump at every offset; at offset 0 also the histogram, every present key and absent ones through query"""
    a = np.frombuffer(cases(k).fastq, dtype=np.uint8)
    for flags in MODES:
        want = kcount_of_np(a, k, flags != 0)
        for offset in OFFSETS:
            kcount_check_device(gpu, scfq, a, k, flags, ("every k", offset), offset=offset, want=want, full=offset == 0)


@pytest.mark.parametrize("k", range(8, 33))
def test_screen(gpu, scfq, k):
    """the index summary, then records, statistics and output bytes: single-end, and the same reads with "\\r\\n" as pairs"""
    c = cases(k)
    cindex = index_of(c.refs, k)
    crlf = fastq_of([(s, b"\r\n") for part in c.parts.values() for s, e in part], final=True)
    with scfq.screen_index_host(c.refs, k) as dindex:
        assert_summary(dindex.summary, cindex, k)
        assert int(dindex.summary.slots) == cindex["slots"]
        want = screen_of_np(cindex, np.frombuffer(c.fastq, dtype=np.uint8), min_hits=1)
        for offset in OFFSETS:
            screen_check_device(gpu, scfq, dindex, cindex, c.fastq, None, dict(min_hits=1), ctx=("every k", k, offset), offs=(offset, 0), want=want)
        screen_check_device(gpu, scfq, dindex, cindex, crlf, None, dict(interleaved=True, min_hits=2, min_hit_pct=5), ctx=("every k, pairs", k), offs=(5, 0))


@pytest.mark.parametrize("k", range(13, 33))
def test_normalize(gpu, scfq, k):
    """records, statistics, histogram and output bytes against a table counted from the case set itself, given and in the two-pass form"""
    assert every_k_one(gpu, scfq, k) == 10


def test_normalize_counts_in_device_memory():
    """the same sweep in a child process in which a wave keeps 64 windows in LDS: the reads of 65 and more windows select from device
    memory at every k"""
    assert child("cases", "every_k", 64, SCFQ_NORM_LDS_WINDOWS="64") == dict(rc=0, case="every_k", calls=80)

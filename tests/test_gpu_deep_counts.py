"""Counts past 32 bits through fq-kcount and its consumer fq-normalize.  One device buffer of about 10 GiB, made here with torch: a single
record whose sequence line is the four homopolymer runs of tests/_deep_counts_cases.py (A x (2^32 + 4096), T x (2^32 + 8192),
C x (2^31 + 5), G x (2^24 + 1), an 'N' between them).  The table it has to give is arithmetic — L - k + 1 per run — so nothing is
compared with a pass over the data outside the library: fq-kcount against the arithmetic, fq-normalize of a small read set against the
checker on the arithmetic table, where the depth saturates at SCFQ_NORM_MAX_DEPTH = 2^32 - 2 next to the marker 2^32 - 1.  Every
comparison is ==.  test_every_k_cases_host.py shows that the read set's records take every shape of the saturation."""
import numpy as np
import pytest

import _deep_counts_cases as deep
from _kcount_check import canonical_key
from _kmers_check import index_of
from _normalize_cases import check_device

pytestmark = pytest.mark.gpu

SUMMARY = ("reads", "lines", "input_bytes", "k", "flags", "windows", "kmers", "skipped", "short_lines", "distinct", "unique", "max_count")


@pytest.fixture(scope="module")
def deep_buffer(gpu):
    torch = gpu
    buf = torch.full((deep.INPUT_BYTES,), ord("N"), dtype=torch.uint8, device="cuda")
    buf[:len(deep.HEAD)] = torch.tensor(list(deep.HEAD), dtype=torch.uint8)
    for letter, at, n in deep.run_offsets():
        buf[at:at + n] = letter[0]
    buf[deep.INPUT_BYTES - len(deep.TAIL):] = torch.tensor(list(deep.TAIL), dtype=torch.uint8)
    yield buf
    del buf
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", params=deep.TABLES, ids=lambda p: "%d-%s" % (p[0], "canonical" if p[1] else "plain"))
def counted(request, scfq, deep_buffer):
    """(k, canonical, summary, table): one pass of fq-kcount over the buffer per table, shared by the tests below"""
    k, canonical = request.param
    s, t = scfq.kcount_device(deep_buffer.data_ptr(), deep_buffer.numel(), k=k, flags=1 if canonical else 0)
    with t:
        yield k, canonical, s, t


def test_kcount_is_the_arithmetic(counted):
    k, canonical, s, t = counted
    want, table = deep.summary_of(k, canonical), deep.table_of(k, canonical)
    assert {name: int(getattr(s, name)) for name in SUMMARY} == want
    assert int(s.passes) == 1 and int(s.slots) >= 1024
    assert [tuple(r) for r in t.dump().tolist()] == sorted(table.items())
    assert [tuple(r) for r in t.dump(2 ** 32).tolist()] == sorted((key, c) for key, c in table.items() if c >= 2 ** 32)
    # either strand in canonical mode; the all-ones key (32 x T at k = 32); keys that are absent
    full = 4 ** k - 1
    ask = [index_of(letter * k) for letter, _ in deep.RUNS] + [1, full - 1, index_of(b"A" * (k - 1) + b"C"), 0x123456789ABCDEF & full]
    assert ask[1] == full
    assert t.query(np.array(ask, dtype=np.uint64)).tolist() == [table.get(canonical_key(v, k) if canonical else v, 0) for v in ask]
    assert t.query([full, 0]).tolist() == ([table[0]] * 2 if canonical else [table[full], table[0]])
    assert t.hist(2).tolist() == [0, len(table)]
    # every count lies above 2^20: the last bin, far behind the bins that the histogram kernel keeps in LDS
    h = t.hist(1 << 20)
    assert int(h[-1]) == len(table) and not h[:-1].any()


def test_normalize_at_the_saturated_depth(gpu, scfq, counted):
    """records, statistics, histogram and output bytes of the read set: every shape of the select at depths up to 2^32 - 2, the key
    without a slot at k = 32 in plain mode, a read of more than 2048 windows, and the keep rule at D = 2^32 - 2 for each target"""
    k, canonical, s, t = counted
    table, data = deep.table_of(k, canonical), deep.fastq_reads(k)
    for kw in deep.CALLS:
        want, got = check_device(gpu, scfq, t, table, k, canonical, data, ctx=("deep", k, canonical), **kw)
        assert int(got.distinct) == len(table)

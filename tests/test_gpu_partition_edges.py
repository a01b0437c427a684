"""fq-readstats, fq-cycles, fq-kmers and fa-gc on the device at the edges of their partitions: the inputs of tests/_partition_cases.py
(pinned by tests/test_partition_cases_host.py) through the helpers and checkers of the four pipelines' own GPU tests.  Every
comparison is ==.  to_dev's guard bytes are 'G', so a read outside the input changes the counts; the readstats table is handed
over full of -1, so a record nobody zeroed shows."""
import numpy as np
import pytest

import _partition_cases as pc
import test_gpu_cycles as cy
import test_gpu_fa_gc as fa
import test_gpu_kmers as km
import test_gpu_readstats as rs
from _cycles_check import table_of_np
from _kmers_check import CANONICAL, index_of
from test_gpu_parity import to_dev

pytestmark = pytest.mark.gpu

K = pc.kernel_constants()
KM_STEP = 16 * K["kKmThreads"]
KS = (1, 7, 8, 12)


# ---- fq-readstats ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1, 15])
def test_r1_lds_cap(gpu, scfq, offset):
    """C - 1 .. C + 2 lines in the middle tile of three, the first of them at every phase of a record"""
    for label, a, facts in pc.r1_lds_cap(K["kRsTile"], K["kRsLineCap"], offset):
        rs.check_buffer(gpu, scfq, a, label, offset=offset)


@pytest.mark.parametrize("first_pad", range(0, 130, 26))
def test_r2_dense_and_sparse_borders(gpu, scfq, first_pad):
    """sparse, dense, sparse inside one line, dense, dense, sparse: every border kind cuts a record at every place"""
    for label, a, facts in pc.r2_borders(K["kRsTile"], K["kRsLineCap"], range(first_pad, first_pad + 26)):
        rs.check_buffer(gpu, scfq, a, label)


# ---- fq-cycles -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("longest", pc.C1_LONGEST)
def test_c1_lane_tiers(gpu, scfq, longest):
    """the group's longest line on both sides of every change of the lanes per line"""
    for label, a, facts in pc.c1_lane_tiers(longest):
        want = table_of_np(a)
        assert max(want[2], want[3]) == longest
        caps = sorted({0, 1, longest - 1, longest, longest + 5})
        for offset in range(16):
            cy.check_buffer(gpu, scfq, a, (label, offset), offset=offset, want=want, caps=caps)


@pytest.mark.parametrize("top", pc.c2_tops(K["kCyWin"]))
def test_c2_window_edge(gpu, scfq, top):
    """the group's longest line on both sides of every change of the number of windows, at every place in its first chunk"""
    win = K["kCyWin"]
    label, a, facts = pc.c2_window_edge(win, top)
    want = table_of_np(a)
    assert max(want[2], want[3]) == top
    caps = sorted({0, win - 16, win - 15, win - 1, win, win + 1, top, top + 1})
    for offset in (0, 5, 15):
        cy.check_buffer(gpu, scfq, a, (label, offset), offset=offset, want=want, caps=caps)


@pytest.mark.parametrize("variant", range(8))
def test_c3_group_edge(gpu, scfq, variant):
    """a record less and more than a group, a last group of one sequence line, a group without windows among groups with some"""
    label, a, facts = list(pc.c3_group_edge(K["kCyGroup"]))[variant]
    cy.check_buffer(gpu, scfq, a, label, offset=3, caps=(0, 25))


# ---- fq-kmers --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("ending", pc.K1_ENDINGS)
@pytest.mark.parametrize("shift", range(16))
def test_k1_behind_the_input(gpu, scfq, shift, ending, k):
    """the position behind the input in a chunk, a wave, a step and a block of its own, behind four kinds of last line"""
    for label, a, facts in pc.k1_behind_the_input(KM_STEP, shift, (ending,)):
        km.check_buffer(gpu, scfq, a, (k,), label, offset=shift)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("deltas", [pc.K2_DELTAS[:8], pc.K2_DELTAS[8:]], ids=["before", "around"])
@pytest.mark.parametrize("eol", [pc.LF, pc.CRLF], ids=["lf", "crlf"])
@pytest.mark.parametrize("shift", [0, 9])
@pytest.mark.parametrize("edge", [1024, KM_STEP])
def test_k2_edges_inside(gpu, scfq, edge, shift, eol, deltas, k):
    """a line end at every place around a wave's and a step's edge, and a letter that is no base next to it"""
    for label, a, facts in pc.k2_edges_inside(edge, shift, (eol,), deltas):
        km.check_buffer(gpu, scfq, a, (k,), label, offset=shift)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("m", pc.K3_RUNS)
def test_k3_merge(gpu, scfq, m, k):
    """runs of one letter next to runs of its complement: the checker, and the literal tables"""
    for label, a, facts in pc.k3_merge(m):
        aligned = (-facts["run_starts"][0]) % 16                   # the second run begins on a lane's first byte
        for offset in (0, aligned):
            km.check_buffer(gpu, scfq, a, (k,), (label, offset), offset=offset)
        t, ptr = to_dev(gpu, a, aligned)
        homo = m - k + 1                                           # windows inside one run
        first, second = (b"A", b"T") if facts["runs"] == "ATA" else (b"C", b"G")
        times = 2 if facts["runs"] == "ATA" else 1                 # A T A: the first letter has two runs
        s, table = scfq.kmers_device(ptr, a.size, k, 0, km.table_buf(k))
        assert (s.windows, s.kmers, s.skipped, s.short_lines) == (facts["seq_len"] - k + 1, facts["seq_len"] - k + 1, 0, 0), label
        assert int(table[index_of(first * k)]) == times * homo and int(table[index_of(second * k)]) == homo, label
        s, table = scfq.kmers_device(ptr, a.size, k, CANONICAL, km.table_buf(k))
        assert int(table[index_of(first * k)]) == (times + 1) * homo and int(table[index_of(second * k)]) == 0, label
        assert int(table[:4 ** k].sum()) == s.kmers == facts["seq_len"] - k + 1, label
        if facts["runs"] == "ATA":
            assert int(table[0]) == 3 * homo, label                # every window inside a run, A or T, is index 0


# ---- fa-gc -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", pc.fa_offsets(K["kFaTileBytes"], K["kFaStepBytes"]))
def test_fa_first_tile_and_step_edges(gpu, scfq, off):
    """the input's first byte around a step edge and in the last bytes of a tile: a first tile of 1 .. 16 bytes, and a later
    tile (or step) that looks back at the input's first byte"""
    T = K["kFaTileBytes"]
    assert T == fa.T
    rng = np.random.default_rng(100 + off)
    for n in (1, 17, T + 1, 2 * T + 1):
        fa.check_at_offset(scfq, gpu, fa.mixed_input(rng, n, off), off, rng, ("mixed", n, off))
    for label, data in fa.long_inputs():
        fa.check_at_offset(scfq, gpu, np.frombuffer(data, dtype=np.uint8), off, rng, (label, off))
    for data in (b"\n>a\nAC", b">"):
        fa.check_at_offset(scfq, gpu, np.frombuffer(data, dtype=np.uint8), off, rng, (data, off))

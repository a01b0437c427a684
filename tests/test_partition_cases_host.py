"""The inputs of tests/_partition_cases.py, pinned on the CPU before a device sees them: every case has, in its bytes, the property
it was built for (found here from the line starts, with nothing of the generator's arithmetic), the slow and the fast checkers
agree on it, and the Python model of the readstats partition writes every table entry of the R1 cases exactly once."""
import itertools

import numpy as np

import _partition_cases as pc
from _cycles_check import table_of, table_of_np
from _kmers_check import kmers_of, kmers_of_np
from _readstats_check import line_spans_np, lines_of, per_read, per_read_np
from test_readstats_partition_model import run_model

K = pc.kernel_constants()
SMALL = 20_000           # bytes up to which the byte-by-byte checkers run
HOST_SHIFTS = (0, 9, 15)


def line_starts(a):
    """start of every line, and one entry behind the last: where the next line would start"""
    starts, tends = line_spans_np(a)
    return starts, tends, np.concatenate([starts, [a.size + 1]])


def lines_with_a_byte_in(starts, lo, hi):
    """(first, last) line that has a byte, text or newline, in [lo, hi)"""
    return int(np.searchsorted(starts, lo, side="right")) - 1, int(np.searchsorted(starts, hi, side="left")) - 1


def checkers_agree(a):
    """the byte-by-byte checkers of the three FASTQ pipelines against their numpy forms; returns whether the case was small enough"""
    if a.size > SMALL:
        return False
    data = a.tobytes()
    rows, lines = per_read_np(a)
    assert rows.tolist() == [list(r) for r in per_read(data)] and lines == len(lines_of(data))
    slow, fast = table_of(data), table_of_np(a)
    assert np.array_equal(slow[0], fast[0]) and slow[1:] == fast[1:]
    for k, canonical in ((1, False), (7, True), (12, False), (12, True)):
        assert kmers_of(data, k, canonical) == kmers_of_np(a, k, canonical), (k, canonical)
    return True


def test_constants_are_the_kernels():
    assert set(K) == {"kRsTile", "kRsLineCap", "kCyGroup", "kCyWin", "kKmThreads", "kFaTileBytes", "kFaStepBytes"}
    assert all(isinstance(v, int) and v > 0 for v in K.values())
    assert pc.c2_tops(1024) == (1008, 1009, 1010, 1023, 1024, 1025, 2033, 2034)
    assert pc.k1_totals(8192) == (1023, 1024, 1025, 8191, 8192, 8193, 16384)
    assert pc.fa_offsets(4096, 1024) == (1008, 1023, 1024, 1025, 2047, 2048, 4079, 4080, 4081, 4095)
    assert sorted({t % 16 for t in pc.k1_totals(16 * K["kKmThreads"]) if t < 16 * K["kKmThreads"]}) == [0, 1, 15]


def test_r1_lines_in_the_middle_tile_and_the_model():
    T, C = K["kRsTile"], K["kRsLineCap"]
    seen = set()
    for offset in (0, 1, 15):
        for label, a, facts in pc.r1_lds_cap(T, C, offset):
            starts, tends, nxt = line_starts(a)
            assert 2 * T < a.size + offset <= 3 * T, label
            first, last = lines_with_a_byte_in(starts, T - offset, 2 * T - offset)
            assert (last - first + 1, first & 3) == (facts["lines_in_middle"], facts["phase"]), label
            assert facts["dense"] == (last - first + 1 > C), label
            assert starts[first] < T - offset, label                                  # the first of them comes from the tile before
            assert (nxt[last + 1] == 2 * T - offset) == facts["ends_on_border"], label
            for lo, hi in ((0, T - offset), (2 * T - offset, a.size)):                # the outer tiles: records of 1 to 3 KB
                f, l = lines_with_a_byte_in(starts, lo, hi)
                assert l - f + 1 <= 200, label
                inner = [r for r in range((f + 3) // 4, (l + 1) // 4 - 1) if starts[4 * r] >= lo and nxt[4 * r + 4] <= hi and
                         not (lo and r == (f + 3) // 4)]
                assert inner and all(1000 <= nxt[4 * r + 4] - starts[4 * r] <= 3000 for r in inner), label
            data = a.tobytes()
            assert run_model(data, T, offset, C) == per_read(data) == [tuple(r) for r in per_read_np(a)[0].tolist()], label
            seen.add((facts["lines_in_middle"] - C, facts["phase"], offset))
    assert seen == set(itertools.product((-1, 0, 1, 2), range(4), (0, 1, 15)))


def cut_kind(a, starts, x):
    """where a border in front of byte x cuts the record it lies in"""
    k = int(np.searchsorted(starts, x, side="right")) - 1
    at_start = int(starts[k]) == x
    if at_start and k % 4 == 0:
        return "record_start"
    if a[x] == 10:
        return "cr_lf" if a[x - 1] == 13 else "lf"
    if a[x] == 13 and a[x + 1] == 10:
        return "on_the_cr"
    if k % 4 == 1:
        return "seq_first" if at_start else "seq"
    return "line_start" if at_start else ("header", None, "plus", "qual")[k % 4]


def test_r2_every_border_kind_meets_every_cut():
    T, C = K["kRsTile"], K["kRsLineCap"]
    pairs, crossed_by_long_line = set(), 0
    for label, a, facts in pc.r2_borders(T, C):
        assert a.size <= 6 * T and a.size > 5 * T and facts["offset"] == 0, label
        starts, tends, nxt = line_starts(a)
        kinds = ""
        for t in range(6):
            f, l = lines_with_a_byte_in(starts, t * T, min((t + 1) * T, a.size))
            kinds += "D" if l - f + 1 > C else "S"
            if kinds[-1] == "D":
                assert 3 * C // 2 <= l - f + 1 <= 5 * C // 2, (label, t, l - f + 1)          # about 2 C
        assert kinds == facts["tiles"] == pc.R2_TILES, (label, kinds)
        f, l = lines_with_a_byte_in(starts, 2 * T, 3 * T)
        assert f == l and f % 4 == 1, label                                            # tile 2: inside one sequence line
        crossed_by_long_line += 1
        for t in range(1, 6):
            pairs.add((kinds[t - 1] + kinds[t], cut_kind(a, starts, t * T)))
        if facts["pad"] == 0:
            short = [r for r in range(starts.size // 4) if nxt[4 * r + 4] - starts[4 * r] < 64]
            crlf = [r for r in short if a[nxt[4 * r + 1] - 2] == 13]
            assert len(short) > C and abs(3 * len(crlf) - len(short)) <= 6, label          # every third one has "\r\n"
    wanted = set(itertools.product(("SD", "DS", "DD"), pc.R2_CUTS))
    assert {p for p in pairs if p[1] in pc.R2_CUTS} == wanted, sorted(wanted - pairs)
    assert crossed_by_long_line == len(pc.R2_PADS) == 130


def odd_line_lengths(a):
    starts, tends = line_spans_np(a)
    return starts[1::2], (tends - starts)[1::2], starts.size


def test_c1_longest_line_of_the_group():
    assert pc.C1_LONGEST == (1, 48, 49, 50, 112, 113, 114, 240, 241, 242, 496, 497, 498)
    for longest in pc.C1_LONGEST:
        cases = list(pc.c1_lane_tiers(longest))
        assert [c[2]["longest_in"] for c in cases] == ["seq", "qual"]
        for label, a, facts in cases:
            table, lines, ms, mq = table_of_np(a)
            assert lines == 4 * 67 == 4 * facts["records"] and lines // 2 <= K["kCyGroup"], label          # one group
            assert max(ms, mq) == longest and (ms > mq) == (facts["longest_in"] == "seq") and ms != mq, label
            s, lens, _ = odd_line_lengths(a)
            assert lens.min() == 0 and len(set(lens.tolist())) >= min(longest + 1, 40), label
            assert b"\r\n" in a.tobytes() and b"\n@" in a.tobytes().replace(b"\r\n@", b""), label          # mixed line ends
            if longest >= 48:
                assert np.count_nonzero(table[:, 1:6].sum(axis=1) < table[:, 0]) > 0 and (table[:8, 1:6] > 0).all(), label      # every letter, and others
            checkers_agree(a)


def test_c2_longest_line_and_where_the_long_lines_start():
    win = K["kCyWin"]
    for top in pc.c2_tops(win):
        label, a, facts = pc.c2_window_edge(win, top)
        s, lens, lines = odd_line_lengths(a)
        assert lines == 4 * 100 and lens.max() == top == facts["top"], label
        long_at = s[lens == top]
        assert sorted((long_at % 16).tolist()) == list(range(16)) == facts["d_values"], label
        kinds = np.flatnonzero(lens == top) & 1
        assert 0 < kinds.sum() < kinds.size, label                                    # sequence lines and quality lines
        assert (lens < 500).sum() >= 160, label
        assert set(lens[lens >= 500].tolist()) == {v for v in pc.c2_tops(win) if v <= top}, label
        assert table_of_np(a)[2:] in ((top, top),), label
        checkers_agree(a)


def test_c3_group_populations():
    group = K["kCyGroup"]
    per = group // 2
    got = {}
    for label, a, facts in pc.c3_group_edge(group):
        s, lens, lines = odd_line_lengths(a)
        odd = lines // 2
        assert lens.size == odd and lens.max() <= 20 and (lines + 3) // 4 == facts["records"], label
        populations = [min(group, odd - g * group) for g in range(0, (odd + group - 1) // group)]
        assert populations == facts["populations"], label
        ends_in_sequence = lines % 4 == 2 and a[-1] != 10
        assert ends_in_sequence == facts["ends_in_sequence"], label
        empty = [g for g in range(len(populations)) if lens[g * group:(g + 1) * group].max() == 0]
        assert empty == ([] if facts["empty_group"] is None else [facts["empty_group"]]), label
        got[label.split("/")[1]] = (facts["records"], populations)
        checkers_agree(a)
    assert got == {"one_less": (per - 1, [group - 2]), "whole": (per, [group]), "one_more": (per + 1, [group, 2]),
                   "two_and_one": (2 * per + 1, [group, group, 2]), "two_and_a_sequence_line": (2 * per + 1, [group, group, 1]),
                   "empty_group_0": (3 * per, [group] * 3), "empty_group_1": (3 * per, [group] * 3), "empty_group_2": (3 * per, [group] * 3)}


def test_k1_residues_and_endings():
    step = 16 * K["kKmThreads"]
    seen = set()
    for shift in HOST_SHIFTS:
        for label, a, facts in pc.k1_behind_the_input(step, shift):
            total = shift + a.size
            assert total == facts["total"] and total % 16 == facts["residue"], label
            data = a.tobytes()
            ls = lines_of(data)
            assert len(ls) % 4 == 2 and ls[-1] == facts["last_line"], label          # the input ends in a sequence line
            ending = "lf" if data.endswith(b"\n") else "long_cr" if data.endswith(b"\r") else "long" if len(ls[-1]) >= 12 else "short"
            assert ending == facts["ending"] and (ending != "short" or 1 <= len(ls[-1]) < 7), label
            seen.add((total, ending))
            checkers_agree(a)
    assert seen == set(itertools.product((1023, 1024, 1025, step - 1, step, step + 1, 2 * step), pc.K1_ENDINGS))


def test_k2_line_ends_and_the_odd_letter():
    step = 16 * K["kKmThreads"]
    for edge in (1024, step):
        for shift in (0, 9):
            seen = set()
            for label, a, facts in pc.k2_edges_inside(edge, shift):
                starts, tends = line_spans_np(a)
                at, eol = facts["eol_at"], facts["eol"]
                assert a[at:at + len(eol)].tobytes() == eol and at + shift - edge == facts["delta"], label
                k = int(np.searchsorted(starts, at, side="right")) - 1 if a[at - 1] != 10 else -1
                assert k % 4 == 1 and tends[k] == at and at - starts[k] >= 12, label          # the end of a sequence line's text
                assert tends[k + 2] == starts[k + 2] and tends[k + 4] - starts[k + 4] == 60, label      # an empty quality line, the next read
                bad = facts["bad_at"]
                j = int(np.searchsorted(starts, bad, side="right")) - 1
                assert j % 4 == 1 and bad < tends[j] and a[bad] == ord("N") and abs(bad + shift - edge) <= 12, label
                seq_text = np.concatenate([a[starts[i]:tends[i]] for i in (k, k + 4)])
                assert (seq_text == ord("N")).sum() == 1 and np.isin(seq_text, np.frombuffer(b"ACGTN", dtype=np.uint8)).all(), label
                seen.add((facts["delta"], eol))
                checkers_agree(a)
            assert seen == set(itertools.product(range(-13, 3), (b"\n", b"\r\n")))


def test_k3_runs():
    assert pc.K3_RUNS == (15, 16, 17, 1024, 1025, 5000)
    for m in pc.K3_RUNS:
        (l1, a1, f1), (l2, a2, f2) = pc.k3_merge(m)
        assert lines_of(a1.tobytes())[1] == b"A" * m + b"T" * m + b"A" * m and lines_of(a2.tobytes())[1] == b"C" * m + b"G" * m
        assert len(lines_of(a1.tobytes())) == len(lines_of(a2.tobytes())) == 4
        for a, f in ((a1, f1), (a2, f2)):
            changes = (np.flatnonzero(a[4:3 + f["seq_len"]] != a[3:2 + f["seq_len"]]) + 4).tolist()
            assert changes == f["run_starts"] and len(changes) == len(f["runs"]) - 1, f      # where the letter changes
        for a in (a1, a2):
            checkers_agree(a)

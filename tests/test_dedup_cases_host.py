"""The inputs of tests/_dedup_cases.py, pinned on the CPU before a device sees them: for every case the oracle and the independent
Python statement of fq_dedup.nim (test_property_host.dedup_reference) give the same bytes and counts, those are the bytes and
counts the generator promises, and the case has — in its bytes — the property it was built for."""
import ctypes

import numpy as np

import _dedup_cases as dc
from conftest import OracleDedupStats
from test_property_host import dedup_reference, nim_lines


def echoed(record):
    return b"".join(line + b"\n" for line in nim_lines(record))


def header_of(record):
    lines = nim_lines(record)
    return lines[0] if lines else b""


def check_case(oracle, name, data, exp, python_reference=True):
    """oracle == Python statement == what the generator promises; returns the oracle's bytes"""
    records, kept = exp["records"], exp["kept"]
    assert b"".join(records) == data, name
    assert len(records) == len(kept) and exp["duplicates"] == kept.count(False), name
    want = b"".join(echoed(r) for r, k in zip(records, kept) if k)
    got, st = oracle.dedup(data)
    assert got == want, name
    n_lines = len(nim_lines(data))
    assert (st.total_reads, st.duplicates, st.records_out, st.bytes_out) == (n_lines // 4, exp["duplicates"], kept.count(True), len(want)), name
    assert (n_lines + 3) // 4 == len(records), name             # a record starts at every fourth line, nowhere else
    if python_reference:
        out, n_reads, n_dups = dedup_reference(data)
        assert (out, n_reads, n_dups) == (want, n_lines // 4, exp["duplicates"]), name
    return got


def test_tail_compare(oracle):
    seen_L = []
    for name, data, exp in dc.cases("tail_compare"):
        check_case(oracle, name, data, exp)
        L, ps = exp["L"], exp["positions"]
        seen_L.append(L)
        headers = [header_of(r) for r in exp["records"]]
        base = headers[0]
        assert 40 <= len(headers) <= 60, (name, len(headers))
        assert ps == [p for p in sorted({64, 65, L - 2, L - 1}) if 64 <= p < L], name
        for r in exp["records"]:
            assert 1 <= len(nim_lines(r)[1]) <= 40, name
        met = set()
        for i, h in enumerate(headers):
            assert len(h) == L, (name, i)
            where = [k for k in range(L) if h[k] != base[k]]
            d = exp["diff_at"][i]
            assert where == ([] if d is None else [d]), (name, i, where)        # exactly one byte, where the case says
            if d != 63:
                assert h[:64] == base[:64], (name, i)                            # eight equal masked words: the walk decides
            if exp["dup_of"][i] is not None:
                assert not exp["kept"][i] and h == headers[exp["dup_of"][i]] and exp["dup_of"][i] < exp["n_first"] <= i, (name, i)
                met.add(exp["diff_at"][i])
            else:
                assert exp["kept"][i] and h not in headers[:i], (name, i)
        assert met == set(ps) | {None}, name                                    # a true duplicate of the base and of a variant of every p
        assert 63 in exp["diff_at"], name
        for p in ps:                                                            # two headers that differ at p alone, from each other too
            assert sum(1 for d, u in zip(exp["diff_at"], exp["dup_of"]) if d == p and u is None) >= 2, (name, p)
    assert tuple(seen_L) == dc.TAIL_L == (64, 65, 66, 71, 72, 73, 127, 128, 129, 255, 256, 257, 300)


def masked_words(h):
    return h[:64].ljust(64, b"\0")


def test_length_only(oracle):
    (name, data, exp), = dc.cases("length_only")
    check_case(oracle, name, data, exp)
    headers = [header_of(r) for r in exp["records"]]
    n_first = exp["n_first"]
    assert headers[:n_first] == headers[n_first:] and len(set(headers[:n_first])) == n_first
    assert exp["kept"] == [True] * n_first + [False] * n_first
    for i in exp["empty_at"]:
        assert headers[i] == b""
    kinds = {"nul": 0, "text": 0}
    for i, j, kind in exp["pairs"]:
        a, b = headers[i], headers[j]
        assert len(a) < len(b) and b.startswith(a), (i, j)
        if kind == "nul":
            assert set(b[len(a):]) == {0} and masked_words(a) == masked_words(b), (i, j)      # only the length tells them apart
        else:
            assert 0 not in b and (masked_words(a) != masked_words(b)) == (len(a) < 64), (i, j)      # (the words hold 64 bytes)
        kinds[kind] += 1
    assert kinds["nul"] and kinds["text"]
    lengths = {(len(headers[i]), len(headers[j])) for i, j, kind in exp["pairs"] if kind == "nul"}
    assert {(2, 3), (2, 4), (3, 4), (7, 8), (7, 9), (8, 9), (15, 16), (15, 17), (16, 17), (63, 64), (63, 65), (64, 65)} <= lengths
    assert b"@a" in headers and b"@a\0" in headers and b"@a\0\0" in headers


def test_input_ends(oracle):
    small_sizes, literal, behind = set(), set(), set()
    terminators = dict(none=b"", lf=b"\n", cr=b"\r", crlf=b"\r\n")
    for name, data, exp in dc.cases("input_ends"):
        check_case(oracle, name, data, exp)
        term, m = terminators[exp["terminator"]], exp["m"]
        assert data.endswith(term) and (exp["terminator"] != "none" or data[-1:] not in (b"\r", b"\n")), name
        last = data[len(data) - len(term) - m:len(data) - len(term)]
        assert len(last) == m and (len(data) == m + len(term) or data[len(data) - len(term) - m - 1:][:1] == b"\n"), name
        for r in exp["records"][:-1]:
            assert r.count(b"\n") == 4 and r.endswith(b"\n") and b"\r" not in r, name
        earlier = [header_of(r) for r in exp["records"][:-1]]
        if earlier:
            twins = [h for h in earlier if len(h) == m and h[:-1] == last[:-1] and h.islower()]       # (the fillers are upper case)
            assert len(twins) == 1 and (twins[0] == last) == exp["equal"], name      # equal, or different in its last byte alone
        # ('\r' without '\n' stays in the header: the last record is then no duplicate even of its twin)
        assert exp["kept"][-1] == (not earlier or not exp["equal"] or exp["terminator"] == "cr"), name
        if name.startswith("input_ends/n="):
            assert len(data) == int(name.split("=")[1].split(",")[0]) <= 40, name
            for h in earlier:
                assert 1 <= len(h) <= 17 and data.count(b"\n\n\n\n") == len(earlier), name
            small_sizes.add((len(data), exp["terminator"]))
            literal.add(data)
        else:
            assert 5000 <= len(data) - m - len(term) < 5200, name
            behind.add((m + len(term), exp["equal"]))
    assert small_sizes >= {(n, t) for n in range(1, 41) for t in terminators if n >= len(terminators[t]) + 1}
    assert {b"a\n\n\n\nb", b"a\n\n\n\na"} <= literal
    assert behind >= {(d, e) for d in range(1, 9) for e in (True, False)}       # the header starts 1 .. 8 bytes before the end


def test_mixed_eol(oracle):
    names = []
    for name, data, exp in dc.cases("mixed_eol"):
        got = check_case(oracle, name, data, exp)
        names.append(name.split("/")[1])
        assert [i for i, r in enumerate(exp["records"]) if b"\r\n" in r] == exp["crlf_records"], name
        if name.endswith("lf_crlf_crcrlf"):
            assert [r.split(b"\n")[0] for r in exp["records"]] == [b"@id", b"@id\r", b"@id\r\r", b"@id\r\r"]
            assert [header_of(r) for r in exp["records"]] == [b"@id", b"@id", b"@id\r", b"@id\r"] and got.count(b"\r") == 1
        elif "one_crlf" in name:
            at, = exp["crlf_records"]
            assert len(exp["records"]) == 200 and at == (100 if "middle" in name else 199) and data.count(b"\r") == 4
            assert exp["kept"][at] == ("_dup" not in name) and (header_of(exp["records"][at]) in [header_of(r) for r in exp["records"][:at]]) == ("_dup" in name)
            # (the groups of 32 records around the CRLF one hold no '\r': they are still copied verbatim)
            assert all(b"\r" not in r for i, r in enumerate(exp["records"]) if i // dc.GROUP != at // dc.GROUP)
        else:
            assert data.endswith(b"@id\r") and header_of(exp["records"][5]) == b"@id" and exp["kept"][-1] and got.endswith(b"@id\r\n")
            assert (b"\r\n" in data) == name.endswith("_crlf_file")
    assert names == ["lf_crlf_crcrlf", "one_crlf_middle", "one_crlf_middle_dup", "one_crlf_last", "one_crlf_last_dup", "final_cr_no_lf",
                     "final_cr_no_lf_crlf_file"]


def test_groups(oracle):
    met = set()
    for name, data, exp in dc.cases("groups"):
        check_case(oracle, name, data, exp)
        count, kept, G = exp["count"], exp["kept"], dc.GROUP
        groups = [kept[g:g + G] for g in range(0, count, G)]
        assert len(kept) == count and kept[0], name
        pat = exp["pattern"]
        if pat == "none":
            assert all(kept), name
        elif pat.startswith("group"):
            g = int(pat[5:])
            assert 1 <= g < len(groups) and not any(groups[g]) and all(all(x) for k, x in enumerate(groups) if k != g), name
        elif pat == "first_of_group":
            assert all(x[0] and not any(x[1:]) for x in groups), name
        elif pat == "last_of_group":
            assert all(x[-1] and not any(x[1:-1]) and (k == 0 or len(x) == 1 or not x[0]) for k, x in enumerate(groups)), name
        else:
            assert pat == "alternating" and kept == [i % 2 == 0 for i in range(count)], name
        last = exp["records"][-1]
        assert len(nim_lines(last)) == exp["final_lines"] and last.endswith(b"\n") == exp["final_newline"], name
        assert (b"\r" in data) == (exp["eol"] == b"\r\n" and (count > 1 or exp["final_lines"] > 1 or exp["final_newline"])), name
        assert data.count(b"\r") in (0, data.count(b"\n")), name
        met.add((count, pat, exp["eol"], exp["final_lines"], exp["final_newline"]))
    assert {m[0] for m in met} == {1, 31, 32, 33, 63, 64, 65, 97}
    for count in (31, 32, 33, 63, 64, 65, 97):
        pats = {m[1] for m in met if m[0] == count}
        assert {"none", "first_of_group", "last_of_group", "alternating"} <= pats
        n_groups = (count + 31) // 32
        assert {p for p in pats if p.startswith("group")} == {"group%d" % g for g in {1, n_groups // 2, n_groups - 1} if 1 <= g < n_groups}
        for pat in pats:
            assert {m[2:] for m in met if m[:2] == (count, pat)} == {(e, l, nl) for e in (b"\n", b"\r\n") for l in (4, 3, 2, 1) for nl in (True, False)}


def test_copy_lengths(oracle):
    met = set()
    for name, data, exp in dc.cases("copy_lengths"):
        got = check_case(oracle, name, data, exp)
        assert b"\r" not in data and data.endswith(b"\n"), name
        if exp["body"] is None:
            r = exp["records"]
            assert got == r[0] + r[1], name
            assert exp["kept"] == [True, True, False] and len(nim_lines(r[0])[1]) == 100000, name
            assert dc.copy_geometry(0, len(r[0]))[1] > 448 * 8, name                          # many rounds of the 8-load loop
            continue
        assert got == data and all(exp["kept"]), name                                          # verbatim: groups are copied whole
        first, second = exp["records"][:dc.GROUP], exp["records"][dc.GROUP:]
        assert len(first) == dc.GROUP and 1 <= len(second) == exp["group_records"] <= dc.GROUP, name
        assert len(second) == dc.GROUP or exp["body"] < 32, name
        residue = sum(map(len, first)) % 16
        head, body, tail = dc.copy_geometry(residue, sum(map(len, second)))
        assert (residue, body, head) == (exp["residue"], exp["body"], (16 - residue) % 16), name
        met.add((body, residue, tail))
    assert {(b, r) for b, r, t in met} == {(b, r) for b in (0, 1, 63, 64, 65, 191, 192, 193, 255, 256, 257, 447, 448, 449, 511, 512, 513, 1025) for r in range(16)}
    assert {t for b, r, t in met} == set(range(16))


def test_saturated(oracle):
    """117 MB: the oracle once (through numpy buffers), the Python statement as well while it stays within seconds"""
    (name, data, exp), = dc.cases("saturated")
    headers = [r[:r.index(b"\n")] for r in exp["records"]]
    assert [len(h) for h in headers] == exp["lengths"] == [0xFFFFFE, 0xFFFFFF, 0x1000000] * 2 + [0x1000000]
    assert headers[:3] == headers[3:6] and len(set(headers[:3])) == 3
    a, b = headers[exp["sibling"][0]], headers[exp["sibling"][1]]
    assert a[:64] == b[:64] and a[64] != b[64] and a[65:] == b[65:]
    assert exp["kept"] == [True] * 3 + [False] * 3 + [True] and 100e6 < len(data) < 125e6
    want = b"".join(r for r, k in zip(exp["records"], exp["kept"]) if k)
    src = np.frombuffer(data, dtype=np.uint8)
    out = np.empty(src.size + 16, dtype=np.uint8)
    st = OracleDedupStats()
    n = oracle.lib.oracle_dedup(src.ctypes.data, src.size, out.ctypes.data, out.size, ctypes.byref(st))
    assert n == len(want) and out[:n].tobytes() == want
    assert (st.total_reads, st.duplicates, st.records_out, st.bytes_out) == (7, 3, 4, len(want))
    assert dedup_reference(data) == (want, 7, 3)            # (about a second: it works on whole lines)

"""The checker of fq-demux: a plain restatement of the contract in include/sc_fqcount.h, unit by unit and sample by sample (lines as
_readstats_check.py has them).  demux_of returns a dict: out1, out2 — bytes —, rows — a list of N + 1 dicts with the fields of
scfq_demux_row —, recs — a list of (sample, mm1, mm2, state) per unit — and every field of scfq_demux_stats but struct_size and
abi_version."""
from _readstats_check import lines_of

STATS_WORDS = 29
INTERLEAVED, HEADER, KEEP_BARCODE = 1, 2, 4
ASSIGNED, UNMATCHED, AMBIGUOUS, NO_BARCODE = 0, 1, 2, 3
DEFAULTS = dict(interleaved=False, header=False, keep_barcode=False, mismatches=1)
ROW_FIELDS = ("units", "perfect", "mismatched", "bases_out", "bytes1", "bytes2", "off1", "off2")
FIELDS = ("reads1", "reads2", "lines1", "lines2", "input_bytes1", "input_bytes2", "pairs", "unpaired", "units_in", "assigned", "undetermined",
          "no_barcode", "unmatched", "ambiguous", "perfect", "mismatched", "reads_in", "reads_out", "bases_in", "bases_out", "bases_clipped",
          "out1_bytes", "out2_bytes", "flags", "mismatches", "n_samples", "dual")
REPORT_HEADER = "sample\tbarcode\tunits\tpct_units\tperfect\tmismatched\tbases_out\tbytes1\tbytes2"


def _raw(x):
    return x.encode() if isinstance(x, str) else bytes(x)


def sheet_of(samples):
    """(name, barcode1, barcode2) triples of bytes, barcode2 = b"" on a single-index sheet"""
    return [(_raw(t[0]), _raw(t[1]), _raw(t[2]) if len(t) > 2 and t[2] is not None else b"") for t in samples]


def candidates(header_text):
    """X1, X2 of header mode"""
    if b":" not in header_text:
        return b"", b""
    tail = header_text[header_text.rindex(b":") + 1:]
    if b"+" not in tail:
        return tail, b""
    cut = tail.index(b"+")
    return tail[:cut], tail[cut + 1:]


def assign(x1, x2, sheet, M):
    """(sample, mm1, mm2, state) of one unit"""
    eligible, best, winners = False, None, []
    for s, (_, b1, b2) in enumerate(sheet):
        if len(x1) < len(b1) or len(x2) < len(b2):
            continue
        eligible = True
        mm1 = sum(1 for i in range(len(b1)) if x1[i] != b1[i])
        mm2 = sum(1 for i in range(len(b2)) if x2[i] != b2[i])
        if mm1 > M or mm2 > M:
            continue
        rank = (mm1 + mm2, -(len(b1) + len(b2)))
        if best is None or rank < best:
            best, winners = rank, [(s, mm1, mm2)]
        elif rank == best:
            winners.append((s, mm1, mm2))
    if not eligible:
        return (0xFFFF, 0xFF, 0xFF, NO_BARCODE)
    if not winners:
        return (0xFFFF, 0xFF, 0xFF, UNMATCHED)
    if len(winners) > 1:
        return (0xFFFF, 0xFF, 0xFF, AMBIGUOUS)
    return winners[0] + (ASSIGNED,)


def _record(lines, i):
    return [lines[4 * i + k] if 4 * i + k < len(lines) else b"" for k in range(4)]


def demux_of(data1, data2, samples, **kw):
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    p = dict(DEFAULTS, **kw)
    sheet = sheet_of(samples)
    N, dual, M = len(sheet), bool(sheet[0][2]), p["mismatches"]
    data1 = bytes(data1)
    data2 = bytes(data2) if data2 is not None else None
    lines1 = lines_of(data1)
    lines2 = lines_of(data2) if data2 is not None else []
    reads1, reads2 = (len(lines1) + 3) // 4, (len(lines2) + 3) // 4
    two, paired = data2 is not None, data2 is not None or p["interleaved"]
    assert not (two and p["interleaved"])
    assert not (dual and not paired and not p["header"]), "a dual sheet needs paired input in inline mode"
    if two:
        pairs, unpaired = min(reads1, reads2), max(reads1, reads2) - min(reads1, reads2)
        units = [(_record(lines1, u), _record(lines2, u)) for u in range(pairs)]
    elif p["interleaved"]:
        pairs, unpaired = reads1 // 2, reads1 % 2
        units = [(_record(lines1, 2 * u), _record(lines1, 2 * u + 1)) for u in range(pairs)]
    else:
        pairs, unpaired = 0, 0
        units = [(_record(lines1, u),) for u in range(reads1)]
    clip_on = not p["header"] and not p["keep_barcode"]
    recs, per_dest = [], [[] for _ in range(N + 1)]
    n = dict.fromkeys(("assigned", "undetermined", "no_barcode", "unmatched", "ambiguous", "perfect", "mismatched", "bases_in", "bases_out",
                       "bases_clipped"), 0)
    for unit in units:
        if p["header"]:
            x1, x2 = candidates(unit[0][0])
        else:
            x1, x2 = unit[0][1], (unit[1][1] if paired else b"")
        rec = assign(x1, x2, sheet, M)
        recs.append(rec)
        s, mm1, mm2, state = rec
        n[("assigned", "unmatched", "ambiguous", "no_barcode")[state]] += 1
        if state == ASSIGNED:
            n["perfect" if mm1 + mm2 == 0 else "mismatched"] += 1
        written, bases = [], 0
        for k, (h, S, sep, Q) in enumerate(unit):
            m = len(sheet[s][1 + k]) if state == ASSIGNED and clip_on else 0
            assert m <= len(S)
            written.append(h + b"\n" + S[m:] + b"\n" + sep + b"\n" + Q[min(len(Q), m):] + b"\n")
            n["bases_in"] += len(S)
            n["bases_clipped"] += m
            bases += len(S) - m
        n["bases_out"] += bases
        per_dest[s if state == ASSIGNED else N].append((written, bases, state == ASSIGNED and mm1 + mm2 == 0))
    n["undetermined"] = n["no_barcode"] + n["unmatched"] + n["ambiguous"]
    rows, out1, out2 = [], [], []
    for d in range(N + 1):
        row = dict.fromkeys(ROW_FIELDS, 0)
        row["off1"], row["off2"] = sum(len(x) for x in out1), sum(len(x) for x in out2)
        for written, bases, perfect in per_dest[d]:
            row["units"] += 1
            row["perfect"] += perfect
            row["mismatched"] += d < N and not perfect
            row["bases_out"] += bases
            if two:
                out1.append(written[0]); out2.append(written[1])
                row["bytes1"] += len(written[0]); row["bytes2"] += len(written[1])
            else:
                out1.append(b"".join(written))
                row["bytes1"] += len(out1[-1])
        rows.append(row)
    out = dict(n, out1=b"".join(out1), out2=b"".join(out2), rows=rows, recs=recs, reads1=reads1, reads2=reads2 if two else 0, lines1=len(lines1),
               lines2=len(lines2), input_bytes1=len(data1), input_bytes2=len(data2) if two else 0, pairs=pairs, unpaired=unpaired, units_in=len(units),
               reads_in=len(units) * (2 if paired else 1), reads_out=len(units) * (2 if paired else 1),
               flags=(INTERLEAVED if p["interleaved"] else 0) | (HEADER if p["header"] else 0) | (KEEP_BARCODE if p["keep_barcode"] else 0), mismatches=M,
               n_samples=N, dual=int(dual))
    out["out1_bytes"], out["out2_bytes"] = len(out["out1"]), len(out["out2"])
    check_identities(out, out["rows"])
    return out


def same(p, q):
    return set(p) == set(q) and all(p[k] == q[k] for k in p)


def check_identities(w, rows):
    assert w["units_in"] == w["assigned"] + w["undetermined"]
    assert w["undetermined"] == w["no_barcode"] + w["unmatched"] + w["ambiguous"]
    assert w["assigned"] == w["perfect"] + w["mismatched"]
    assert w["reads_in"] == w["reads_out"]
    assert w["bases_in"] == w["bases_out"] + w["bases_clipped"]
    assert len(rows) == w["n_samples"] + 1
    assert sum(r["units"] for r in rows) == w["units_in"] and rows[-1]["units"] == w["undetermined"]
    assert sum(r["perfect"] for r in rows) == w["perfect"] and sum(r["mismatched"] for r in rows) == w["mismatched"]
    assert rows[-1]["perfect"] == 0 and rows[-1]["mismatched"] == 0
    assert all(r["units"] == r["perfect"] + r["mismatched"] for r in rows[:-1])
    assert sum(r["bases_out"] for r in rows) == w["bases_out"]
    assert sum(r["bytes1"] for r in rows) == w["out1_bytes"] and sum(r["bytes2"] for r in rows) == w["out2_bytes"]
    assert rows[0]["off1"] == 0 and rows[0]["off2"] == 0
    for d in range(len(rows) - 1):
        assert rows[d + 1]["off1"] == rows[d]["off1"] + rows[d]["bytes1"] and rows[d + 1]["off2"] == rows[d]["off2"] + rows[d]["bytes2"]


def rows_of(rows):
    """a list of scfq.DemuxRow as the checker's dicts"""
    return [{name: int(getattr(r, name)) for name in ROW_FIELDS} for r in rows]


def recs_of(recs):
    """scfq.DemuxRec entries (a ctypes array, or an (n, 8) uint8 array) as the checker's tuples"""
    out = []
    for r in recs:
        if hasattr(r, "sample"):
            assert bytes(r.reserved) == b"\0\0\0"
            out.append((int(r.sample), int(r.mm1), int(r.mm2), int(r.state)))
        else:
            b = bytes(bytearray(int(x) for x in r))
            assert len(b) == 8 and b[5:] == b"\0\0\0"
            out.append((b[0] | b[1] << 8, b[2], b[3], b[4]))
    return out


def assert_stats(s, rows, want, ctx=""):
    """s: a scfq.DemuxStats; rows: its DemuxRow list; want: the checker's dict; every field compared with =="""
    assert int(s.struct_size) == 8 * STATS_WORDS and int(s.abi_version) > 0, ctx
    for name in FIELDS:
        assert int(getattr(s, name)) == want[name], (ctx, name, int(getattr(s, name)), want[name])
    got = rows_of(rows)
    assert got == want["rows"], (ctx, [(d, g, w) for d, (g, w) in enumerate(zip(got, want["rows"])) if g != w][:3])
    check_identities({name: int(getattr(s, name)) for name in FIELDS}, got)


def report_text(w, samples):
    """the rows of scfq_format_demux_row_tsv for a checker's dict, one line each"""
    sheet = sheet_of(samples)
    lines = []
    for d, r in enumerate(w["rows"]):
        und = d == len(sheet)
        name = "undetermined" if und else sheet[d][0].decode()
        bc = "-" if und else (sheet[d][1] + (b"+" + sheet[d][2] if sheet[d][2] else b"")).decode()
        pct = 10000 * r["units"] // w["units_in"] if w["units_in"] else 0
        lines.append("\t".join([name, bc, str(r["units"]), "%d.%02d" % (pct // 100, pct % 100)] +
                               [str(r[k]) for k in ("perfect", "mismatched", "bases_out", "bytes1", "bytes2")]))
    return lines

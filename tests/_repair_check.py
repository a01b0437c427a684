"""fq-repair restated in plain Python (include/sc_fqcount.h has the definition): a dictionary from a name to two lists of record indices,
zipped.  Nothing of the device's hash is in here, so `collisions` and `rounds` are not restated, and `path` only where the definition
fixes it.  repair_of is what every test compares with ==; mates_by_pairs states the matching rule once more by comparing all pairs."""
from _readstats_check import lines_of

STATS_WORDS = 24
SINGLE = 0xFFFFFFFF
OUTPUTS = ("out1", "out2", "singles1", "singles2")
FIELDS = ("reads1", "reads2", "lines1", "lines2", "input_bytes1", "input_bytes2", "pairs", "singles1", "singles2", "moved", "in_step", "repeated1",
          "repeated2", "out1_bytes", "out2_bytes", "singles1_bytes", "singles2_bytes", "flags")
HASH_FIELDS = ("collisions", "rounds", "path", "hash_bits")      # not restated
REPORT_FIELDS = ("reads1", "reads2", "pairs", "singles1", "singles2", "moved", "in_step", "repeated1", "repeated2", "out1_bytes", "out2_bytes",
                 "singles1_bytes", "singles2_bytes")
STATS_HEADER = "\t".join(REPORT_FIELDS)
REC_HEADER = "input\trecord\tmate"


def name_of(header):
    """the name of a record from the text of its header line"""
    name = bytes(header)[1:]                            # the first byte goes, whatever it is
    cut = [k for k in (name.find(b" "), name.find(b"\t")) if k >= 0]
    if cut:
        name = name[:min(cut)]
    if len(name) >= 2 and name[-2:] in (b"/1", b"/2"):
        name = name[:-2]
    return name


def mates_of(names1, names2):
    """the table: per record of R1 its mate's index in R2 or SINGLE, then the same for R2's records"""
    where = {}
    for i, n in enumerate(names1):
        where.setdefault(n, ([], []))[0].append(i)
    for j, n in enumerate(names2):
        where.setdefault(n, ([], []))[1].append(j)
    t1, t2 = [SINGLE] * len(names1), [SINGLE] * len(names2)
    for first, second in where.values():
        for i, j in zip(first, second):
            t1[i], t2[j] = j, i
    return t1 + t2


def mates_by_pairs(names1, names2):
    """the same table from the matching rule alone: record i of R1, the r-th in R1 with its name, is the mate of record j of R2 iff the
    names are equal and j is the r-th in R2 with it"""
    rank1 = [sum(1 for v in range(i) if names1[v] == n) for i, n in enumerate(names1)]
    rank2 = [sum(1 for v in range(j) if names2[v] == n) for j, n in enumerate(names2)]
    t1, t2 = [SINGLE] * len(names1), [SINGLE] * len(names2)
    for i, n in enumerate(names1):
        for j, m in enumerate(names2):
            if n == m and rank1[i] == rank2[j]:
                assert t1[i] == SINGLE and t2[j] == SINGLE
                t1[i], t2[j] = j, i
    return t1 + t2


def _echo(lines, i):
    return b"".join(t + b"\n" for t in lines[4 * i:4 * i + 4])


def _repeated(names):
    return len(names) - len(set(names))


def repair_of(data1, data2):
    l1, l2 = lines_of(bytes(data1)), lines_of(bytes(data2))
    r1, r2 = (len(l1) + 3) // 4, (len(l2) + 3) // 4
    names1, names2 = [name_of(l1[4 * i]) for i in range(r1)], [name_of(l2[4 * j]) for j in range(r2)]
    table = mates_of(names1, names2)
    out1 = b"".join(_echo(l1, i) for i in range(r1) if table[i] != SINGLE)
    out2 = b"".join(_echo(l2, table[i]) for i in range(r1) if table[i] != SINGLE)
    singles1 = b"".join(_echo(l1, i) for i in range(r1) if table[i] == SINGLE)
    singles2 = b"".join(_echo(l2, j) for j in range(r2) if table[r1 + j] == SINGLE)
    pairs = sum(1 for i in range(r1) if table[i] != SINGLE)
    moved = sum(1 for i in range(r1) if table[i] not in (SINGLE, i))
    out = dict(reads1=r1, reads2=r2, lines1=len(l1), lines2=len(l2), input_bytes1=len(data1), input_bytes2=len(data2), pairs=pairs, singles1=r1 - pairs,
               singles2=r2 - pairs, moved=moved, in_step=int(r1 == r2 and pairs == r1 and moved == 0), repeated1=_repeated(names1),
               repeated2=_repeated(names2), table=table, names1=names1, names2=names2, out1=out1, out2=out2, singles1_out=singles1, singles2_out=singles2,
               out1_bytes=len(out1), out2_bytes=len(out2), singles1_bytes=len(singles1), singles2_bytes=len(singles2), flags=0)
    out["outs"] = [out1, out2, singles1, singles2]
    check_identities(out)
    return out


def check_identities(w, table=None):
    assert w["pairs"] + w["singles1"] == w["reads1"] and w["pairs"] + w["singles2"] == w["reads2"] and w["moved"] <= w["pairs"]
    assert w["in_step"] == int(w["reads1"] == w["reads2"] and w["singles1"] == 0 and w["singles2"] == 0 and w["moved"] == 0)
    assert w["repeated1"] <= max(w["reads1"] - 1, 0) and w["repeated2"] <= max(w["reads2"] - 1, 0)
    assert w["out1_bytes"] + w["singles1_bytes"] >= w["reads1"] and w["out2_bytes"] + w["singles2_bytes"] >= w["reads2"]
    table = w.get("table") if table is None else table
    if table is not None:
        r1 = w["reads1"]
        assert len(table) == r1 + w["reads2"]
        for i in range(r1):
            assert table[i] == SINGLE or table[r1 + table[i]] == i
        for j in range(w["reads2"]):
            assert table[r1 + j] == SINGLE or table[table[r1 + j]] == j


def assert_stats(s, want, ctx="", path=None):
    """s: a scfq.RepairStats; want: a checker's dict; every field but the hash's compared with ==.  path: what `path` has to be, when the
    case fixes it"""
    assert int(s.struct_size) == 8 * STATS_WORDS and int(s.abi_version) > 0, ctx
    for name in FIELDS:
        assert int(getattr(s, name)) == want[name], (ctx, name, int(getattr(s, name)), want[name])
    check_identities({name: int(getattr(s, name)) for name in FIELDS})
    assert int(s.path) in (0, 1) and (path is None or int(s.path) == path), (ctx, int(s.path), path)
    if int(s.path) == 0:
        assert want["in_step"] == 1, ctx


def stats_text(w):
    """the row of scfq_format_repair_stats_tsv for a checker's dict"""
    return "\t".join(str(w[k]) for k in REPORT_FIELDS)


def rec_text(which, record, mate):
    """the row of scfq_format_repair_rec_tsv"""
    return "%d\t%d\t%s" % (which, record, "-" if mate == SINGLE else "%d" % mate)


def per_read_text(w, header=False):
    rows = [REC_HEADER] if header else []
    r1 = w["reads1"]
    rows += [rec_text(1 if u < r1 else 2, u if u < r1 else u - r1, m) for u, m in enumerate(w["table"])]
    return "".join(r + "\n" for r in rows)

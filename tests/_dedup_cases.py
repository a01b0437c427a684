"""Inputs for the edges of fq-dedup (seq-collection_amd/csrc/scfq_dedup.hip), built where its kernels change path: the compare
behind the hash past byte 64, headers that differ in their length alone, the first and last bytes of the input, mixed line ends,
the gather's groups of 32 records, the thresholds of its wave-wide copy, and headers longer than the packed length holds.

Every generator yields (name, bytes, expectations), is deterministic and needs numpy at most.  expectations always holds
  records     the input cut into its records (a record starts at every fourth line), as bytes
  kept        for each record, whether fq-dedup echoes it
  duplicates  the number of dropped records
and what the family exists for (tests/test_dedup_cases_host.py asserts each from the bytes before a device sees them).

`python tests/_dedup_cases.py --run FAMILY` runs a family through the library in this process, with whatever SCFQ_DEDUP_* the
environment holds (they are read once per process), compares bytes and statistics with the oracle and prints one JSON line.
"""
import json
import os
import sys
import time

FAMILIES = ("tail_compare", "length_only", "input_ends", "mixed_eol", "groups", "copy_lengths", "saturated")
GROUP = 32               # records per group of dd_gather
SATURATED = 0xFFFFFF     # the largest header length dd_hash_headers packs beside the start


def _seq(k):
    return bytes(b"ACGT"[(k + 3 * j) & 3] for j in range(k))


def _qual(k):
    return bytes(35 + (k + 5 * j) % 40 for j in range(k))


def _rec(hdr, k, eol=b"\n"):
    """a whole record with a read of k bases"""
    return hdr + eol + _seq(k) + eol + b"+" + eol + _qual(k) + eol


def _filler(k, salt=0):
    """k lowercase bytes, no two neighbours equal"""
    return bytes(97 + (salt + 7 * j + j // 26) % 26 for j in range(k))


def _first_occurrence(headers):
    seen, kept = set(), []
    for h in headers:
        kept.append(h not in seen)
        seen.add(h)
    return kept


def _exp(records, kept, **more):
    return dict(records=records, kept=kept, duplicates=kept.count(False), **more)


# ---------------------------------------------------------------------------------------------------------------- a. tail_compare
TAIL_L = (64, 65, 66, 71, 72, 73, 127, 128, 129, 255, 256, 257, 300)
_VARIANT_BYTES = bytes(range(0x21, 0x60))      # 63 values, none lowercase (the base header is '@' + lowercase), none an EOL


def tail_positions(L):
    return sorted({p for p in (64, 65, L - 2, L - 1) if 64 <= p < L})


def tail_compare():
    """Headers of L bytes that share their first 64 bytes and differ from the base header in ONE byte, at p in {64, 65, L-2, L-1}
    (many values per p: two variants of one p differ at p alone); one exact duplicate of the base and of a variant of every p;
    records that differ from the base at byte 63 alone (one, or all variants where L == 64 leaves no p).  The hashes of 40-60
    headers truncated to 4 bits must collide: then only the byte walk behind the eight masked words tells the variants apart."""
    for L in TAIL_L:
        base = b"@" + _filler(L - 1, L)
        ps = tail_positions(L)
        n_var = 44 // len(ps) if ps else 0
        headers, diff_at, dup_of = [base], [None], [None]
        for v in range(n_var):
            for p in ps:
                headers.append(base[:p] + _VARIANT_BYTES[v:v + 1] + base[p + 1:])
                diff_at.append(p)
                dup_of.append(None)
        for v in range(1 if ps else 44):
            headers.append(base[:63] + _VARIANT_BYTES[v:v + 1] + base[64:])
            diff_at.append(63)
            dup_of.append(None)
        n_first = len(headers)
        for src in [0] + [1 + j for j in range(len(ps))]:      # the base, and the first variant of every p
            headers.append(headers[src])
            diff_at.append(diff_at[src])
            dup_of.append(src)
        kept = [d is None for d in dup_of]
        records = [_rec(h, 1 + (7 * i + L) % 40) for i, h in enumerate(headers)]
        yield "tail_compare/L=%d" % L, b"".join(records), _exp(records, kept, L=L, positions=ps, diff_at=diff_at, dup_of=dup_of,
                                                              n_first=n_first)


# ----------------------------------------------------------------------------------------------------------------- b. length_only
def length_only():
    """Headers whose eight masked words agree and whose length alone differs (a header and the same header with NUL bytes
    behind it), the same with other bytes behind it (the words differ), an empty header line twice, and every header a second
    time: each pair (i, j, 'nul' | 'text') must be told apart, each copy must be dropped."""
    headers, pairs = [], []

    def family(stem, extra, kind, n_max):
        idx = []
        for k in range(n_max + 1):
            h = stem + extra * k
            if h in headers:
                idx.append(headers.index(h))
            else:
                headers.append(h)
                idx.append(len(headers) - 1)
        pairs.extend((idx[a], idx[b], kind) for a in range(len(idx)) for b in range(a + 1, len(idx)))

    for c in b"abcdefgh":                       # @a, @a\0, @a\0\0 (and up to five, and eight stems: 4-bit hashes of some pair collide)
        family(b"@" + bytes([c]), b"\0", "nul", 5)
    for n in (7, 15, 63):                       # 7/8/9, 15/16/17, 63/64/65: the shorter a prefix, the rest NUL
        family(b"@" + _filler(n - 1, n), b"\0", "nul", 2)
    for c in b"ab":
        family(b"@" + bytes([c]), b"x", "text", 2)
    for n in (7, 15, 63):
        family(b"@" + _filler(n - 1, n), b"x", "text", 2)
    headers.append(b"")
    n_first = len(headers)
    headers = headers + headers                 # every header again, the empty one included
    kept = [i < n_first for i in range(len(headers))]
    records = [_rec(h, 1 + (3 * i) % 40) for i, h in enumerate(headers)]
    yield "length_only/all", b"".join(records), _exp(records, kept, pairs=pairs, n_first=n_first, empty_at=(n_first - 1, 2 * n_first - 1))


# ------------------------------------------------------------------------------------------------------------------ c. input_ends
_TERMINATORS = (("none", b""), ("lf", b"\n"), ("cr", b"\r"), ("crlf", b"\r\n"))
_LOWER = b"abcdefghijklmnopq"      # the header of m bytes the last one repeats: abc...
_UPPER = b"ABCDEFGHIJKLMNOPQ"      # headers of the records that only fill


def _minimal(h):
    return h + b"\n\n\n\n"


def _last_header(m, equal):
    h = _LOWER[:m]
    return h if equal else h[:-1] + bytes([h[-1] + 1])


def _end_case(prefix_records, m, equal, tname, term, name):
    last = _last_header(m, equal) + term
    records = prefix_records + [last]
    # (a final "\r" without "\n" stays part of the header: fq_dedup.nim reads lines as Nim's readLine does)
    final = _last_header(m, equal) + (b"\r" if tname == "cr" else b"")
    kept = _first_occurrence([r.split(b"\n")[0] for r in prefix_records] + [final])      # (the records before it are LF only)
    return name, b"".join(records), _exp(records, kept, m=m, equal=equal, terminator=tname, final_header=final)


def input_ends():
    """Every total size n = 1 .. 40 of `minimal records + last header`: the records are h\\n\\n\\n\\n with headers of 1 .. 17 bytes, the
    last header (m bytes: every m up to n = 16, then 1, 2, 7, 8, 9, 16, 17) repeats an earlier header or differs from it in its last
    byte, and nothing, \\n, \\r or \\r\\n follows it.  Then the same tails behind 5 000 bytes of ordinary records, with the last header
    starting 1 .. 9 bytes before the end of the input."""
    for n in range(1, 41):
        for tname, term in _TERMINATORS:
            for m in (range(1, 18) if n <= 16 else (1, 2, 7, 8, 9, 16, 17)):
                rest = n - m - len(term)
                if rest == 0:                   # the header alone
                    yield _end_case([], m, True, tname, term, "input_ends/n=%d,m=%d,%s,alone" % (n, m, tname))
                    continue
                rest -= m + 4                   # the record whose header the last one repeats
                if rest < 0 or 0 < rest < 5:
                    continue
                fill = []
                while rest:
                    k = min(rest, 21) if rest - min(rest, 21) not in range(1, 5) else rest - 5
                    fill.append(_minimal(_UPPER[:k - 4]))
                    rest -= k
                # (the repeated header directly before the last one for odd n, the fillers between them for even n)
                prefix = fill + [_minimal(_LOWER[:m])] if n & 1 else [_minimal(_LOWER[:m])] + fill
                for equal in (True, False):
                    yield _end_case(list(prefix), m, equal, tname, term,
                                    "input_ends/n=%d,m=%d,%s,%s" % (n, m, tname, "equal" if equal else "differs"))
    ordinary = [_rec(b"@r%d/%s" % (i, _filler(20 + i % 30, i)), 30 + i % 40) for i in range(60)]
    for m in range(1, 10):
        body = ordinary[:20] + [_rec(_LOWER[:m], 25)] + ordinary[20:]
        size = 0
        prefix = []
        for r in body:                          # about 5 000 bytes, the repeated header among them
            if size >= 5000:
                break
            prefix.append(r)
            size += len(r)
        for tname, term in _TERMINATORS:
            for equal in (True, False):
                yield _end_case(list(prefix), m, equal, tname, term,
                                "input_ends/behind5000,m=%d,%s,%s" % (m, tname, "equal" if equal else "differs"))


# ------------------------------------------------------------------------------------------------------------------- d. mixed_eol
def _lf_file(n, salt):
    return [_rec(b"@m%d.%d %s" % (salt, i, _filler(10 + i % 20, i)), 20 + (11 * i) % 40) for i in range(n)]


def mixed_eol():
    """LF and CRLF records in one file.  One "\\r\\n" anywhere tells every kernel to look behind the newlines, while the groups without
    a '\\r' are still copied verbatim; an ID is the same ID whichever of the two ends its line, and only one '\\r' is stripped."""
    recs = [_rec(b"@id", 10), _rec(b"@id", 12, b"\r\n"), b"@id\r\r\n" + _rec(b"", 9)[1:], _rec(b"@id\r", 7, b"\r\n")]
    yield "mixed_eol/lf_crlf_crcrlf", b"".join(recs), _exp(recs, [True, False, True, False], crlf_records=[1, 2, 3])
    for where in ("middle", "last"):
        for dup in (False, True):
            recs = _lf_file(200, 1 + dup)
            at = 100 if where == "middle" else 199
            hdr = recs[37].split(b"\n")[0] if dup else recs[at].split(b"\n")[0]
            recs[at] = _rec(hdr, 33, b"\r\n")
            kept = [not (dup and i == at) for i in range(200)]
            yield "mixed_eol/one_crlf_%s%s" % (where, "_dup" if dup else ""), b"".join(recs), _exp(recs, kept, crlf_records=[at])
    for crlf_elsewhere in (False, True):        # a final header "@id\r" without '\n' keeps its '\r': not the ID "@id"
        recs = _lf_file(40, 3)
        recs[5] = _rec(b"@id", 21, b"\r\n" if crlf_elsewhere else b"\n")
        recs.append(b"@id\r")
        yield "mixed_eol/final_cr_no_lf%s" % ("_crlf_file" if crlf_elsewhere else ""), b"".join(recs), \
            _exp(recs, [True] * 41, crlf_records=[5] if crlf_elsewhere else [])


# ---------------------------------------------------------------------------------------------------------------------- e. groups
GROUP_COUNTS = (1, 31, 32, 33, 63, 64, 65, 97)
FINAL_SHAPES = [(lines, newline) for lines in (4, 3, 2, 1) for newline in (True, False)]


def group_patterns(count):
    """name -> the records dropped.  Record 0 opens the file and is always kept; a group is dropped whole where an earlier group
    exists (g: the first such group, the middle one, the last one — its neighbours stay whole)."""
    n_groups = (count + GROUP - 1) // GROUP
    pats = {"none": set()}
    if count == 1:
        return pats
    for g in sorted({1, n_groups // 2, n_groups - 1} - {0}):
        if g < n_groups:
            pats["group%d" % g] = set(range(g * GROUP, min(count, (g + 1) * GROUP)))
    pats["first_of_group"] = {i for i in range(count) if i % GROUP}
    pats["last_of_group"] = {i for i in range(1, count) if i % GROUP != GROUP - 1 and i != count - 1}
    pats["alternating"] = set(range(1, count, 2))
    return pats


def groups():
    """Record counts around one, two and three groups of 32, with the dropped records placed by pattern; the final record with
    4, 3, 2 or 1 lines, with and without a final newline; everything in LF and in CRLF."""
    for count in GROUP_COUNTS:
        for pname, dropped in group_patterns(count).items():
            for eol_name, eol in (("lf", b"\n"), ("crlf", b"\r\n")):
                for lines, newline in FINAL_SHAPES:
                    headers, kept_idx = [], []
                    for i in range(count):
                        if i in dropped:
                            headers.append(headers[kept_idx[(7 * i) % len(kept_idx)]])
                        else:
                            headers.append(b"@g%d:%s" % (i, _filler(5 + i % 9, i)))
                            kept_idx.append(i)
                    records = [_rec(h, 1 + (5 * i) % 40, eol) for i, h in enumerate(headers)]
                    last = records[-1].split(eol)[:lines]
                    records[-1] = eol.join(last) + (eol if newline else b"")
                    kept = [i not in dropped for i in range(count)]
                    yield "groups/n=%d,%s,%s,last=%dlines%s" % (count, pname, eol_name, lines, "" if newline else ",no_newline"), \
                        b"".join(records), _exp(records, kept, count=count, pattern=pname, dropped=sorted(dropped), eol=eol,
                                                final_lines=lines, final_newline=newline)


# ---------------------------------------------------------------------------------------------------------------- f. copy_lengths
COPY_BODIES = (0, 1, 63, 64, 65, 191, 192, 193, 255, 256, 257, 447, 448, 449, 511, 512, 513, 1025)


def _fit(tag, count, total):
    """count records with distinct headers, total bytes exactly: one read padded (two bytes a base, a header byte for an odd rest)"""
    recs = [_rec(b"@%s%d" % (tag, i), 1) for i in range(count)]
    rest = total - sum(map(len, recs))
    if rest < 0:
        return None
    recs[count // 2] = _rec(b"@%s%d" % (tag, count // 2) + b"_" * (rest & 1), 1 + rest // 2)
    assert sum(map(len, recs)) == total
    return recs


def copy_geometry(dst_residue, length):
    """(head bytes, body chunks, tail bytes) of wave_copy for a destination at dst_residue mod 16"""
    head = min((16 - dst_residue) & 15, length)
    return head, (length - head) // 16, (length - head) % 16


def copy_lengths():
    """wave_copy's paths: its head bytes 0 .. 15, its body through the 8-load loop (more than 448 chunks of 16 bytes), the 4-load
    step (more than 192), the last steps, and its tail.  Group 0 (32 records, kept) ends at every residue mod 16; group 1 behind
    it is kept verbatim and is as long as gives the copy the named body, at that destination, in a 16-byte aligned output
    (32 records, or as many as fit into the short ones: group 1 is the file's last).  Then one record of 100 000 bases in a
    group that also drops a record: copied on its own, through the 8-load loop."""
    for body in COPY_BODIES:
        for residue in range(16):
            first = _fit(b"p", GROUP, 32 * 12 + 16 + residue)
            head = (16 - residue) & 15
            length = head + 16 * body + (11 if body == 0 else (7 * body + 3 * residue) % 16)
            count = GROUP
            while (second := _fit(b"q", count, length)) is None:
                count -= 1
            records = first + second
            yield "copy_lengths/body=%d,residue=%d" % (body, residue), b"".join(records), \
                _exp(records, [True] * len(records), body=body, residue=residue, group_records=count)
    big = [_rec(b"@big", 100000), _rec(b"@small", 10), _rec(b"@big", 5)]
    yield "copy_lengths/one_record_100000_bases", b"".join(big), _exp(big, [True, True, False], body=None, residue=0, group_records=3)


# ------------------------------------------------------------------------------------------------------------------- g. saturated
def saturated(with_sibling=True):
    """Headers of 0xFFFFFE, 0xFFFFFF and 0x1000000 bytes: the last two do not fit the 24 bits beside the packed start and are
    looked up again through the line index.  Each is met twice; one more header of 0x1000000 bytes differs from its sibling at
    byte 64 alone.  About 117 MB: a family of its own."""
    block = _filler(4096, 1)
    headers = []
    for tag, L in ((b"@A", SATURATED - 1), (b"@B", SATURATED), (b"@C", SATURATED + 1)):
        headers.append((tag + block * (L // 4096 + 1))[:L])
    order = [0, 1, 2, 0, 1, 2]
    if with_sibling:
        h = headers[2]
        headers.append(h[:64] + b"#" + h[65:])
        order.append(3)
    records = [_rec(headers[k], 5 + i) for i, k in enumerate(order)]
    kept = [True, True, True, False, False, False] + [True] * with_sibling
    yield "saturated/three_lengths_twice" + ("_and_sibling" if with_sibling else ""), b"".join(records), \
        _exp(records, kept, lengths=[len(headers[k]) for k in order], sibling=(2, 6) if with_sibling else None)


def cases(family):
    assert family in FAMILIES, family
    return globals()[family]()


# ---------------------------------------------------------------------------------------------------------------- the child process
def oracle_dedup(oracle, a):
    """oracle.dedup through numpy buffers: (bytes, statistics) of inputs of any size"""
    import ctypes
    import numpy as np
    import conftest
    out = np.empty(a.size + 16, dtype=np.uint8)
    st = conftest.OracleDedupStats()
    n = oracle.lib.oracle_dedup(a.ctypes.data, a.size, out.ctypes.data, out.size, ctypes.byref(st))
    assert n >= 0, n
    return out[:n].tobytes(), st


def library_dedup(scfq, a):
    """scfq.dedup_host through numpy buffers: the sizing call, then the result into host memory"""
    import ctypes
    import numpy as np
    st, nb = scfq.DedupStats(), ctypes.c_uint64()
    st.struct_size = ctypes.sizeof(st)
    rc = scfq.lib().scfq_dedup_buffer(a.ctypes.data, a.size, 0, None, 0, 0, ctypes.byref(nb), ctypes.byref(st))
    assert rc == 0, rc
    out = np.empty(max(nb.value, 1), dtype=np.uint8)
    st = scfq.DedupStats()
    st.struct_size = ctypes.sizeof(st)
    rc = scfq.lib().scfq_dedup_buffer(a.ctypes.data, a.size, 0, out.ctypes.data, nb.value, 0, ctypes.byref(nb), ctypes.byref(st))
    assert rc == 0, rc
    return out[:nb.value].tobytes(), st


def run_family(family):
    import numpy as np
    import conftest
    import scfq
    oracle = conftest._oracle_for_subprocess()
    big = family == "saturated"
    scfq.lib()
    if big:                     # (its time is the device's: the library is loaded and has met the device before the clock starts)
        scfq.dedup_host(b"@a\nA\n+\nI\n")
    t0 = time.perf_counter()
    n_cases, collisions = 0, []
    for name, data, exp in cases(family):
        a = np.frombuffer(data, dtype=np.uint8)
        want, ost = oracle_dedup(oracle, a) if big else oracle.dedup(a)
        t0 = time.perf_counter() if big else t0
        got, st = library_dedup(scfq, a) if big else scfq.dedup_host(a)
        stats = (st.total_reads, st.duplicates, st.records_out, st.bytes_out)
        wstats = (ost.total_reads, ost.duplicates, ost.records_out, ost.bytes_out)
        if stats != wstats or got != want:
            k = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
            print("MISMATCH %s: statistics %r, oracle %r; %d bytes, oracle %d, first difference at byte %d; input %r"
                  % (name, stats, wstats, len(got), len(want), k, data[:64]))
            return 1
        assert st.duplicates == exp["duplicates"], (name, st.duplicates, exp["duplicates"])
        collisions.append(st.hash_collisions)
        n_cases += 1
    print(json.dumps(dict(family=family, cases=n_cases, min_hash_collisions=min(collisions), seconds=round(time.perf_counter() - t0, 3),
                          hash_bits=os.environ.get("SCFQ_DEDUP_HASH_BITS"), fused=os.environ.get("SCFQ_DEDUP_FUSED_HASH"))))
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--run":
        sys.exit(run_family(sys.argv[2]))
    sys.exit("usage: _dedup_cases.py --run FAMILY")

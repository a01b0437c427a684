"""Helper run in a subprocess by test_gpu_scan_taper.py with SCFQ_TILES_PER_RANGE=8 SCFQ_TAPER_WAVES=4 in the environment, so that inputs of
a few hundred tiles are scanned under a tapered geometry (8 / 4 / 2 tiles per range): every word of the partial against the oracle.
Prints one "ok <group>" line per group of cases; the parent asserts on them."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "seq-collection_amd", "pyhost"))
import torch
import scfq

assert os.environ.get("SCFQ_TILES_PER_RANGE") == "8" and os.environ.get("SCFQ_TAPER_WAVES") == "4"
TILE = 4096
O = ctypes.CDLL(os.path.join(ROOT, "oracle", "libfqcount_oracle.so"))
O.oracle_partial.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p]
scfq.set_wait_stream(torch.cuda.current_stream().cuda_stream)
rng = np.random.default_rng(20261019)
MAX_N = 1023 * TILE + 4095


def oracle_partial(a, prev, want_hist=False):
    w = (ctypes.c_uint64 * 27)()
    h = (ctypes.c_uint64 * 1024)() if want_hist else None
    O.oracle_partial(a.ctypes.data if a.size else None, a.size, prev, w, ctypes.byref(h) if want_hist else None)
    return ([int(x) for x in w], [int(x) for x in h]) if want_hist else [int(x) for x in w]


def records(n, read_len, eol):
    """FASTQ records of one read length (header, sequence, '+', quality), cut at n bytes"""
    seqs = rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), n, p=[0.27, 0.22, 0.23, 0.27, 0.01]).tobytes()
    quals = rng.choice(np.frombuffer(b"#,:F", dtype=np.uint8), n).tobytes()
    out, size, k = [], 0, 0
    while size < n:
        at = (k * read_len) % (n - read_len)
        rec = b"@SIM:1:FC%06d:1:1101:%d:%d 1:N:0:ACGT" % (k, 1000 + k % 977, 2000 + k % 991) + eol + seqs[at:at + read_len] + eol + b"+" + eol + \
            quals[at:at + read_len] + eol
        out.append(rec)
        size += len(rec)
        k += 1
    return np.frombuffer(b"".join(out)[:n], dtype=np.uint8).copy()


CORPORA = {
    "illumina": records(MAX_N, 150, b"\n"),
    "crlf": records(MAX_N, 150, b"\r\n"),
    "long": records(MAX_N, 23_000, b"\n"),       # most tiles hold no newline at all
    "blank": rng.choice(np.frombuffer(b"\n\n\n\nG\r", dtype=np.uint8), MAX_N).astype(np.uint8),
}


def to_dev(arr, offset):
    """device copy of arr placed `offset` bytes past a 4 KiB boundary, guard bytes ('G') around it"""
    pad = 8192
    t = torch.full((pad + offset + arr.size + pad,), 0x47, dtype=torch.uint8, device="cuda")
    start = ((t.data_ptr() + pad + 4095) // 4096) * 4096 - t.data_ptr() + offset
    t[start:start + arr.size] = torch.from_numpy(arr)
    return t, t.data_ptr() + start


def sizes_string(g):
    return "/".join(str(s[2]) for s in g.segments())


def check(a, offset, prev, flags, ctx, min_segments):
    g = scfq.debug_scan_geometry(a.size, offset, flags)
    assert g.n_segments >= min_segments, (ctx, g.segments())
    t, ptr = to_dev(a, offset)
    want = oracle_partial(a, prev)
    p = scfq.partial_device(ptr, a.size, prev, flags=flags)
    ran = scfq.debug_last_scan_kernel()
    assert ran.endswith(" tiles_per_range=" + sizes_string(g)), (ctx, ran, g.segments())
    want25 = want[:25] if flags & scfq.SCFQ_STRUCT_CHECK else want[:13] + [0] * 12
    assert p.words()[:25] == want25, (ctx, g.segments())
    assert p.bytes == a.size and p.last_byte == int(a[-1]), ctx
    return g


# ---- every corpus at 1, 9, 300 and 1 023 tiles plus stray bytes, at pointer offsets 0, 1 and 4 095, flags 0 and STRUCT_CHECK ----
strays = iter([1, 4095, 2048, 63, 4033, 17, 1000, 3071, 64, 65, 4094, 2])
for tiles in (1, 9, 300, 1023):
    for offset in (0, 1, 4095):
        n = tiles * TILE + next(strays)
        for name, corpus in CORPORA.items():
            for flags in (0, scfq.SCFQ_STRUCT_CHECK):
                prev = (-1, 10, 13, 65)[(tiles + offset + flags) % 4]
                check(corpus[:n], offset, prev, flags, (name, tiles, offset, flags), 3 if tiles >= 300 else 1)
    print("ok tiles %d" % tiles)

# ---- a "\r\n" and a record boundary exactly on every segment boundary; the last byte in the smallest segment's edge tile ----
for offset in (0, 1, 4095):
    n = 299 * TILE + 1234
    g = scfq.debug_scan_geometry(n, offset, 0)
    assert g.n_segments >= 3 and g.n_tiles * TILE > offset + n, g.segments()     # the last tile is an edge tile
    cuts = [s[1] * TILE - offset for s in g.segments()[1:]]                       # data offsets of the segments' first bytes
    for split in (False, True):
        a = CORPORA["crlf"][:n].copy()
        for c in cuts:
            a[c - 160:c + 160] = ord("A")
            if split:      # '\r' is the last byte of one segment, '\n' the first byte of the next: the record starts one byte in
                a[c - 1], a[c], a[c + 1] = 13, 10, ord("@")
            else:          # "\r\n" ends the segment, the next record starts the next one
                a[c - 2], a[c - 1], a[c] = 13, 10, ord("@")
        for flags in (0, scfq.SCFQ_STRUCT_CHECK):
            check(a, offset, -1, flags, ("cuts", offset, split, flags), 3)
print("ok segment boundaries")

# ---- one chunked session: three chunks with carried state, each of them tapered ----
chunk = 300 * TILE
a = np.concatenate([CORPORA["crlf"][:chunk + 1], CORPORA["illumina"][:2 * chunk - 778]])      # (a "\r\n" split by the first cut or not: the corpus decides)
assert scfq.debug_scan_geometry(chunk, 0, 0).n_segments >= 3 and scfq.debug_scan_geometry(a.size - 2 * chunk, 0, 0).n_segments >= 3
for flags in (0, scfq.SCFQ_STRUCT_CHECK):
    want = oracle_partial(a, -1)
    p = scfq.partial_host(a, -1, flags=flags, chunk_bytes=chunk)
    assert scfq.debug_last_scan_kernel().endswith(" tiles_per_range=8/4/2"), scfq.debug_last_scan_kernel()
    want25 = want[:25] if flags & scfq.SCFQ_STRUCT_CHECK else want[:13] + [0] * 12
    assert p.words()[:25] == want25, ("chunked", flags)
    assert p.bytes == a.size
print("ok chunked session")

# ---- the histogram path stays uniform and still matches ----
a = CORPORA["illumina"][:300 * TILE + 99]
flags = scfq.SCFQ_QUAL_HIST | scfq.SCFQ_STRUCT_CHECK
g = scfq.debug_scan_geometry(a.size, 1, flags)
assert g.n_segments == 1 and scfq.debug_scan_geometry(a.size, 1, scfq.SCFQ_STRUCT_CHECK).n_segments >= 3
t, ptr = to_dev(a, 1)
want, want_h = oracle_partial(a, -1, want_hist=True)
for f in (flags | scfq.SCFQ_HIST_EXACT, flags):
    p, h = scfq.partial_device(ptr, a.size, -1, flags=f, want_hist=True)
    assert scfq.debug_last_scan_kernel().endswith(" tiles_per_range=8"), scfq.debug_last_scan_kernel()
    assert p.words()[:25] == want[:25], ("hist", f)
    ks = range(4) if p.hist_class == 0 else [p.hist_class - 1]
    for k in ks:
        assert list(h)[k * 256:(k + 1) * 256] == want_h[k * 256:(k + 1) * 256], ("hist", f, k)
print("ok histogram uniform")

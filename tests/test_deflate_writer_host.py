"""DEFLATE streams zlib's compressor never writes (tests/_deflate_writer.py) through everything on the host that decodes them: zlib
itself (pins the corpus), the library's own inflater, SCFQ_INFLATE=zlib, the parallel single-member reader, BGZF members on the host
threads, the mid-member take-over (scfq_gzfast Resume), the Python models of the device symbol loops, the device search's header
acceptance rule restated, and the r5 split of the BGZF member CRC.  No device."""
import hashlib
import os
import subprocess
import sys
import zlib

import pytest

import _deflate_writer as W
from test_crc32_host import _mulmod, _raw_crc, _tables, _xpow8
from test_dense_loop_model import inflate_dense, new_stats
from test_inflate_host import EnvPatch, pgz_env
from test_lane_loop_model import inflate_in_rounds

HERE = os.path.dirname(os.path.abspath(__file__))
PYHOST = os.path.join(os.path.dirname(HERE), "seq-collection_amd", "pyhost")


@pytest.fixture(scope="module")
def corpus():
    """{name: Builder} of every valid shape, 150 KB (host readers) and one BGZF member's worth (models, BGZF members)"""
    big = {name: W.valid_case(name, 150_000, 11) for name in W.VALID}
    for b in big.values():
        b.raw = b.deflate()
    small = {name: W.member_case(name, 12) for name in W.VALID}
    return {"big": big, "small": small, "invalid": W.invalid_cases()}


def test_writer_output_is_what_zlib_inflates(corpus):
    for size in ("big", "small"):
        for name, b in corpus[size].items():
            assert W.zlib_inflate(b.raw) == bytes(b.data), (size, name)
    for name, raw in corpus["invalid"].items():
        with pytest.raises(zlib.error):
            W.zlib_inflate(raw)
        with pytest.raises(zlib.error):
            zlib.decompress(raw, -15)


def test_the_shapes_are_there(corpus):
    """every shape the corpus claims to hold is in its streams"""
    seen = set()
    for name, b in corpus["big"].items():
        for kind, body, shape in b.blocks:
            if kind == "stored":
                seen.add("stored %s" % ("empty" if not body else "data"))
                continue
            if kind != "dyn":
                continue
            litlens, distlens, hdr = W._dyn_codes(body, shape)
            dists = {t[1] for t in body if t.__class__ is not int}
            seen |= {"distance %d" % d for d in dists & {32768, 32767, 32507}}
            if any(len(t) > 2 and t[2:] == (284, 31) for t in body if t.__class__ is not int):
                seen.add("258 as 284+31")
            used = [s for s, f in enumerate(W.used_symbols(body)[0]) if f]
            if name == "long_codes" and min(litlens[s] for s in used) >= 13:
                seen.add("13-15 bit codes on used symbols")
                if any(t.__class__ is not int and t[0] >= 227 and t[1] > 24576 for t in body):
                    assert litlens[284] == 15 and distlens[29] == 15
                    seen.add("48-bit pairs")
            if sum(1 for v in distlens if v) == 1:
                seen.add("one distance code")
            if not any(distlens):
                seen.add("no distance codes")
            if sum(1 for v in litlens if v) == 1:
                seen.add("one lit/len code")
            if W.lens_alloc(litlens, W.LIT_ROOT) >= 1300:
                seen.add("lit table >= 1300")
            if W.lens_alloc(distlens, W.DIST_ROOT) >= 390:
                seen.add("dist table >= 390")
            assert W.lens_alloc(litlens, W.LIT_ROOT) <= W.LIT_ENTRIES and W.lens_alloc(distlens, W.DIST_ROOT) <= W.DIST_ENTRIES
            items = W.rle_lengths(litlens + distlens, len(litlens), hdr.get("use16", True), hdr.get("use17", True), hdr.get("use18", True),
                                  hdr.get("cross", True))
            seen |= {"crossing run %d" % s for s in W.crossing_runs(items, len(litlens))}
            seen |= {"HLIT %d" % len(litlens) for _ in [0] if len(litlens) in (257, 286)}
            seen |= {"HDIST %d" % len(distlens) for _ in [0] if len(distlens) in (1, 30)}
            if hdr.get("hclen") == 19:
                seen.add("HCLEN 19")
    want = {"distance 32768", "distance 32767", "distance 32507", "258 as 284+31", "13-15 bit codes on used symbols", "48-bit pairs",
            "one distance code", "no distance codes", "one lit/len code", "lit table >= 1300", "dist table >= 390", "crossing run 16",
            "crossing run 18", "HLIT 257", "HLIT 286", "HDIST 1", "HDIST 30", "HCLEN 19", "stored empty", "stored data"}
    assert want <= seen, want - seen


def test_max_table_codes_reach_the_reserve():
    assert W.max_table_counts("lit")[1] >= 1300 and W.max_table_counts("dist")[1] >= 390
    # the reserve itself is zlib's bound (`enough 288 10 15` = 1334, `enough 32 8 15` = 402) plus a few entries
    assert W.max_table_counts("lit")[1] <= 1334 <= W.LIT_ENTRIES and W.max_table_counts("dist")[1] <= 402 <= W.DIST_ENTRIES


def _read(scfq, tmp_path, blob, cap, chunk=1 << 16, name="c.fq.gz"):
    f = tmp_path / name
    f.write_bytes(blob)
    return scfq.debug_read_file(str(f), cap, chunk)


def _rejects(scfq, fn):
    with pytest.raises(scfq.ScfqError) as e:
        fn()
    return e.value.rc == scfq.SCFQ_EGZ


def test_own_inflater_and_parallel_reader(scfq, tmp_path, corpus):
    for name, b in corpus["big"].items():
        data = bytes(b.data)
        blob = W.gzip_member(b.raw, data) + W.gzip_member(corpus["small"][name].raw, bytes(corpus["small"][name].data))
        want = data + bytes(corpus["small"][name].data)
        for chunk in (1 << 16, 0):
            assert _read(scfq, tmp_path, blob, len(want) + 16, chunk) == want, (name, chunk)
        with EnvPatch(pgz_env()):
            assert _read(scfq, tmp_path, blob, len(want) + 16, 1 << 20) == want, (name, "pgz")
    with EnvPatch(pgz_env()):
        # several MB in one member: the parallel reader's segments start inside the crafted shapes
        b = W.Builder(3)
        for name in W.VALID:
            part = W.valid_case(name, 400_000, 21)
            b.blocks += part.blocks
            b.data += part.data
        raw = b.deflate()
        assert W.zlib_inflate(raw) == bytes(b.data)
        assert _read(scfq, tmp_path, W.gzip_member(raw, bytes(b.data)), len(b.data) + 16, 1 << 20) == bytes(b.data)
    for name, raw in corpus["invalid"].items():
        blob = W.gzip_member(raw, b"")
        assert _rejects(scfq, lambda: _read(scfq, tmp_path, blob, 1 << 20)), name
        with EnvPatch(pgz_env()):
            assert _rejects(scfq, lambda: _read(scfq, tmp_path, blob, 1 << 20)), (name, "pgz")


def test_zlib_switch_on_the_corpus(scfq, tmp_path, corpus):
    """SCFQ_INFLATE=zlib and =own (read once per process) give the same bytes and the same rejections"""
    paths, want = [], []
    for name, b in corpus["big"].items():
        f = tmp_path / (name + ".gz")
        f.write_bytes(W.gzip_member(b.raw, bytes(b.data)))
        paths.append(str(f))
        want.append(hashlib.sha256(bytes(b.data)).hexdigest())
    for name, raw in corpus["invalid"].items():
        f = tmp_path / (name + ".bad.gz")
        f.write_bytes(W.gzip_member(raw, b""))
        paths.append(str(f))
        want.append("EGZ")
    code = ("import sys, hashlib; sys.path.insert(0, sys.argv[1]); import scfq\n"
            "for p in sys.argv[2:]:\n"
            "    try: print(hashlib.sha256(scfq.debug_read_file(p, 1 << 21, 1 << 16)).hexdigest())\n"
            "    except scfq.ScfqError as e: print('EGZ' if e.rc == scfq.SCFQ_EGZ else e.rc)\n")
    for mode in ("zlib", "own"):
        r = subprocess.run([sys.executable, "-c", code, PYHOST] + paths, env=dict(os.environ, SCFQ_INFLATE=mode), capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.split() == want, (mode, r.stderr[-2000:])


def test_bgzf_members_on_the_host_threads(scfq, tmp_path, corpus):
    img, want = b"", b""
    for name, b in corpus["small"].items():
        data = bytes(b.data)
        assert len(data) <= 65536
        img += W.bgzf_member(b.raw, data)
        want += data
    img += W.bgzf_member(W.Builder().deflate(), b"")
    for chunk in (1 << 16, 1 << 20):
        assert _read(scfq, tmp_path, img, len(want) + 16, chunk) == want, chunk
    for name, raw in corpus["invalid"].items():
        bad = W.bgzf_member(corpus["small"]["far_distances"].raw, bytes(corpus["small"]["far_distances"].data)) + W.bgzf_member(raw, b"")
        assert _rejects(scfq, lambda: _read(scfq, tmp_path, bad + W.bgzf_member(W.Builder().deflate(), b""), 1 << 20)), name


def test_resume_at_every_block_boundary(scfq, tmp_path, corpus):
    """the take-over (scfq_gzfast Resume) cut at each block start of a crafted member"""
    for name in ("far_distances", "len284_31", "long_codes", "sync_flush", "header_edges", "max_tables"):
        b = corpus["big"][name]
        data = bytes(b.data)
        f = tmp_path / (name + ".gz")
        f.write_bytes(W.gzip_member(b.raw, data))
        for at in sorted(set(b.block_out)):
            assert scfq.debug_gz_resume(str(f), at, len(data) + 16, 1 << 16) == data, (name, at)


def test_device_loop_models_on_the_corpus():
    """(the models walk every bit in Python: a few KB of each shape, distances as far as that history allows; then the far end of
    the window in streams made for the models)"""
    for name in W.VALID:
        b = W.valid_case(name, 3_000, 12)
        b.raw = b.deflate()
        data = bytes(b.data)
        assert len(data) <= 65536
        assert inflate_dense(b.raw, new_stats()) == data, name
        assert inflate_in_rounds(b.raw, {"rounds": 0, "alone": 0}) == data, name
    # the far end of the window and the longest pairs: 34 KB of history as one stored block (cheap for the models), then copies of
    # distance 32 768 / 32 767 / 32 507, 258 as 284 + 31, and length code 284 with distance code 29 on 15-bit codes (48 bits a pair)
    for seed in (7, 8):
        b = W.far_model_case(seed)
        raw, data = b.deflate(), bytes(b.data)
        far = {t[1] for kind, body, _ in b.blocks if kind == "dyn" for t in body if t.__class__ is not int}
        assert {32768, 32767, 32507} <= far and any(d > 24576 for d in far - {32768, 32767, 32507})
        kind, body, shape = b.blocks[-1]
        litlens, distlens, _ = W._dyn_codes(body, shape)
        assert litlens[284] == 15 and distlens[29] == 15 and any(t.__class__ is not int and 227 <= t[0] < 258 for t in body)
        assert W.zlib_inflate(raw) == data
        assert inflate_dense(raw, new_stats()) == data, seed
        assert inflate_in_rounds(raw, {"rounds": 0, "alone": 0}) == data, seed


# ---- the device search's acceptance rule (gz_inflate_kernels.hpp: sync_fields32, sync_kraft, sync_deep / sync_deep_tab) -----------
class _Bits:
    def __init__(self, raw, bit):
        self.v, self.p = int.from_bytes(raw + bytes(64), "little"), bit

    def take(self, n):
        x = (self.v >> self.p) & ((1 << n) - 1)
        self.p += n
        return x


def search_accepts(raw, bit):
    """position `bit` may start a dynamic block (lit_mask 0): the kernel's rule, step by step"""
    r = _Bits(raw, bit)
    r.take(1)
    if r.take(2) != 2:
        return False
    hlit_f, hdist_f, hclen = r.take(5), r.take(5), r.take(4) + 4
    if hlit_f > 29 or hdist_f > 29:                                          # sync_fields32
        return False
    hlit, hdist = hlit_f + 257, hdist_f + 1
    cl = [0] * 19
    for k in range(hclen):
        cl[W.CL_ORDER[k]] = r.take(3)
    if W.kraft(cl, 7) != 128:                                                # sync_kraft: a complete code-length code
        return False
    codes = {c: s for s, c in enumerate(W.canonical(cl)) if c[1]}
    k, prev, kraft_l, kraft_d, n_d, max_d, len256 = 0, 0, 0, 0, 0, 0, 0
    total = hlit + hdist
    while k < total:
        code = n = 0
        while (code, n) not in codes:
            code |= r.take(1) << n
            n += 1
        sym = codes[(code, n)]
        rep, val = 1, sym
        if sym == 16:
            if k == 0:
                return False
            val, rep = prev, 3 + r.take(2)
        elif sym == 17:
            val, rep = 0, 3 + r.take(3)
        elif sym == 18:
            val, rep = 0, 11 + r.take(7)
        if k + rep > total:
            return False
        if val:
            in_l = 0 if k >= hlit else (rep if k + rep <= hlit else hlit - k)
            in_d = rep - in_l
            kraft_l += in_l * (32768 >> val)
            kraft_d += in_d * (32768 >> val)
            if kraft_l > 32768 or kraft_d > 32768:
                return False
            if k <= 256 < k + rep:
                len256 = val
            if in_d:
                n_d += in_d
                max_d = max(max_d, val)
        k += rep
        prev = val
    if len256 == 0 or kraft_l != 32768:
        return False
    return kraft_d == 32768 or n_d == 0 or (n_d == 1 and max_d == 1)


def test_search_rule_accepts_every_complete_header(corpus):
    n = 0
    for size in ("big", "small"):
        for name, b in corpus[size].items():
            for (kind, body, shape), bit in zip(b.blocks, b.block_bits):
                if kind != "dyn":
                    continue
                litlens = W._dyn_codes(body, shape)[0]
                if sum(1 for v in litlens if v) == 1:
                    # an incomplete lit/len code of one 1-bit code (a block of nothing but end-of-block): zlib accepts it, the search
                    # does not by design (gz_inflate_kernels.hpp: "never a real block"); the walk decodes such a block as a gap
                    assert not search_accepts(b.raw, bit), (name, bit)
                else:
                    assert search_accepts(b.raw, bit), (name, bit)
                    n += 1
    assert n > 100


def test_search_rule_rejects_invalid_headers(corpus):
    """the invalid dynamic headers start right after a valid block: the rule must refuse every one that zlib refuses at the header"""
    header_cases = ("oversubscribed_litlen", "oversubscribed_dist", "incomplete_litlen", "no_end_of_block_code", "repeat16_first",
                    "repeats_overrun", "hlit_287", "hdist_31")
    for name in header_cases:
        b = W.Builder(5)
        b.records(3_000)
        b.cut()
        b.raw_block(lambda w, last: None)
        b.deflate()
        bit = b.block_bits[-1]
        raw = corpus["invalid"][name]
        assert search_accepts(raw, 0) and not search_accepts(raw, bit), name


# ---- the r5 BGZF member CRC (bgzf_inflate_kernel.hpp: bgzf_crc_consts_init, bgzf_crc32_members) ---------------------------------
def crc_consts():
    """g_crc_consts: [t] x^(8 * 256 * (255 - t)), [256 + lo] x^(8 lo), [512 + hi] x^(8 * 256 hi), hi = 0 .. 256"""
    c = [0] * (3 * 256 + 8)
    for t in range(256):
        c[t] = _xpow8(256 * (255 - t))
        c[256 + t] = _xpow8(t)
        c[512 + t] = _xpow8(256 * t)
    c[512 + 256] = _xpow8(65536)
    return c


def member_crc_r5(data, consts, tabs):
    """256 threads x 256 bytes of a 64 KiB virtual message (zeros, then the member), one product per thread, xor-reduced"""
    n = len(data)
    assert n <= 65536
    pad = 65536 - n
    red = 0
    for t in range(256):
        v = 256 * t
        if v + 256 <= pad:
            continue                                         # all zeros: c = 0
        c = _raw_crc(data[v - pad:v - pad + 256], tabs) if v >= pad else _raw_crc(data[:v + 256 - pad], tabs)
        red ^= _mulmod(consts[t], c)
    xn = _mulmod(consts[512 + (n >> 8)], consts[256 + (n & 255)])
    return red ^ _mulmod(xn, 0xFFFFFFFF) ^ 0xFFFFFFFF


def test_bgzf_member_crc_split_of_r5():
    import random
    tabs, consts, rng = _tables(), crc_consts(), random.Random(8)
    for n in (0, 1, 255, 256, 257, 65279, 65280, 65535, 65536):
        data = bytes(rng.randrange(256) for _ in range(n))
        assert member_crc_r5(data, consts, tabs) == zlib.crc32(data), n

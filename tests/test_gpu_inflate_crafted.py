"""The device inflaters (bgzf_inflate, gz_segment_decode and the search in front of it) on DEFLATE streams zlib's compressor never
writes (tests/_deflate_writer.py): far distances up to 32 768, 258 as 284 + 31, one or no distance codes, precode runs across the
literal/length | distance border, 15-bit codes on used symbols, tables at the LDS reserve, sync-flush stored blocks; invalid streams;
BGZF members of every ISIZE edge; and references to bytes before a member's start whose trailer agrees with a lenient decoder.
Tiny images first, then valid streams, then invalid ones."""
import hashlib
import os
import socket
import subprocess
import sys
import zlib

import numpy as np
import pytest

import _deflate_writer as W
from conftest import PKG
from test_ingest_sources import bgzf_block, fastq_bytes

pytestmark = pytest.mark.gpu

SC = os.path.join(PKG, "sc")
PYHOST = os.path.join(PKG, "pyhost")
DEV_ENV = {"SCFQ_GZ_DEVICE_MIN_MB": "0", "SCFQ_GZ_DEVICE_SEGMENT_KB": "32", "SCFQ_VERBOSE": "1"}
BATCH_ENV = dict(DEV_ENV, SCFQ_GZ_DEVICE_BATCH_SEGMENTS="8", SCFQ_GZ_DEVICE_CHAIN_GROUP="3")
GROUP_ENV = dict(DEV_ENV, SCFQ_GZ_DEVICE_CHAIN_GROUP="5")
SEG16_ENV = dict(DEV_ENV, SCFQ_GZ_DEVICE_SEGMENT_KB="16")
EOF_MEMBER = bgzf_block(b"")


def run(path, **env):
    return subprocess.run([SC, "fq-count", str(path)], capture_output=True, text=True, env=dict(os.environ, **env), timeout=300)


def strip(s):
    return "\n".join(ln for ln in s.splitlines() if not ln.startswith("scfq"))


def test_small_crafted_images_first(gpu, scfq):
    """a few KB of every shape, one member each: a kernel fault shows up here before anything large runs"""
    for name in W.VALID:
        b = W.valid_case(name, 3_000, 31)
        raw = b.deflate()
        data = bytes(b.data)
        assert W.zlib_inflate(raw) == data
        assert scfq.debug_bgzf_inflate(W.bgzf_member(raw, data) + EOF_MEMBER, len(data) + 16) == data, name


_LOOP_CHILD = """
import sys, hashlib
sys.path.insert(0, sys.argv[1])
import scfq
for p in sys.argv[2:]:
    img = open(p, "rb").read()
    try:
        print(hashlib.sha256(scfq.debug_bgzf_inflate(img, 1 << 24)).hexdigest())
    except scfq.ScfqError as e:
        print("EGZ" if e.rc == scfq.SCFQ_EGZ else "rc%d" % e.rc)
"""


def test_crafted_bgzf_members_in_all_three_loops(gpu, tmp_path):
    """every valid shape cut into members of at most 64 KiB (several seeds: one image), every invalid stream as the second member
    of an image of its own; dense, lanes and serial symbol loops, each in a process of its own"""
    members, data = [], b""
    for seed in (41, 42, 43):
        for name in W.VALID:
            b = W.member_case(name, seed)
            members.append(W.bgzf_member(b.raw, bytes(b.data)))
            data += bytes(b.data)
    paths, want = [], []
    f = tmp_path / "valid.bgzf"
    f.write_bytes(b"".join(members) + EOF_MEMBER)
    paths.append(str(f))
    want.append(hashlib.sha256(data).hexdigest())
    for name, raw in W.invalid_cases().items():
        f = tmp_path / (name + ".bgzf")
        f.write_bytes(members[0] + W.bgzf_member(raw, b"") + EOF_MEMBER)
        paths.append(str(f))
        want.append("EGZ")
    for loop in ("dense", "lanes", "serial"):
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", _LOOP_CHILD, PYHOST] + paths,
                           env=dict(os.environ, SCFQ_INFLATE_LOOP=loop), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (loop, r.stderr[-2000:])
        got = r.stdout.split()
        assert got == want, (loop, [(os.path.basename(p), g) for p, g, w in zip(paths, got, want) if g != w])


def _member_of(n, seed):
    """a BGZF member of exactly n bytes of FASTQ text (compressible enough for BSIZE at n = 65 536)"""
    data = fastq_bytes(n + 1000, seed=seed)[:n]
    b = W.Builder(seed)
    b.text(data)
    raw = b.deflate()
    assert bytes(b.data) == data and W.zlib_inflate(raw) == data
    return W.bgzf_member(raw, data), data


def test_bgzf_member_isize_edges(gpu, scfq, oracle, tmp_path):
    """ISIZE 0, 1, 255, 256, 257, 65 279, 65 280, 65 535, 65 536: the 256-byte borders of the CRC split and its x^(8 * 65 536) entry,
    first, in the middle and last in one image; the bytes, and count_file against the oracle"""
    sizes = (0, 1, 255, 256, 257, 65279, 65280, 65535, 65536)
    edge = [_member_of(n, 60 + i) for i, n in enumerate(sizes)]
    filler = [_member_of(40_000, 90 + i) for i in range(3)]
    for order in (edge + filler, filler[:1] + edge + filler[1:], filler + edge):
        img = b"".join(m for m, _ in order) + EOF_MEMBER
        data = b"".join(d for _, d in order)
        assert scfq.debug_bgzf_inflate(img, len(data) + 16) == data
        f = tmp_path / "edges.fq.gz"
        f.write_bytes(img)
        oc = oracle.count(np.frombuffer(data, dtype=np.uint8))
        c = scfq.count_file(str(f), flags=scfq.SCFQ_QUAL_HIST | scfq.SCFQ_STRUCT_CHECK)
        for fld in ("reads", "gc_bases", "n_bases", "bases", "lines", "newlines", "input_bytes", "bad_at", "bad_plus"):
            assert getattr(c, fld) == getattr(oc, fld), fld
        assert list(c.qual_hist) == list(oc.qual_hist)
    # and one the device must refuse: the 65 536-byte member with a CRC-32 off by one bit
    m, d = edge[-1]
    bad = m[:-8] + bytes([m[-8] ^ 1]) + m[-7:]
    with pytest.raises(scfq.ScfqError) as e:
        scfq.debug_bgzf_inflate(bad + EOF_MEMBER, len(d) + 16)
    assert e.value.rc == scfq.SCFQ_EGZ


# a first record whose name holds a byte of each literal class above 127: the search rules out block headers that give codes to literal
# classes absent from the file's first 192 KiB (gz_inflate_kernels.hpp: lit_mask) — a heuristic, by design; the maximal tables give every
# literal a code, so without this record their blocks are decoded as gaps (a right row, but not the chain this test is about)
CLASS_RECORD = b"@classes \x80\xa0\xc0\xe0\nACGT\n+\nFFFF\n"


def _big_member(name, size, seed):
    b = W.valid_case(name, size, seed, head=CLASS_RECORD)
    raw = b.deflate()
    data = bytes(b.data)
    assert W.zlib_inflate(raw) == data
    return W.gzip_member(raw, data), data


def test_crafted_gzip_members_on_the_device_path(gpu, oracle, tmp_path):
    """sc fq-count on a 2 MB member of each shape, in four environments (32 KiB segments, batches of 8, chain groups of 5, 16 KiB
    segments): row == oracle; shapes whose block headers the search takes run on the chain, in more than one segment"""
    for name in W.VALID:
        blob, data = _big_member(name, 2_000_000, 51)
        f = tmp_path / (name + ".fq.gz")
        f.write_bytes(blob)
        want = oracle.tsv(oracle.count(np.frombuffer(data, dtype=np.uint8))) + "\n"
        for env in (BATCH_ENV, GROUP_ENV, DEV_ENV, SEG16_ENV):
            r = run(f, **env)
            assert r.returncode == 0 and r.stdout == want, (name, env, r.stderr[-2000:])
            if name in W.SEARCH_REJECTS:
                # the one-code lit/len block (end-of-block only) is not a block start to the search by design (gz_inflate_kernels.hpp:
                # sync_deep_tab, "never a real block"): where it falls behind a segment border the walk decodes it as a gap; the row is
                # what counts
                continue
            assert "on the chain" in r.stderr and "host path" not in r.stderr, (name, env, r.stderr[-2000:])
            line = [ln for ln in r.stderr.splitlines() if "segments planned" in ln][-1]
            decoded = int(line.split(" decoded")[0].split(", ")[-1])
            assert decoded > 1, (name, line)


def test_far_copies_across_segment_and_batch_borders(gpu, oracle, tmp_path):
    """literal-only stretches of blocks whose output is close to 32 768 bytes on either side, every block opened by copies of
    distance 32 768 (and 32 767, 32 507): the window of a segment shorter than the window reaches two segments back"""
    b = W.Builder(71)
    b.records(40_000, literal=True)
    b.cut()
    r = b.rng
    while len(b.data) < 4_000_000:
        for d in (32768, 32768, 32767, 32507):
            b.far_record_copy(d, force258=r.random() < 0.5)
        target = len(b.data) + r.choice([31_000, 32_000, 32_600, 33_000, 34_500, 16_000])
        while len(b.data) < target:
            b.record(r.randint(20, 300), literal=True)
        b.cut()
    raw = b.deflate()
    data = bytes(b.data)
    assert W.zlib_inflate(raw) == data
    f = tmp_path / "far.fq.gz"
    f.write_bytes(W.gzip_member(raw, data))
    want = oracle.tsv(oracle.count(np.frombuffer(data, dtype=np.uint8))) + "\n"
    for env in (BATCH_ENV, GROUP_ENV, DEV_ENV, SEG16_ENV):
        res = run(f, **env)
        assert res.returncode == 0 and res.stdout == want, (env, res.stderr[-2000:])
        assert "on the chain" in res.stderr and "host path" not in res.stderr, (env, res.stderr[-2000:])


def test_invalid_streams_on_the_device_gzip_path(gpu, tmp_path):
    """2 MB of valid blocks, then each invalid stream's bad block: exit code, row and messages as on the host path (gzread)"""
    good = W.valid_case("far_distances", 2_000_000, 52)
    good_raw = good.deflate()
    for name, raw in W.invalid_cases().items():
        f = tmp_path / (name + ".fq.gz")
        # the valid part, then the invalid stream as a member of its own: a damaged second member
        f.write_bytes(W.gzip_member(good_raw, bytes(good.data)) + W.gzip_member(raw, b""))
        host = run(f, SCFQ_GZ_DEVICE="0")
        assert host.returncode != 0 and host.stdout == "", (name, host.stderr[-500:])
        for env in (DEV_ENV, BATCH_ENV, GROUP_ENV):
            dev = run(f, **env)
            assert (dev.returncode, dev.stdout) == (host.returncode, host.stdout), (name, dev.stderr[-1500:])
            assert strip(dev.stderr) == strip(host.stderr), name


# ---- references before a member's start ------------------------------------------------------------------------------------------
def toofar_member(history, seed, n_out, early=30_000, every=3_000):
    """a member that is valid apart from copies reaching up to 32 KiB before its own start, one in every block of its first `early`
    bytes (blocks of `every` bytes), then FASTQ text to n_out bytes.  Returns (raw, [output with the previous member's bytes in front,
    output with zeros in front])"""
    b = W.Builder(seed)
    b.data = bytearray(history[-32768:])
    h = len(b.data)
    r = b.rng
    while len(b.data) - h < early:
        b.records(every // 2, literal=True)
        own = len(b.data) - h
        b.copy(own + r.randint(1, min(h, 32768 - own) - 300), r.randint(3, 258))
        b.cut()
    b.records(n_out - (len(b.data) - h))
    b.cut()
    raw = b.deflate()
    lenient = [W.lenient_inflate(raw, history), W.lenient_inflate(raw, zeros=True)]
    assert lenient[0] == bytes(b.data[h:]) and lenient[1] != lenient[0]
    with pytest.raises(zlib.error):
        W.zlib_inflate(raw)
    return raw, lenient


def test_bgzf_reference_before_the_member_start(gpu, scfq):
    first = fastq_bytes(60_000, seed=81)[:60_000]
    m1 = W.Builder(2)
    m1.text(first)
    raw1 = m1.deflate()
    raw2, lenient = toofar_member(first, 82, 50_000, early=20_000)
    for out in lenient:
        img = W.bgzf_member(raw1, first) + W.bgzf_member(raw2, out) + EOF_MEMBER
        with pytest.raises(scfq.ScfqError) as e:
            scfq.debug_bgzf_inflate(img, 1 << 20)
        assert e.value.rc == scfq.SCFQ_EGZ


def _two_member_file(tmp_path, variant, m1_bytes, m2_bytes, name):
    a = fastq_bytes(m1_bytes + 1000, seed=83)[:m1_bytes]
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 9)
    raw1 = co.compress(a) + co.flush()
    raw2, lenient = toofar_member(a, 84, m2_bytes)
    f = tmp_path / name
    f.write_bytes(W.gzip_member(raw1, a) + W.gzip_member(raw2, lenient[variant]))
    return f


def test_gzip_reference_before_the_member_start(gpu, tmp_path):
    for variant in (0, 1):
        f = _two_member_file(tmp_path, variant, 3_000_000, 2_000_000, "toofar%d.fq.gz" % variant)
        host = run(f, SCFQ_GZ_DEVICE="0")
        assert host.returncode != 0 and host.stdout == "", host.stderr[-500:]
        for env in (DEV_ENV, BATCH_ENV, GROUP_ENV):
            dev = run(f, **env)
            assert (dev.returncode, dev.stdout) == (host.returncode, host.stdout), (variant, env, dev.stderr[-1500:])
            assert strip(dev.stderr) == strip(host.stderr), (variant, env)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_ranks_raw(world, path, env):
    """`sc fq-count --shard-rank` processes over TCP; (exit codes, (stdout, stderr)) in rank order, whatever the exit codes"""
    port = _free_port()
    procs = [subprocess.Popen(["timeout", "-k", "10", "240", SC, "fq-count", "--shard-rank=%d" % r, "--shard-world=%d" % world,
                               "--rendezvous=127.0.0.1:%d" % port, "--transport=tcp", "--devices=0", str(path)],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=dict(os.environ, **env))
             for r in reversed(range(world))]
    outs = [p.communicate(timeout=300) for p in procs]
    return [p.returncode for p in procs][::-1], outs[::-1]


_FASTQ = {}


def _block_scheme_file(path, variant, world=3, clean_blocks=3, far_blocks=3):
    """Two members laid out for the block scheme of a sharded count (scfq_api.hip: at least world x 8 MiB, at most one member start
    per share): member 2 starts in rank 1's share, and rank 2's share begins one byte in front of member 2's block `clean_blocks`, so
    that rank 2's stretch begins at that block, about 6 KB (less than 32 KiB) of output into member 2.  The blocks up to about 28 KB of
    output are valid; the `far_blocks` behind them each copy bytes from before member 2's start (variant 0: the trailer's CRC-32 is that
    of a decoder that reads member 1's bytes there, variant 1: zeros; None: no such copies, a valid file); the rest of member 2 is an
    ordinary deflate stream behind an empty stored block.  Returns the bytes zlib inflates (None: it rejects the file)."""
    world_min = world * (8 << 20)
    if world not in _FASTQ:
        tail = fastq_bytes(world_min * 95 // 100, seed=92)              # member 2's ordinary part: level 1, ~2.6 : 1, over a third of the file
        _FASTQ[world] = (fastq_bytes(2 * len(tail) + (4 << 20), seed=91), tail)     # member 1: about twice member 2 (what is needed of it)
    a, tail = _FASTQ[world]
    hist = a[-32768:]
    b = W.Builder(93)
    b.data = bytearray(hist)
    h = len(b.data)
    r = b.rng
    for k in range(clean_blocks):
        b.records(2_000, literal=True)
        b.cut()
    # ~20 KB of output on 13 - 15-bit literal codes (~40 KB of deflate data): the stretch in front of rank 2 (rank 1's, which decodes a
    # little past its end to prove it) does not reach the blocks below; only rank 2's own window check can refuse them
    while len(b.data) - h < 25_000:
        b.records(1_000, literal=True)
        b.cut(lit="long", dist="none")
    for k in range(far_blocks):
        b.records(500, literal=True)
        own = len(b.data) - h
        assert own + 400 < 32768
        if variant is not None:
            b.copy(own + r.randint(1, 32768 - own - 300), r.randint(3, 258))
        b.cut()
    b.stored(b"")
    head_raw = b.deflate(final=False)
    co = zlib.compressobj(1, zlib.DEFLATED, -15, 9)
    raw2 = head_raw + co.compress(tail) + co.flush()
    own2 = bytes(b.data[h:]) + tail
    if variant is None:
        out2 = own2
        assert W.zlib_inflate(raw2) == own2
    else:
        out2 = W.lenient_inflate(raw2, a if variant == 0 else b"", zeros=variant == 1)
        with pytest.raises(zlib.error):
            W.zlib_inflate(raw2)
    m2 = W.gzip_member(raw2, out2)
    cut_off = 10 + (b.block_bits[clean_blocks] >> 3) - 1            # rank 2's share starts here, relative to member 2's start
    # member 1: level 1 up to a little short of its size (full flushes: byte-aligned, not final), then one final stored block whose
    # length sets member 1's size M1 so that the share of rank 2 starts exactly at M1 + cut_off: 2 * ((M1 + |m2|) // 3) == M1 + cut_off
    target = next(m1 for m1 in range(2 * len(m2) - 3 * cut_off - 8, 2 * len(m2) - 3 * cut_off + 8)
                  if (m1 + len(m2)) // world * (world - 1) == m1 + cut_off)
    co = zlib.compressobj(1, zlib.DEFLATED, -15, 9)
    zpart, used = b"", 0
    while len(zpart) < target - 23 - 40_000:                          # (a full flush every 64 KiB: the length so far is exact)
        zpart += co.compress(a[used:used + 65536]) + co.flush(zlib.Z_FULL_FLUSH)
        used += 65536
        assert used < len(a)
    pad = target - 18 - len(zpart) - 5
    assert 0 <= pad <= 65535, pad
    data1 = a[:used] + a[used:used + pad]
    assert len(data1) == used + pad
    w = W.BitWriter()
    W.write_stored(w, 1, data1[used:])
    m1 = W.gzip_member(zpart + w.getvalue(), data1)
    assert len(m1) == target
    size = len(m1) + len(m2)
    assert size >= world_min and size // world * (world - 1) == len(m1) + cut_off and size // world < len(m1)
    with open(path, "wb") as fh:
        fh.write(m1 + m2)
    return data1 + own2 if variant is None else None


def test_sharded_stretch_reference_before_the_member_start(gpu, oracle, tmp_path):
    """3 ranks, block scheme: rank 2's stretch begins at a block start about 6 KB into member 2, and blocks of it that lie less than
    32 KiB into the member copy bytes from before member 2's start.  The count must end as the single process's does — exit code,
    stdout and gzread's message alone — with no row.  First the same layout without those copies: the block scheme runs (rank 2
    inflates a stretch of its own, the cuts join up) and the row is the oracle's.
    (What refuses the damaged file here is the stretch in front of rank 2: rank 1's, which meets a member end although it was to end at
    a block boundary (scfq_gzdev.hpp, "the file is not ONE member after all"), so the exchange does not join up.  Rank 2's own check of
    its window against the history that exists (GzStretch::valid) is not what this test reaches.)"""
    env = {"SCFQ_VERBOSE": "1"}
    f = tmp_path / "shard_ok.fq.gz"
    data = _block_scheme_file(f, None)
    codes, outs = _run_ranks_raw(3, f, env)
    assert codes == [0, 0, 0], (codes, [o[1][-1500:] for o in outs])
    assert outs[0][0] == oracle.tsv(oracle.count(np.frombuffer(data, dtype=np.uint8))) + "\n", outs[0][1][-2000:]
    assert "scfq gzdev" in outs[2][1] and "did not join up" not in outs[0][1], outs[2][1][-2000:]
    for variant in (0, 1):
        f = tmp_path / ("shard%d.fq.gz" % variant)
        _block_scheme_file(f, variant)
        host = run(f, SCFQ_GZ_DEVICE="0")
        assert host.returncode != 0 and host.stdout == "", host.stderr[-500:]
        codes, outs = _run_ranks_raw(3, f, env)
        assert all(c not in (124, 137) for c in codes), codes
        # (rank 2 inflated the stretch behind its block cut: the block scheme ran, not the member one, where rank 2 holds no member)
        assert "scfq gzdev" in outs[2][1], (variant, outs[2][1][-2000:])
        assert (codes[0], outs[0][0]) == (host.returncode, host.stdout), (variant, codes, [o[1][-1500:] for o in outs])
        assert strip(outs[0][1]) == strip(host.stderr), (variant, outs[0][1][-1500:], host.stderr[-500:])

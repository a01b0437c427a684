"""The range geometry of a scan launch (csrc/fq_scan_geometry.hpp) through scfq_debug_scan_geometry: host only, no device."""
import pytest

TILE = 4096
MAX_TPR = 960
MAX_SEGMENTS = 6


def geometry(scfq, n_tiles, **kw):
    return scfq.debug_scan_geometry(n_tiles * TILE, **kw)


def check(g, n_tiles):
    """every property a launch relies on; returns the segments"""
    segs = g.segments()
    assert 1 <= len(segs) <= MAX_SEGMENTS
    assert g.n_tiles == n_tiles
    assert segs[0][0] == 0 and segs[0][1] == 0
    n_ranges = 0
    for s, (first_range, first_tile, tpr) in enumerate(segs):
        end_tile = segs[s + 1][1] if s + 1 < len(segs) else n_tiles
        assert 1 <= tpr <= MAX_TPR
        assert first_range == n_ranges, "segments are contiguous in ranges"
        assert end_tile > first_tile, "no empty segment"
        # ranges of tpr tiles from first_tile, the last one clipped to end_tile: every tile of [first_tile, end_tile) is in exactly one,
        # and the next segment starts where this one ends
        n_ranges += -(-(end_tile - first_tile) // tpr)
        if s:
            assert tpr <= segs[s - 1][2], "range sizes never grow"
        if s + 1 < len(segs):
            assert (end_tile - first_tile) % tpr == 0, "only the last range of a launch is clipped"
    assert g.n_ranges == n_ranges
    return segs


def test_small_base_every_size(scfq, monkeypatch):
    monkeypatch.setenv("SCFQ_TILES_PER_RANGE", "8")
    monkeypatch.setenv("SCFQ_TAPER_WAVES", "4")
    tapered = 0
    for n_tiles in range(1, 2001):
        segs = check(geometry(scfq, n_tiles), n_tiles)
        assert segs[0][2] == 8 or len(segs) == 1
        tapered += len(segs) >= 3
        if n_tiles <= 4 * 8:      # resident all at once: uniform
            assert segs == [(0, 0, 8)]
    assert tapered > 1900
    for n_tiles in (7, 8, 9):
        assert check(geometry(scfq, n_tiles), n_tiles) == [(0, 0, 8)]


@pytest.mark.parametrize("n_tiles", [1, 2, 15, 16, 17, 99, 100, 101, 2_441_407, 2**32 - 2])
def test_default_base(scfq, monkeypatch, n_tiles):
    monkeypatch.delenv("SCFQ_TILES_PER_RANGE", raising=False)
    monkeypatch.delenv("SCFQ_TAPER_WAVES", raising=False)
    segs = check(geometry(scfq, n_tiles), n_tiles)
    if n_tiles == 2_441_407:      # the 10 GB launch of the benchmark on 256 CUs
        assert segs[0][2] == 100 and len(segs) >= 3
    # the histogram forms keep uniform ranges of the same base size
    h = geometry(scfq, n_tiles, flags=scfq.SCFQ_QUAL_HIST)
    assert check(h, n_tiles) == [(0, 0, segs[0][2])]


@pytest.mark.parametrize("tpr", [None, 1, 8, 100, 960])
def test_taper_off_is_uniform(scfq, monkeypatch, tpr):
    monkeypatch.setenv("SCFQ_TAPER_WAVES", "0")
    if tpr is None:
        monkeypatch.delenv("SCFQ_TILES_PER_RANGE", raising=False)
    else:
        monkeypatch.setenv("SCFQ_TILES_PER_RANGE", str(tpr))
    for n_tiles in (1, 2, 7, 8, 9, 1999, 2_441_407, 2**32 - 2):
        g = geometry(scfq, n_tiles)
        segs = check(g, n_tiles)
        assert len(segs) == 1
        base = segs[0][2]
        if tpr is not None:
            assert base == tpr
        assert g.n_ranges == -(-n_tiles // base)


def test_pointer_offset_counts_tiles(scfq, monkeypatch):
    monkeypatch.setenv("SCFQ_TILES_PER_RANGE", "8")
    monkeypatch.setenv("SCFQ_TAPER_WAVES", "4")
    assert scfq.debug_scan_geometry(300 * TILE, ptr_offset=0).n_tiles == 300
    assert scfq.debug_scan_geometry(300 * TILE, ptr_offset=1).n_tiles == 301
    assert scfq.debug_scan_geometry(300 * TILE - 4095, ptr_offset=4095).n_tiles == 300
    assert scfq.debug_scan_geometry(1, ptr_offset=4095).n_tiles == 1

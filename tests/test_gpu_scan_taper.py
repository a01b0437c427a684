"""The tapered range geometry of the scan kernel (big ranges first, small ranges last) must not change a single word of a partial.
SCFQ_TILES_PER_RANGE=8 SCFQ_TAPER_WAVES=4 bring the taper (8 / 4 / 2 tiles per range) down to inputs of a few hundred tiles; the cases
run in ONE child process with those knobs (tests/_scan_taper_check.py), which asserts through scfq_debug_scan_geometry that at least
three segments are in force wherever a case is about the taper, and prints one line per group of cases."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def child(gpu):
    e = dict(os.environ)
    e.update({"SCFQ_TILES_PER_RANGE": "8", "SCFQ_TAPER_WAVES": "4"})
    return subprocess.run([sys.executable, os.path.join(HERE, "_scan_taper_check.py")], env=e, capture_output=True, text=True)


def group_ok(child, name):
    assert "ok " + name in child.stdout.splitlines(), child.stdout + child.stderr


@pytest.mark.parametrize("tiles", [1, 9, 300, 1023])
def test_every_corpus_offset_and_flag(child, tiles):
    group_ok(child, "tiles %d" % tiles)


def test_crlf_and_record_start_on_every_segment_boundary(child):
    group_ok(child, "segment boundaries")


def test_chunked_session_every_chunk_tapered(child):
    group_ok(child, "chunked session")


def test_histogram_path_stays_uniform(child):
    group_ok(child, "histogram uniform")


def test_child_ran_to_its_end(child):
    assert child.returncode == 0, child.stdout + child.stderr

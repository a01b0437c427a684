"""tests/_caller_cases.py can tell right from wrong before a device sees it: the table covers every `*_device` wrapper, a decoy has its
input's byte length and another result in every part that tests/test_gpu_caller_stream.py compares, the twelve worker seeds of
tests/test_gpu_threads.py give twelve different results, and every planted case occurs."""
import itertools

import numpy as np
import pytest

import _caller_cases as T


def differs(a, b):
    return type(a) != type(b) or a != b


def test_the_table_names_every_device_wrapper(scfq):
    wrappers = {name for name in dir(scfq) if name.endswith("_device")}
    jobs = {T.wrapper_of(j) for j in T.JOBS}
    assert jobs <= wrappers, jobs - wrappers
    assert set(T.OUTSIDE_THE_CONTRACT) <= wrappers and not set(T.OUTSIDE_THE_CONTRACT) & jobs
    assert all(reason for reason in T.OUTSIDE_THE_CONTRACT.values())
    assert wrappers == jobs | set(T.OUTSIDE_THE_CONTRACT), wrappers ^ (jobs | set(T.OUTSIDE_THE_CONTRACT))
    assert len(T.BY_NAME) == len(T.JOBS)
    # the forms the table owes besides one job per wrapper
    names = set(T.BY_NAME)
    for wrapper in ("insert_size", "merge", "trim", "screen", "demux", "norm"):
        assert {wrapper + "_device", wrapper + "_device interleaved"} <= names, wrapper
    assert {"partial_device", "partial_device+hist", "norm_device two-pass"} <= names
    ks = sorted(j.k for j in T.JOBS if isinstance(j, T.Kmers))
    assert ks[0] <= 7 and ks[-1] >= 8
    assert T.BY_NAME["fa_index_device"].run.__code__.co_names.count("fa_count_intervals") == 1


def test_every_part_is_compared_and_has_content():
    for job in T.JOBS:
        w = T.wanted(job, 0)
        assert job.primary in job.parts and set(job.parts) <= set(w), job
        assert {name for name, _ in job.outs} <= set(job.parts), job
        for name, size in job.outs:
            assert isinstance(w[name], bytes) and len(w[name]) % size == 0 and len(w[name]) > 0, (job, name)


@pytest.mark.parametrize("job", T.JOBS, ids=repr)
def test_decoys(job):
    for seed in T.WORKER_SEEDS:
        real, decoy = job.make(seed), job.decoy(seed)
        assert [d.size for d in decoy] == [r.size for r in real] and all(r.size > 0 for r in real), (job, seed)
        for r, d in zip(real, decoy):
            assert int((r == 10).sum()) != int((d == 10).sum()) or seed == T.SINGLE and job.kind == "fasta", (job, seed, "the same number of lines")
            assert not np.array_equal(r, d)
        w, v = T.wanted(job, seed), T.wanted(job, seed, decoy=True)
        for part in job.parts:
            assert differs(w[part], v[part]), (job, seed, part, "the decoy's result is the input's")


@pytest.mark.parametrize("job", T.JOBS, ids=repr)
def test_worker_seeds_differ_pairwise(job):
    assert len(T.WORKER_SEEDS) == 12
    for a, b in itertools.combinations(T.WORKER_SEEDS, 2):
        assert differs(T.wanted(job, a)[job.primary], T.wanted(job, b)[job.primary]), (job, a, b)


def test_the_special_seeds_are_special():
    for text in T.fastq(T.SHORT_LINES):
        data = text.tobytes()
        assert data.count(b"\n") + 1 > len(data) // 24 + 1024, "the line index's first guess holds these lines"
    for text in T.fastq(T.CRLF) + T.fasta(T.CRLF):
        data = text.tobytes()
        assert data.count(b"\r\n") == data.count(b"\n") > 100
    for seed in T.WORKER_SEEDS:
        if seed != T.CRLF:
            assert all(13 not in text for text in T.fastq(seed) + T.fasta(seed)), seed
    r1, r2, il = T.fastq(T.SINGLE)
    assert r1.tobytes().count(b"\n") == r2.tobytes().count(b"\n") == 4 and il.tobytes().count(b"\n") == 8
    assert T.wanted(T.BY_NAME["fa_index_device"], T.SINGLE)["summary"]["contigs"] == 1
    assert all(text.size == 0 for text in T.fastq(T.EMPTY) + T.fasta(T.EMPTY))
    for job in T.JOBS:
        if job.accepts_empty:
            T.wanted(job, T.EMPTY)                                   # the checker accepts no input at all
    for seed in T.WORKER_SEEDS:
        if seed not in (T.SHORT_LINES, T.SINGLE):
            assert all(300 <= text.tobytes().count(b"\n") // 4 <= 500 for text in T.fastq(seed)[:2]), seed


FULL = [s for s in T.WORKER_SEEDS if s != T.SINGLE]                  # (one pair cannot hold every case)


def stats(name, seed):
    w = T.wanted(T.BY_NAME[name], seed)
    return w.get("stats") or w.get("summary") or w.get("head")


@pytest.mark.parametrize("seed", FULL)
def test_every_planted_case_occurs(seed):
    for form in ("", " interleaved"):
        s = stats("insert_size_device" + form, seed)
        assert min(s["overlapped"], s["not_overlapped"], s["read_through"]) >= 10, (seed, form, s)
        s = stats("merge_device" + form, seed)
        assert s["merged"] >= 10 and s["not_overlapped"] >= 10, (seed, form, s)
        s = stats("trim_device" + form, seed)
        assert min(s["cut_overlap"], s["cut_adapter"], s["cut_polyg"], s["cut_quality"]) >= 5 and s["reads_out"] > 100, (seed, form, s)
        s = stats("screen_device" + form, seed)
        assert s["matched_reads"] >= 10 and 100 < s["reads_out"] < s["reads_in"], (seed, form, s)
        s = stats("demux_device" + form, seed)
        assert min(s["perfect"], s["mismatched"], s["unmatched"]) >= 5 and s["assigned"] >= 50 and s["undetermined"] >= 50, (seed, form, s)
        rows = T.wanted(T.BY_NAME["demux_device" + form], seed)["rows"]
        assert all(r["units"] > 0 for r in rows), (seed, form, rows)
    for name in ("norm_device", "norm_device interleaved", "norm_device two-pass"):
        s = stats(name, seed)
        assert min(s["dropped_low"], s["dropped_high"], s["units_out"]) >= 10, (seed, name, s)
    s = stats("dedup_device", seed)
    assert s["duplicates"] >= 20 and s["records_out"] >= 200, (seed, s)
    w = T.wanted(T.BY_NAME["adapters_device"], seed)
    assert all(h >= 3 for h in w["hits"][:3]), (seed, w["hits"])
    s = stats("kcount_device", seed)
    assert s["max_count"] >= 8 and s["unique"] > 1000 and s["skipped"] > 0, (seed, s)
    assert T.wanted(T.BY_NAME["count_device"], seed)["counts"]["bad_at"] == 0


def test_the_single_pair_has_work():
    """one pair: it comes from a reference, its mates overlap and merge, and both run through into their adapters"""
    assert stats("merge_device", T.SINGLE)["merged"] == 1
    assert stats("insert_size_device interleaved", T.SINGLE)["overlapped"] == 1
    assert stats("screen_device", T.SINGLE)["matched_reads"] == 2
    assert stats("trim_device", T.SINGLE)["cut_adapter"] + stats("trim_device", T.SINGLE)["cut_overlap"] == 2

"""The stream leases, the scratch pool and the shared handles under twelve host threads: more than the 8 idle streams that
scfq_scratch.hip keeps per device (a ninth concurrent call creates a stream and destroys it afterwards), fewer than the 16 staging
sessions.  Every thread works on ITS OWN inputs (the worker seeds of tests/_caller_cases.py, whose results differ pairwise:
tests/test_caller_cases_host.py), so a result that leaks from one thread's call into another's does not compare equal; every wanted
result comes from the command's checker and is computed before the threads start; every comparison is ==.

Every test runs its schedule once from one thread first, which also gives the time that the hang guard is scaled by: a worker that
is still running after 100 times that (60 s at least) ends the session, since nothing may start on a device after a hang."""
import os
import threading
import time
import traceback

import numpy as np
import pytest

import _caller_cases as T
from conftest import GOLDEN
from _kcount_check import canonical_key, dump_of, hist_of

pytestmark = pytest.mark.gpu

THREADS = 12
ROUNDS = 5


def run_threads(torch, scfq, work, n=THREADS, rounds=1, alone_shares=None):
    """work(i, round): one round of thread i's share.  The shares one after another from this thread (one round of all of them, or of
    the first alone_shares: the time that scales the hang guard), then `n` threads behind a barrier, every one with a stream of its own
    as its wait stream"""
    t0 = time.monotonic()
    for i in range(alone_shares or n):
        work(i, 0)
    torch.cuda.synchronize()
    alone = (time.monotonic() - t0) * rounds * n / (alone_shares or n)
    failures, barrier = [], threading.Barrier(n)

    def worker(i):
        try:
            torch.cuda.set_device(0)
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                scfq.set_wait_stream(stream.cuda_stream)            # (per host thread)
                barrier.wait(60)
                for r in range(rounds):
                    work(i, r)
                stream.synchronize()
        except BaseException as e:      # (an assertion in a thread is otherwise lost)
            failures.append((i, repr(e)[:2000], traceback.format_exc()[-1500:]))

    threads = [threading.Thread(target=worker, args=(i,), daemon=True) for i in range(n)]
    for th in threads:
        th.start()
    deadline = time.monotonic() + max(60.0, 100.0 * alone)
    for th in threads:
        th.join(max(0.0, deadline - time.monotonic()))
    stuck = [i for i, th in enumerate(threads) if th.is_alive()]
    if stuck:
        pytest.exit("threads %s were still running %.0f s after their start (the same work took %.2f s from one thread): a hang; nothing more "
                    "may start on the device" % (stuck, max(60.0, 100.0 * alone), alone), returncode=3)
    assert not failures, failures[:3]


class Inputs:
    """the inputs of one seed in device memory, at a pointer offset of its own"""

    def __init__(self, torch, seed):
        self.seed = seed
        r1, r2, il = T.fastq(seed)
        off = (0, 1, 17, 64, 4095, 33)[seed % 6]
        self.held = dict(r1=T.place(torch, r1, off), r2=T.place(torch, r2, (off + 7) % 4096), il=T.place(torch, il, off), fa=T.place(torch, T.fasta(seed)[0], off))
        self.sizes = dict(r1=r1.size, r2=r2.size, il=il.size, fa=T.fasta(seed)[0].size)

    def ptrs(self, job):
        names = {"single": ("r1",), "pair": ("r1", "r2"), "interleaved": ("il",), "fasta": ("fa",)}[job.kind]
        return [(self.held[n][1], self.sizes[n]) for n in names]


@pytest.fixture(scope="module")
def inputs(gpu):
    return {seed: Inputs(gpu, seed) for seed in T.ALL_SEEDS}


@pytest.fixture(scope="module")
def shared(gpu, scfq):
    """one screen index and one sample sheet for every thread"""
    with scfq.screen_index_files(T.SCREEN_FA) as index, scfq.demux_sheet(list(T.SAMPLES)) as sheet:
        yield dict(index=index, sheet=sheet)


@pytest.fixture(scope="module")
def tables(gpu, scfq):
    """the k-mer table of every worker seed's reads, for fq-normalize against a given table"""
    made = {seed: scfq.kcount_host(*T.fastq(seed)[:2], k=T.K, flags=scfq.SCFQ_KCOUNT_CANONICAL)[1] for seed in T.WORKER_SEEDS}
    yield made
    for t in made.values():
        t.close()


def context_of(job, seed, shared, tables):
    if isinstance(job, T.Screen):
        return shared["index"]
    if isinstance(job, T.Demux):
        return shared["sheet"]
    if isinstance(job, T.Normalize) and not job.two_pass:
        return tables[seed]
    return None


def all_wanted(jobs, seeds):
    for job in jobs:
        for seed in seeds:
            T.wanted(job, seed)


def test_every_command_side_by_side(gpu, scfq, inputs, shared, tables):
    """thread i runs the whole job list, rotated by i, five times on the inputs of seed i"""
    torch = gpu
    all_wanted(T.JOBS, T.WORKER_SEEDS)

    def work(i, r):
        seed = T.WORKER_SEEDS[i]
        for job in T.JOBS[i % len(T.JOBS):] + T.JOBS[:i % len(T.JOBS)]:
            T.call(torch, scfq, job, inputs[seed].ptrs(job), T.wanted(job, seed), context_of(job, seed, shared, tables), (job.name, "thread %d" % i, "round %d" % r))

    before = scfq.lib().scfq_device_bytes_now()
    run_threads(torch, scfq, work, rounds=ROUNDS)
    assert scfq.lib().scfq_device_bytes_now() == before


ONE_COMMAND = ("trim_device", "merge_device", "screen_device", "demux_device", "kcount_device", "norm_device", "norm_device two-pass",
               "kmers_device k=9 canonical", "fa_index_device")


@pytest.mark.parametrize("name", ONE_COMMAND)
def test_one_command_in_every_thread(gpu, scfq, inputs, shared, tables, name):
    """twelve threads, the same command, twelve different inputs.  (fa-gc: the header allows one call at a time per index; every
    thread builds its own and queries it)"""
    torch, job = gpu, T.BY_NAME[name]
    all_wanted([job], T.WORKER_SEEDS)

    def work(i, r):
        seed = T.WORKER_SEEDS[i]
        T.call(torch, scfq, job, inputs[seed].ptrs(job), T.wanted(job, seed), context_of(job, seed, shared, tables), (name, "thread %d" % i, "round %d" % r))

    before = scfq.lib().scfq_device_bytes_now()
    run_threads(torch, scfq, work, rounds=ROUNDS)
    assert scfq.lib().scfq_device_bytes_now() == before


def test_no_input_at_all_from_twelve_threads(gpu, scfq, inputs, shared, tables):
    """every command that accepts an empty input, side by side with the others on the input of seed 0"""
    torch = gpu
    jobs = [j for j in T.JOBS if j.accepts_empty]
    all_wanted(jobs, (0, T.EMPTY))
    tables = dict(tables)
    with scfq.kcount_host(b"", k=T.K, flags=scfq.SCFQ_KCOUNT_CANONICAL)[1] as empty_table:
        tables[T.EMPTY] = empty_table

        def work(i, r):
            seed = T.EMPTY if i % 2 else 0
            for job in jobs[i % len(jobs):] + jobs[:i % len(jobs)]:
                T.call(torch, scfq, job, inputs[seed].ptrs(job), T.wanted(job, seed), context_of(job, seed, shared, tables), (job.name, "thread %d" % i, "seed %d" % seed))

        run_threads(torch, scfq, work)


def test_one_kcount_table_many_readers(gpu, scfq, inputs):
    """hist, dump and query of twelve threads on ONE table share 8 MiB of scratch and a cursor under the table's lock; a table of 2^20
    slots makes dump walk more than one piece of it.  Four more threads run fq-normalize against the same table meanwhile, which reads
    it without that lock"""
    torch = gpu
    norm = T.BY_NAME["norm_device"]
    base = norm.make(0)
    table = T.kcount_table(base).table
    keys = np.array(sorted(table), np.uint64)
    plans = []
    for i in range(THREADS):
        rng = np.random.default_rng(500 + i)
        present = keys[rng.choice(keys.size, 200, replace=False)]
        absent = np.array([v for v in (int(x) & (4 ** T.K - 1) for x in rng.integers(0, 2 ** 62, 150)) if canonical_key(v, T.K) not in table][:100], np.uint64)
        bins, lo = 3 + 5 * i, 1 + i % 4
        hi = 0 if i % 3 == 0 else lo + 2 * i
        plans.append(dict(bins=bins, lo=lo, hi=hi, ask=np.concatenate([present, absent]), hist=hist_of(table, bins),
                          dump=np.array(dump_of(table, lo, hi), np.uint64).reshape(-1, 2).tobytes(), counts=[table[int(v)] for v in present] + [0] * absent.size))
        assert absent.size == 100 and len(plans[-1]["dump"]) > 0
    assert len({p["dump"] for p in plans}) > 6
    norm_seeds = (4, 5, 6, 7)
    norm_want = {seed: norm.wanted(norm.make(seed), base=base) for seed in norm_seeds}
    s, t = scfq.kcount_device(*[x for p in inputs[0].ptrs(norm) for x in p], k=T.K, flags=scfq.SCFQ_KCOUNT_CANONICAL, table_bits=20)
    with t:
        assert int(s.slots) == 1 << 20 and int(s.distinct) == len(table)

        def work(i, r):
            if i >= THREADS:
                seed = norm_seeds[i - THREADS]
                T.call(torch, scfq, norm, inputs[seed].ptrs(norm), norm_want[seed], t, ("normalize against the shared table", "seed %d" % seed, "round %d" % r))
                return
            p = plans[i]
            assert t.hist(p["bins"]).tolist() == p["hist"], ("hist", i, r)
            assert t.dump(p["lo"], p["hi"]).tobytes() == p["dump"], ("dump", i, r)
            assert t.query(p["ask"]).tolist() == p["counts"], ("query", i, r)

        run_threads(torch, scfq, work, n=THREADS + len(norm_seeds), rounds=20)


def test_one_screen_index_and_one_demux_sheet_shared(gpu, scfq, inputs, shared):
    """twelve threads, one index and one sheet, different inputs and options"""
    torch = gpu
    jobs = []
    for i in range(THREADS):
        kind = ("pair", "interleaved")[i % 2]
        jobs.append((T.Screen("screen_device variant %d" % i, kind=kind, opts=dict(min_hits=1 + i % 3, keep_matched=bool(i & 2))),
                     T.Demux("demux_device variant %d" % i, kind=kind, opts=dict(mismatches=i % 3, keep_barcode=bool(i & 4)))))
    want = {(j.name, i): j.wanted(j.make(T.WORKER_SEEDS[i])) for i, pair in enumerate(jobs) for j in pair}
    for k in (0, 1):
        assert len({want[(pair[k].name, i)]["out1"] for i, pair in enumerate(jobs)}) == THREADS

    def work(i, r):
        seed = T.WORKER_SEEDS[i]
        for job, ctx in zip(jobs[i], (shared["index"], shared["sheet"])):
            T.call(torch, scfq, job, inputs[seed].ptrs(job), want[(job.name, i)], ctx, (job.name, "thread %d" % i, "round %d" % r))

    run_threads(torch, scfq, work, rounds=ROUNDS)


def file_calls(scfq, tmp, tag):
    """[(label, call)]: entry points that open and stage their inputs themselves, gzip members and second files included"""
    g = lambda *parts: os.path.join(GOLDEN, *parts)
    kmer_head = T.Kmers.HEAD

    def kmers(path, k, flags):
        s, table = scfq.kmers_file(path, k, flags, True)
        return T.fields_of(s, kmer_head), table.tobytes()

    def trim(p1, p2):
        names = [os.path.join(tmp, "%s_%d.fq" % (tag, j)) for j in (1, 2)]
        fds = [os.open(n, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o600) for n in names]
        try:
            s = scfq.trim_file(p1, p2, scfq.trim_opts(poly_g=5, window_quality=20), *fds)
        finally:
            for fd in fds:
                os.close(fd)
        return T.fields_of(s, T.TRIM_FIELDS, ("adapter_reads",)), [open(n, "rb").read() for n in names]

    def kcount(p1, p2):
        s, t = scfq.kcount_files(p1, p2, k=T.K, flags=scfq.SCFQ_KCOUNT_CANONICAL)
        with t:
            return T.fields_of(s, T.Kcount.HEAD), t.dump(1, 0).tobytes()

    return [("kmers dup.fq.gz", lambda: kmers(g("dup.fq.gz"), 6, 0)),
            ("kmers two_member.fq.gz", lambda: kmers(g("edge", "two_member.fq.gz"), 9, scfq.SCFQ_KMERS_CANONICAL)),
            ("read_stats pairs/r2.fq.gz", lambda: bytes(scfq.read_stats_file(g("pairs", "r2.fq.gz")))),
            ("read_stats two_member.fq.gz", lambda: bytes(scfq.read_stats_file(g("edge", "two_member.fq.gz")))),
            ("read_stats novaseq.fq", lambda: bytes(scfq.read_stats_file(g("novaseq.fq")))),
            ("trim r1.fq r2.fq.gz", lambda: trim(g("trim", "r1.fq"), g("trim", "r2.fq.gz"))),
            ("trim screen r1.fq r2.fq.gz", lambda: trim(g("screen", "r1.fq"), g("screen", "r2.fq.gz"))),
            ("kcount normalize r1.fq r2.fq.gz", lambda: kcount(g("normalize", "r1.fq"), g("normalize", "r2.fq.gz"))),
            ("kcount reads.fq", lambda: kcount(g("kcount", "reads.fq"), None)),
            ("cycles demux/r2.fq.gz", lambda: (lambda r: (bytes(r[0]), r[1].tobytes()))(scfq.cycles_file(g("demux", "r2.fq.gz"), 64)))]


def test_file_entry_points(gpu, scfq, tmp_path):
    """twelve threads run *_file calls on the committed fixtures, so staging sessions overlap; the results are those of the same calls
    made alone.  (scfq_device_bytes_now() is not compared here: a staging session keeps its buffers for the next file, and twelve
    sessions at once hold more than one did)"""
    alone = [call() for _, call in file_calls(scfq, str(tmp_path), "alone")]
    assert all(len(r[1]) > 0 for r in alone if isinstance(r, tuple))
    calls = [file_calls(scfq, str(tmp_path), "t%d" % i) for i in range(THREADS)]

    def work(i, r):
        n = len(alone)
        for k in list(range(i % n, n)) + list(range(i % n)):
            label, call = calls[i][k]
            assert call() == alone[k], (label, "thread %d" % i, "round %d" % r)

    run_threads(gpu, scfq, work, alone_shares=2)

"""The command line of `sc`, invocation by invocation: return code, stdout and stderr of every case below are compared byte for byte with
what the host program printed BEFORE its commands were moved onto one option table (cli/sc_cli.hpp).

The expected triples are data, tests/golden/cli_grammar.json and cli_grammar_gpu.json.  They were recorded from the binary of the commit
before that change, never from the program under test:

    python tests/test_cli_grammar_host.py --record /path/to/that/build/sc           (the cases without a device)
    python tests/test_cli_grammar_host.py --record-gpu /path/to/that/build/sc       (the seven table-driven commands on the device)

Every case runs in tests/golden with relative paths, so the texts hold no path of the machine that recorded them (where --absolute
prints the working directory it is stored as {CWD}).  A usage error prints the command's whole help first: the file stores that as
{HELP}, which stands for the recorded stdout of `sc COMMAND --help`.

None of the host cases reaches the device: they end in the parser, at a file that cannot be opened, or at a header-only run."""
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SC = os.path.join(ROOT, "seq-collection_amd", "sc")
HOST_JSON = os.path.join(GOLDEN, "cli_grammar.json")
GPU_JSON = os.path.join(GOLDEN, "cli_grammar_gpu.json")

R1, R2, IL, ONE = "pairs/r1.fq", "pairs/r2.fq", "pairs/interleaved.fq", "illumina_1.fq"      # relative to tests/golden
TABLE = ("fq-count", "fq-readstats", "fq-cycles", "fq-kmers", "fq-adapters", "fq-insert-size", "fq-merge")     # through parse_options()
OWN_LOOP = ("fq-meta", "fa-gc", "fq-dedup")                                                    # the reference's own grammar
CLUSTER = tuple(c for c in TABLE if c != "fq-merge")                                           # have -t / -b / -a
PAIRED = ("fq-insert-size", "fq-merge")

# (option, digit cap, lowest, highest) of every bounded number
NUMBERS = {
    "fq-cycles": [("max-cycles", 8, 0, 1 << 24)],
    "fq-adapters": [("max-positions", 8, 0, 1 << 24)],
    "fq-kmers": [("k", 18, 1, 12), ("top", 18, 0, 10 ** 18 - 1)],
    "fq-insert-size": [("min-overlap", 6, 1, 512), ("max-mismatches", 6, 0, 65535), ("max-mismatch-pct", 6, 0, 100)],
    "fq-merge": [("min-overlap", 6, 1, 512), ("max-mismatches", 6, 0, 65535), ("max-mismatch-pct", 6, 0, 100), ("phred-offset", 6, 33, 64)],
}


def invocations():
    """the list of the before/after comparison: argument vectors, the command first"""
    out = [[], ["-h"], ["--help"], ["-v"], ["--version"], ["bogus"], ["--bogus"], ["-x"]]
    for cmd in TABLE + OWN_LOOP:
        two = cmd in PAIRED
        out += [[cmd], [cmd, "-h"], [cmd, "--help"], [cmd, "-th"], [cmd, "-hx"], [cmd, "missing.fq", "--help"], [cmd, "--", "-h"]]
        out += [[cmd, "-t"], [cmd, "-tb"], [cmd, "-tba"], [cmd, "-t", "-b", "-a"], [cmd, "--header", "--absolute"], [cmd, "--header", "--basename"]]
        out += [[cmd, "-tx"], [cmd, "-x"], [cmd, "--bogus"], [cmd, "--header=1"], [cmd, "-t=1"], [cmd, "---"], [cmd, "--=x"], [cmd, "-tb", "--bogus"],
                [cmd, "--bogus", "-tx"]]
        out += [[cmd, "--", "--header"], [cmd, "--", "--header", "--bogus"], [cmd, "-t", "--", "-t"], [cmd, "--"], [cmd, "-t", "--"]]
        out += [[cmd, "-"], [cmd, "-", "-"], [cmd, "-t", "-"], [cmd, ""], [cmd, "ab"], [cmd, "ab", "cd"], [cmd, "-tb", "ab"]]
        out += [[cmd, "missing.fq"], [cmd, "missing.fq.gz"], [cmd, "-tba", "missing.fq"], [cmd, "missing.fq", "other.fq"], [cmd, "dir/missing.fq.gz", "x.fq"]]
        out += [[cmd, "--basename"], [cmd, "-b"], [cmd, "--absolute", "--basename"]]
        if two:
            # (fq-insert-size opens its second file with the device session up: SECOND_MISSING below, on the device)
            out += [[cmd, R1, m] for m in ("missing.fq", "missing.fq.gz") if cmd == "fq-merge"]
            out += [[cmd, "missing.fq", R2], [cmd, "missing.fq.gz", R2], [cmd, R1, "ab"],
                    [cmd, "ab", R2], [cmd, "--interleaved", "missing.fq"], [cmd, "--interleaved", "missing.fq.gz"], [cmd, "--interleaved", "ab"],
                    [cmd, "--interleaved"], [cmd, "--interleaved", "--", "--interleaved"], [cmd, "--interleaved=1", "missing.fq"]]
        for name, cap, lo, hi in NUMBERS.get(cmd, []):
            opt = "--" + name
            end = [] if cmd == "fq-merge" else ["-t"]          # accepted values end at the header (fq-merge: at "No FASTQ specified")
            values = ["", "x", "-1", "2.5", "+1", " 1", "1 ", "0x1", str(lo), str(hi), str(hi + 1), str(lo).zfill(cap), str(lo).zfill(cap + 1),
                      str(hi).zfill(cap + 1), "9" * cap, "9" * (cap + 1)]
            if lo > 0:
                values += [str(lo - 1), "0"]
            out += [[cmd, opt + "=" + v] + end for v in values]
            out += [[cmd, opt] + end, [cmd, opt, "5"] + end, [cmd, opt + "=" + str(lo), opt + "=x"], [cmd, opt + "=x", "--bogus"], [cmd, "--bogus", opt + "=x"],
                    [cmd, "--", opt + "=x"]]
    # fq-merge: --phred-offset is 33 or 64 (the second check shows the number), its paths, and which output option goes with which input form
    out += [["fq-merge", "--phred-offset=" + v] for v in ("34", "63", "040", "000064", "0000033", "64", "33")]
    out += [["fq-merge", o + "=" + v] for o in ("--unmerged1", "--unmerged2", "--unmerged") for v in ("", "u.fq")]
    out += [["fq-merge", o] for o in ("--unmerged1", "--unmerged2", "--unmerged", "--stats", "--stats=1")]
    out += [["fq-merge"] + a for a in (["a.fq"], ["a.fq", "b.fq", "c.fq"], ["--interleaved", "a.fq", "b.fq"], ["--interleaved", "--unmerged1=u.fq", "a.fq"],
                                       ["--interleaved", "--unmerged2=u.fq", "a.fq"], ["--unmerged=u.fq", "a.fq", "b.fq"],
                                       ["--unmerged1=u.fq", "--unmerged2=v.fq", "--unmerged=w.fq", "a.fq", "b.fq"], ["--interleaved", "--unmerged=u.fq"],
                                       ["--unmerged1=u.fq", "missing.fq", R2], ["--interleaved", "--unmerged=u.fq", "missing.fq"])]
    # fq-insert-size: FASTQs come in twos
    out += [["fq-insert-size"] + a for a in (["a.fq"], ["a.fq", "b.fq", "c.fq"], ["-t", "a.fq"], ["--interleaved", "a.fq", "b.fq", "c.fq"], ["--dist", "-t"],
                                             ["--dist", "-tb"], ["--dist=1"], ["--dist"])]
    # fq-readstats --hist, fq-kmers, fq-adapters --adapter, fq-cycles
    out += [["fq-readstats", "--hist=" + v, "-t"] for v in ("len", "gc", "qual", "", "foo", "len,gc", "LEN")]
    out += [["fq-readstats", "--hist", "-t"], ["fq-readstats", "--hist", "len", "-t"], ["fq-readstats", "--hist=gc", "-tba"], ["fq-readstats", "--hist=gc"]]
    out += [["fq-kmers"] + a for a in (["--totals", "-t"], ["--totals", "-tba"], ["--canonical", "-t"], ["--canonical", "--totals"], ["--canonical=1"],
                                       ["--k=3", "--top=2", "--totals", "--canonical", "-t"], ["--k=12", "--totals", "missing.fq"])]
    ad = "--adapter="
    out += [["fq-adapters", ad + v, "-t"] for v in ("", "x", "n:", ":ACGT", "n:ACGX", "n:acgt", "a\tb:ACGT", "n:" + "A" * 32, "n:" + "A" * 33, "n:ACGT", "a:b:ACGT",
                                                    "n:AC:GT", "n=1:ACGT")]
    out += [["fq-adapters"] + [ad + "p%d:ACGT" % k for k in range(n)] + ["-t"] for n in (2, 8, 9)]
    out += [["fq-adapters"] + a for a in (["--adapter", "-t"], ["--adapter", "n:ACGT", "-t"], ["--totals", "-t"], ["--totals", "-tba"], ["--counts", "-t"],
                                          [ad + "n:ACGT", "--totals", "-tb"], ["--counts", "--totals"], ["--counts=1"], [ad + "bad", "--bogus"],
                                          ["--bogus", ad + "bad"], [ad + "n:ACGT", "missing.fq"])]
    # fq-count's own options: accepted ones end at the header; the shard options describe no rank without a rendezvous
    for opts in (["--debug"], ["--struct-check"], ["--qual-hist"], ["--stats"], ["--struct-check", "--qual-hist", "--stats"], ["--jobs=3"], ["--jobs=0"],
                 ["--jobs=-1"], ["--jobs=x"], ["--jobs="], ["--devices=0"], ["--devices=0,1"], ["--devices="], ["--devices=x,,1"], ["--transport=tcp"],
                 ["--transport=rccl"], ["--rendezvous=h:1"], ["--rendezvous="]):
        out += [["fq-count"] + opts + ["-t"], ["fq-count"] + opts]
    out += [["fq-count"] + a for a in (["--transport=udp", "-t"], ["--transport=", "-t"], ["--transport", "-t"], ["--transport", "tcp", "-t"], ["--jobs", "-t"],
                                       ["--jobs", "3", "-t"], ["--devices", "-t"], ["--rendezvous", "-t"], ["--shard-rank", "-t"], ["--shard-world", "-t"],
                                       ["--debug=1", "-t"], ["--stats=1", "-t"], ["--shard-rank=0", "-t"], ["--shard-world=2", "-t"],
                                       ["--shard-rank=x", "-t"], ["--shard-world=x", "-t"], ["--shard-rank=0", "--shard-world=2", "-t"],
                                       ["--shard-rank=2", "--shard-world=2", "--rendezvous=h:1", "-t"], ["--shard-rank=0", "--shard-world=1", "--rendezvous=nocolon", "-t"],
                                       ["--shard-rank=-1", "--shard-world=1", "--rendezvous=h:1"], ["--jobs=2", "missing.fq", "other.fq"],
                                       ["--jobs=1", "missing.fq.gz", "other.fq"], ["--stats", "missing.fq"], ["--struct-check", "ab"])]
    # fq-meta's spellings of -n, fa-gc's of --pos and its missing arguments, fq-dedup's one file
    out += [["fq-meta"] + a + ["-t"] for a in (["-n", "5"], ["-n5"], ["-n=5"], ["--lines", "5"], ["--lines=5"], ["-n", "x"], ["-nx"], ["-n="], ["--lines="],
                                               ["--lines=-1"], ["-n", "-1"], ["--whole-file"], ["--whole-file=1"], ["-n", "5", "--bogus"])]
    out += [["fq-meta", "-t", "-n"], ["fq-meta", "-t", "--lines"], ["fq-meta", "-n", "5", "missing.fq"], ["fq-meta", "-tb", "-n5", "missing.fq.gz"],
            ["fq-meta", "--whole-file", "missing.fq"]]
    pos = "chr1:5"
    out += [["fa-gc"] + a for a in (["-p", pos, "missing.fa", "50"], ["-p=" + pos, "missing.fa", "50"], ["--pos=" + pos, "missing.fa", "50"],
                                    ["--pos", pos, "missing.fa", "50"], ["-p" + pos, "missing.fa", "50"], ["missing.fa", "50", "-p", pos], ["-p"], ["--pos"],
                                    ["missing.fa", "-p"], ["-p", pos], ["--pos=" + pos], ["missing.fa"], ["missing.fa", "50"], ["-p", pos, "missing.fa"],
                                    ["--pos=", "missing.fa", "50"], ["-p", pos, "missing.fa", "x"], ["-p", pos, "missing.fa", "-5"],
                                    ["-p", pos, "missing.fa", "50", "x"], ["-p", "chr1:x", "missing.fa", "50"], ["-p", "missing.bed", "missing.fa", "50"],
                                    ["-p", "missing.bcf", "missing.fa", "50"], ["-p", pos, "--", "-p", "50"], ["-p", pos, "missing.fa.gz", "50"])]
    out += [["fq-dedup"] + a for a in (["STDIN"], ["a.fq", "b.fq"], ["-h", "a.fq"], ["a.fq", "--help"], ["pairs"], ["--", "missing.fq"])]
    seen, unique = set(), []
    for a in out:
        if tuple(a) not in seen:
            seen.add(tuple(a))
            unique.append(a)
    return unique


def gpu_invocations():
    """the seven table-driven commands on the smallest fixtures: (command, spelling one, spelling two); both print the same"""
    return [
        ("fq-count", ["-tba", "--", ONE], ["--header", "--basename", "--absolute", "--", ONE]),
        ("fq-count", ["-tb", "--struct-check", "--qual-hist", "--jobs=1", "--", ONE, IL], ["--qual-hist", "--header", "--struct-check", "--basename", "--jobs=1", "--", ONE, IL]),
        ("fq-readstats", ["-tba", "--", ONE], ["--header", "--basename", "--absolute", "--", ONE]),
        ("fq-readstats", ["-bt", "--hist=len", "--", ONE], ["--hist=len", "--basename", "--header", "--", ONE]),
        ("fq-cycles", ["-tb", "--max-cycles=5", "--", ONE], ["--max-cycles=5", "--header", "--basename", "--", ONE]),
        ("fq-kmers", ["-tb", "--k=3", "--top=4", "--canonical", "--", ONE], ["--canonical", "--top=4", "--k=3", "--header", "--basename", "--", ONE]),
        ("fq-kmers", ["-t", "--totals", "--", ONE], ["--totals", "--header", "--", ONE]),
        ("fq-adapters", ["-tb", "--max-positions=4", "--counts", "--adapter=x:AGATCGG", "--adapter=g:GGG", "--", ONE],
         ["--adapter=x:AGATCGG", "--adapter=g:GGG", "--counts", "--max-positions=4", "--header", "--basename", "--", ONE]),
        ("fq-adapters", ["-t", "--totals", "--", ONE], ["--header", "--totals", "--", ONE]),
        ("fq-insert-size", ["-tb", "--min-overlap=20", "--max-mismatches=3", "--max-mismatch-pct=10", "--", R1, R2],
         ["--max-mismatch-pct=10", "--max-mismatches=3", "--min-overlap=20", "--header", "--basename", "--", R1, R2]),
        ("fq-insert-size", ["-ta", "--interleaved", "--", IL], ["--interleaved", "--header", "--absolute", "--", IL]),
        # (fq-merge has no short options: its two spellings differ in the order of the options)
        ("fq-merge", ["--stats", "--min-overlap=20", "--phred-offset=33", "--", R1, R2], ["--phred-offset=33", "--min-overlap=20", "--stats", "--", R1, R2]),
        ("fq-merge", ["--interleaved", "--stats", "--", IL], ["--stats", "--interleaved", "--", IL]),
    ]


# the second of two paths missing: fq-insert-size names it like fq-merge does, with the exit code of the suffix
SECOND_MISSING = (["fq-insert-size", R1, "missing.fq"], ["fq-insert-size", R1, "missing.fq.gz"])
STATS_CASE = ("fq-count", ["-tb", "--stats", "--jobs=1", "--", ONE, IL], ["--stats", "--header", "--basename", "--jobs=1", "--", ONE, IL])


def run(sc, args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "SC_GPU_CHUNK", "SC_CLEAN_EXIT")}
    r = subprocess.run([os.path.abspath(sc)] + list(args), cwd=GOLDEN, capture_output=True, stdin=subprocess.DEVNULL, env=env)
    out, err = (t.decode("utf-8").replace(GOLDEN, "{CWD}") for t in (r.stdout, r.stderr))
    return r.returncode, out, err


def run_all(sc, cases):
    with ThreadPoolExecutor(8) as pool:
        return list(pool.map(lambda a: run(sc, a), cases))


def help_of(results, cmd):
    return results[json.dumps([cmd, "--help"] if cmd else ["--help"])][1]


def expand(results, args, triple):
    rc, out, err = triple
    return rc, out.replace("{HELP}", help_of(results, args[0] if args and args[0] in TABLE + OWN_LOOP else "")), err


def record(sc, path, cases):
    got = dict(zip((json.dumps(a) for a in cases), run_all(sc, cases)))
    lines = []
    for a in cases:
        rc, out, err = got[json.dumps(a)]
        h = help_of(got, a[0] if a and a[0] in TABLE + OWN_LOOP else "")
        if a[-1:] != ["--help"] and out.startswith(h):
            out = "{HELP}" + out[len(h):]
        assert "HIP" not in err and "hip" not in err, (a, err)          # a host case must not reach the device
        lines.append(json.dumps({"args": a, "rc": rc, "out": out, "err": err}))
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(lines) + "\n]\n")


def load(path):
    with open(path) as f:
        return {json.dumps(c["args"]): (c["rc"], c["out"], c["err"]) for c in json.load(f)}


@pytest.fixture(scope="module")
def recorded():
    return load(HOST_JSON)


@pytest.fixture(scope="module")
def now():
    cases = invocations()
    return dict(zip((json.dumps(a) for a in cases), run_all(SC, cases)))


def test_the_list_is_the_recorded_one(recorded):
    cases = invocations()
    assert [json.dumps(a) for a in cases] == list(recorded), "record again from the earlier binary (see the module's docstring)"
    assert len(cases) > 700
    for cmd in TABLE + OWN_LOOP:
        assert sum(1 for a in cases if a and a[0] == cmd) >= 40, cmd


@pytest.mark.parametrize("cmd", ("",) + TABLE + OWN_LOOP)
def test_every_invocation_answers_as_before(recorded, now, cmd):
    checked = 0
    for a in invocations():
        if (a[0] if a and a[0] in TABLE + OWN_LOOP else "") != cmd:
            continue
        key = json.dumps(a)
        assert now[key] == expand(recorded, a, recorded[key]), a
        checked += 1
    assert checked >= 8


def test_commands_that_must_answer_alike(now):
    """what the shared parser keeps equal, asserted directly: the same stderr and return code but for the names"""
    def got(*a):
        return now[json.dumps(list(a))]

    base = got("fq-cycles", "--bogus")
    assert base[0] == 1 and base[2] == "\x1b[31mError 1: Error: Unknown option: --bogus\x1b[0m\n"
    for cmd in TABLE:
        assert (got(cmd, "--bogus")[0], got(cmd, "--bogus")[2]) == (base[0], base[2]), cmd
        assert got(cmd, "--bogus")[1] == got(cmd, "--help")[1] == got(cmd)[1] == got(cmd, "-h")[1], cmd          # the help comes first, on stdout
        assert got(cmd, "--header=1")[2] == base[2].replace("--bogus", "--header=1"), cmd
        assert got(cmd, "--", "--header")[2] == got("fq-cycles", "--", "--header")[2] or cmd in PAIRED, cmd
        assert got(cmd, "--stats" if cmd == "fq-merge" else "--basename") == (3, "", "\x1b[31mError 3: No FASTQ specified\x1b[0m\n"), cmd
    for cmd in CLUSTER:
        assert got(cmd, "-tx") == (1, got(cmd, "--help")[1], "\x1b[31mError 1: Error: Unknown option: -x\x1b[0m\n"), cmd
        assert got(cmd, "-th") == (0, got(cmd, "--help")[1], ""), cmd
        assert got(cmd, "-tb")[1].endswith("\tbasename\n") and got(cmd, "-tba")[1].endswith("\tbasename\tabsolute\n"), cmd
        assert got(cmd, "-tba")[1] == got(cmd, "-t", "-b", "-a")[1] and got(cmd, "-tb")[1] == got(cmd, "--header", "--basename")[1], cmd
        if cmd not in PAIRED:
            for args in (["missing.fq"], ["missing.fq.gz"], ["ab"], ["-"], ["--", "--header"]):
                assert got(cmd, *args) == got("fq-cycles", *args), (cmd, args)
    assert got("fq-merge", "-tx")[2] == base[2].replace("--bogus", "-tx") and got("fq-merge", "-x")[2] == base[2].replace("--bogus", "-x")
    for a, b in (("missing.fq", R2), ("missing.fq.gz", R2), ("--interleaved", "missing.fq"), ("--interleaved", "missing.fq.gz"), (R1, "ab"), ("ab", R2)):
        assert got("fq-merge", a, b) == got("fq-insert-size", a, b), (a, b)
    for a, b in ((R1, "missing.fq"), ("missing.fq", R2), (R1, "missing.fq.gz"), ("missing.fq.gz", R2), ("--interleaved", "missing.fq")):
        assert got("fq-merge", a, b) == got("fq-cycles", a if a.startswith("missing") else b), (a, b)
    # a bad value reads the same whichever command and option it was given to
    bad = got("fq-cycles", "--max-cycles=x", "-t")
    assert (bad[0], bad[2]) == (1, "\x1b[31mError 1: Error: Bad value for --max-cycles: x\x1b[0m\n")
    for cmd, rows in NUMBERS.items():
        end = [] if cmd == "fq-merge" else ["-t"]
        for name, cap, lo, hi in rows:
            opt = "--" + name
            for v in ("x", "", "-1", "2.5", str(hi + 1), str(lo).zfill(cap + 1)):
                r = got(cmd, opt + "=" + v, *end)
                assert (r[0], r[1], r[2]) == (1, got(cmd, "--help")[1], bad[2].replace("--max-cycles: x", opt + ": " + v)), (cmd, opt, v)
            for v in (str(lo), str(hi), str(lo).zfill(cap)):
                assert got(cmd, opt + "=" + v, *end)[0] == (3 if cmd == "fq-merge" else 0), (cmd, opt, v)
            assert got(cmd, opt, *end)[2] == base[2].replace("--bogus", opt), (cmd, opt)
    assert got("fq-merge", "--phred-offset=040")[2] == bad[2].replace("--max-cycles: x", "--phred-offset: 40")
    assert got("fq-adapters", "--adapter=n:ACGX", "-t")[2] == bad[2].replace("--max-cycles: x", "--adapter: n:ACGX")
    assert got("fq-merge", "--unmerged1=")[2] == bad[2].replace("--max-cycles: x", "--unmerged1: ")
    assert got("fq-readstats", "--hist=foo", "-t")[2] == base[2].replace("--bogus", "--hist=foo")
    assert got("fq-count", "--transport=udp", "-t")[2] == base[2].replace("--bogus", "--transport=udp")


def record_gpu(sc, path):
    lines = []
    for cmd, one, two in gpu_invocations():
        for args in (one, two):
            rc, out, err = run(sc, [cmd] + args)
            lines.append(json.dumps({"args": [cmd] + args, "rc": rc, "out": out, "err": err}))
    for args in SECOND_MISSING:
        rc, out, err = run(sc, args)
        lines.append(json.dumps({"args": args, "rc": rc, "out": out, "err": err}))
    for args in STATS_CASE[1:]:
        rc, out, err = run(sc, [STATS_CASE[0]] + args)
        lines.append(json.dumps({"args": [STATS_CASE[0]] + args, "rc": rc, "out": out, "err": ""}))          # (its stderr holds timings)
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(lines) + "\n]\n")


@pytest.mark.gpu
def test_table_driven_commands_on_the_device(gpu):
    """each of the seven commands once per spelling on the smallest fixtures: both spellings print the same, and what the earlier
    binary printed for the same arguments"""
    recorded = load(GPU_JSON)
    seen = set()
    for cmd, one, two in gpu_invocations():
        a, b = run(SC, [cmd] + one), run(SC, [cmd] + two)
        assert a == b, (cmd, one, two)
        assert a[0] == 0 and a[1], (cmd, a)
        assert a == recorded[json.dumps([cmd] + one)] == recorded[json.dumps([cmd] + two)], (cmd, one)
        seen.add(cmd)
    assert seen == set(TABLE)
    host = load(HOST_JSON)
    for args in SECOND_MISSING:
        assert run(SC, args) == recorded[json.dumps(args)] == host[json.dumps(["fq-merge"] + args[1:])], args
    # --stats: the rows as before; stderr is one line of JSON per file (its timings differ from run to run)
    cmd, one, two = STATS_CASE
    a, b = run(SC, [cmd] + one), run(SC, [cmd] + two)
    assert (a[0], a[1]) == (b[0], b[1]) == recorded[json.dumps([cmd] + one)][:2] == recorded[json.dumps([cmd] + two)][:2] and a[0] == 0
    for r in (a, b):
        rows = [json.loads(line) for line in r[2].splitlines()]
        assert [row["file"] for row in rows] == [ONE, IL] and all(row["input_bytes"] > 0 and isinstance(row["stages_ms"], list) for row in rows)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--record":
        record(sys.argv[2], HOST_JSON, invocations())
    elif len(sys.argv) == 3 and sys.argv[1] == "--record-gpu":
        record_gpu(sys.argv[2], os.environ.get("SC_RECORD_TO", GPU_JSON))
    else:
        sys.exit(__doc__)

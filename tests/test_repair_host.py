"""fq-repair without a device: the checker (_repair_check.py) against an all-pairs statement of the matching rule and against hand-worked
cases, the fixture against its generator, the ABI (symbols, struct layout, C99 header), the formatters, the argument checks, the grammar
of `sc fq-repair`, and what the caller-case inputs of tests/_repair_cases.py hold for tests/test_gpu_repair_callers.py."""
import ctypes
import gzip
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import _caller_cases as T
from conftest import GOLDEN, PKG, ROOT
from _repair_cases import JOB
from _repair_check import (FIELDS, HASH_FIELDS, OUTPUTS, REC_HEADER, REPORT_FIELDS, SINGLE, STATS_HEADER, STATS_WORDS, check_identities, mates_by_pairs,
                           mates_of, name_of, per_read_text, rec_text, repair_of, stats_text)

SC = os.path.join(PKG, "sc")
REPAIR = os.path.join(GOLDEN, "repair")
NEW = ("scfq_repair_buffers", "scfq_repair_files", "scfq_format_repair_stats_tsv", "scfq_format_repair_rec_tsv", "scfq_repair_error_detail")


def run(*args):
    return subprocess.run([SC] + list(args), capture_output=True, text=True, stdin=subprocess.DEVNULL)


def load_generator():
    spec = importlib.util.spec_from_file_location("make_repair", os.path.join(REPAIR, "make_repair.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def fq(headers):
    return b"".join(b"@%s\nACGT\n+\nIIII\n" % h for h in headers)


# ---- the checker ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(3))
def test_the_dictionary_agrees_with_all_pairs(seed):
    """200 random records a side over the alphabet ab with names of 0 .. 3 bytes: repeats abound"""
    rng = np.random.default_rng([20261101, seed])
    names = [[bytes(rng.choice(np.frombuffer(b"ab", np.uint8), int(rng.integers(0, 4))).tobytes()) for _ in range(200 - 7 * side)] for side in (0, 1)]
    a, b = mates_of(*names), mates_by_pairs(*names)
    assert a == b and len(a) == 393
    pairs = sum(1 for m in a[:200] if m != SINGLE)
    assert 100 < pairs < 193 and len(set(names[0])) <= 15 and any(m not in (SINGLE, i) for i, m in enumerate(a[:200]))
    # the whole restatement on the same records: the table is this one
    w = repair_of(fq(names[0]), fq([n + b"\tx" for n in names[1]]))
    assert w["table"] == a and w["pairs"] == pairs and w["repeated1"] == 200 - len(set(names[0]))
    check_identities(w)


def test_hand_computed_anchors():
    # the name rule: the first byte goes whatever it is, the cut is exclusive, one suffix goes, once
    for header, name in ((b"", b""), (b"@", b""), (b"@/1", b""), (b"@a/1/2", b"a/1"), (b"@a /1", b"a"), (b"@a\tb", b"a"), (b"name", b"ame"), (b"@a/3", b"a/3"),
                         (b"@/2 x", b""), (b"@ab/1 c/2", b"ab"), (b"@ a", b""), (b"@a/1\t/2", b"a"), (b"@1", b"1"), (b"@/", b"/"), (b">x/2", b"x"),
                         (b"@a b\tc", b"a"), (b"@a\tb c", b"a"), (b"@//1", b"/")):
        assert name_of(header) == name, header
    # the plain join; comments differ, one record a side finds no mate
    w = repair_of(fq([b"a 1:N", b"b 1:N", b"c 1:N"]), fq([b"c 2:N", b"a 2:N", b"d 2:N"]))
    assert w["table"] == [1, SINGLE, 0, 2, 0, SINGLE] and (w["pairs"], w["singles1"], w["singles2"], w["moved"], w["in_step"]) == (2, 1, 1, 2, 0)
    assert w["out1"] == fq([b"a 1:N", b"c 1:N"]) and w["out2"] == fq([b"a 2:N", b"c 2:N"])
    assert w["singles1_out"] == fq([b"b 1:N"]) and w["singles2_out"] == fq([b"d 2:N"])
    # repeated names: the r-th with the r-th; what is beyond the other input's count is single
    w = repair_of(fq([b"x/1", b"y/1", b"x/1", b"x/1"]), fq([b"x/2", b"x/2", b"y/2"]))
    assert w["table"] == [0, 2, 1, SINGLE, 0, 2, 1] and (w["repeated1"], w["repeated2"], w["moved"]) == (2, 1, 2)
    # in step, repeats and empty names included: the input maps onto itself
    same = [b"q/1", b"", b"q/1", b" c", b"/1"]
    w = repair_of(fq(same), fq(same))
    assert w["table"] == list(range(5)) * 2 and w["in_step"] == 1 and w["repeated1"] == 3 and w["singles1_bytes"] == 0
    # CR LF and a last record without newline: the names are the texts', the echo has '\n' alone; a cut record has the lines it has
    w = repair_of(b"@a/1\r\nAC\r\n+\r\nII\r\n@b/1\r\nAC\r\n+\r\nII", b"@b")
    assert w["table"] == [SINGLE, 0, 1] and w["out1"] == b"@b/1\nAC\n+\nII\n" and w["out2"] == b"@b\n" and w["lines2"] == 1 and w["reads2"] == 1
    # a blank line is a record's header: the empty name
    assert repair_of(b"\n", b"@\n")["pairs"] == 1
    w = repair_of(b"", b"")
    assert (w["reads1"], w["pairs"], w["in_step"], w["table"]) == (0, 0, 1, [])
    w = repair_of(fq([b"a"]), b"")
    assert (w["pairs"], w["singles1"], w["in_step"], w["table"]) == (0, 1, 0, [SINGLE])


# ---- the fixture ------------------------------------------------------------------------------------------------------------
def test_fixture_is_what_its_generator_writes():
    m = load_generator()
    files, w = m.make_files()
    assert sorted(files) == sorted(n for n in os.listdir(REPAIR) if not n.endswith(".py") and n != "__pycache__")
    for name, data in files.items():
        have = open(os.path.join(REPAIR, name), "rb").read()
        if name.endswith(".gz"):       # (the compressed bytes are zlib's business)
            have, data = gzip.decompress(have), gzip.decompress(data)
        assert have == data, name
        assert len(have) < 1 << 20
    check_identities(w)


def test_fixture_holds_what_it_plants():
    m = load_generator()
    files, w = m.make_files()
    r1, r2 = files["r1.fq"], files["r2.fq"]
    assert not r1.endswith(b"\n") and not r2.endswith(b"\n") and b"\r" not in r1 + r2
    in1 = [p for p in range(m.FRAGMENTS) if m.in_r1(p)]
    assert 140 <= w["reads1"] == len(in1) <= 160 and 140 <= w["reads2"] <= 160 and w["in_step"] == 0
    # dropped records: their mates are the singles
    only1 = [p for p in in1 if not m.in_r2(p)]
    only2 = [p for p in range(m.FRAGMENTS) if m.in_r2(p) and not m.in_r1(p)]
    assert only1 and only2 and w["singles1"] == len(only1) and w["singles2"] == len(only2) and m.REPEATED[2] in only1
    for p in only1:
        assert w["table"][in1.index(p)] == SINGLE, p
    # the shuffled block: in R1's order in out2, though R2 holds it in another
    block = [b"@frag%d " % p for p in m.BLOCK if m.in_r1(p) and m.in_r2(p) and p % 10 != 1]
    at1, at2, out2 = [r1.index(h) for h in block], [r2.index(h) for h in block], [w["out2"].index(h) for h in block]
    assert at1 == sorted(at1) and at2 != sorted(at2) and out2 == sorted(out2)
    # suffixes, differing comments, the tab, the name that is only a suffix, the repeated name
    assert b"@frag11/1\n" in r1 and b"@frag11/2\n" in w["out2"] and b"@frag0 1:N:0:ACGT\n" in w["out1"] and b"@frag0 2:N:0:ACGT\n" in w["out2"]
    assert b"@frag%d\tlane=3\n" % m.TAB in w["out1"] and b"@/1\n" in w["out1"] and b"@/2\n" in w["out2"]
    assert r1.count(b"@twice ") == 3 and r2.count(b"@twice ") == 2 and w["out1"].count(b"@twice ") == 2 and w["singles1_out"].count(b"@twice ") == 1
    assert (w["repeated1"], w["repeated2"]) == (2, 1)
    assert w["out1"].count(b"\n") == w["out2"].count(b"\n") == 4 * w["pairs"] and w["moved"] > 0
    assert files["report.tsv"].decode() == STATS_HEADER + "\n" + stats_text(w) + "\n" and files["per_read.tsv"].decode() == per_read_text(w, header=True)


# ---- the ABI ----------------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_listed(scfq):
    header = open(os.path.join(ROOT, "include", "sc_fqcount.h")).read()
    debug = open(os.path.join(ROOT, "include", "sc_fqcount_debug.h")).read()
    L = scfq.lib()
    for name in NEW:
        assert name + "(" in header and name in scfq.EXPORTS and hasattr(L, name), name
    assert "scfq_debug_repair_stages(" in debug and "scfq_debug_repair_stages" in scfq.EXPORTS and len(scfq.repair_stages()) == 9
    assert scfq.SCFQ_REPAIR_SINGLE == SINGLE and scfq.REPAIR_OUTPUTS == OUTPUTS
    for name in ("RepairOpts", "RepairStats", "repair_opts", "repair_resident", "repair_host", "repair_files", "format_repair_stats_tsv", "format_repair_rec_tsv"):
        assert hasattr(scfq, name), name
    assert not hasattr(scfq, "repair_device")


def test_struct_layout(scfq, tmp_path):
    S = scfq.RepairStats
    names = tuple(f[0] for f in S._fields_)
    assert names == scfq.REPAIR_STATS_FIELDS and len(names) == STATS_WORDS and set(FIELDS) | set(HASH_FIELDS) | {"struct_size", "abi_version"} == set(names)
    for i, name in enumerate(names):
        assert getattr(S, name).offset == 8 * i and getattr(S, name).size == 8, name
    assert ctypes.sizeof(S) == 8 * STATS_WORDS and ctypes.sizeof(scfq.RepairOpts) == 32
    src = tmp_path / "t.c"
    offsets = " && ".join("offsetof(scfq_repair_stats, %s) == %d" % (name, 8 * i) for i, name in enumerate(names))
    src.write_text('#include <stddef.h>\n#include "sc_fqcount.h"\n#include "sc_fqcount_debug.h"\n'
                   "typedef char sizes[sizeof(scfq_repair_stats) == 192 && sizeof(scfq_repair_opts) == 32 ? 1 : -1];\n"
                   "typedef char at[" + offsets + " ? 1 : -1];\n"
                   "typedef char consts[SCFQ_REPAIR_SINGLE == 0xFFFFFFFFu && offsetof(scfq_repair_opts, flags) == 8 && offsetof(scfq_repair_opts, hash_bits) == 12\n"
                   "                    && offsetof(scfq_repair_opts, reserved) == 16 ? 1 : -1];\n"
                   "int main(void){ scfq_repair_stats s; scfq_repair_opts o; uint32_t t[2]; double ms[9]; char b[8];\n"
                   "  s.struct_size = sizeof s; o.struct_size = sizeof o;\n"
                   "  return scfq_repair_buffers(0, 0, 0, 0, 0, &o, t, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, &s) + scfq_repair_files(\"x\", \"y\", &o, 0, -1, -1, -1, -1, -1, &s)\n"
                   "         + scfq_format_repair_stats_tsv(&s, 0, b, 8) + scfq_format_repair_rec_tsv(1, 0, t[0], b, 8) + scfq_debug_repair_stages(ms, 9)\n"
                   "         + (scfq_repair_error_detail() != 0) == 12345; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)])


def test_formatters(scfq):
    assert scfq.format_repair_stats_tsv(None, header=True) == STATS_HEADER
    s = scfq.RepairStats()
    s.struct_size = ctypes.sizeof(s)
    w = {name: 1000 + 7 * i for i, name in enumerate(REPORT_FIELDS)}
    for k, v in w.items():
        setattr(s, k, v)
    assert scfq.format_repair_stats_tsv(s) == stats_text(w)
    s.pairs = w["pairs"] = 2 ** 64 - 1
    assert scfq.format_repair_stats_tsv(s) == stats_text(w)
    assert scfq.format_repair_rec_tsv(0) == REC_HEADER == "input\trecord\tmate"
    for which, record, mate in ((1, 0, 0), (2, 2 ** 31 - 1, 2 ** 31 - 2), (1, 5, SINGLE), (2, 9, SINGLE), (2, 2 ** 40, 7)):
        assert scfq.format_repair_rec_tsv(which, record, mate) == rec_text(which, record, mate)
    assert scfq.format_repair_rec_tsv(1, 5) == "1\t5\t-"
    L = scfq.lib()
    assert L.scfq_format_repair_rec_tsv(2, 7, 12, None, 0) == len("2\t7\t12")
    small = ctypes.create_string_buffer(b"#" * 8, 8)
    assert L.scfq_format_repair_rec_tsv(2, 7, 12, small, 5) == 6 and small.raw == b"2\t7\t\0###"
    assert L.scfq_format_repair_stats_tsv(None, 0, None, 0) == scfq.SCFQ_EARG
    w = repair_of(fq([b"a", b"b"]), fq([b"b"]))
    assert per_read_text(w, header=True) == "input\trecord\tmate\n1\t0\t-\n1\t1\t0\n2\t0\t1\n"


def test_argument_checks_come_before_the_device(scfq):
    """none of these needs a device: without one, a call that got past the checks returns SCFQ_EHIP"""
    L = scfq.lib()
    detail = L.scfq_repair_error_detail
    fastq = b"@h/1\nACGTACGTAAAAAAAAAA\n+\nIIIIIIIIIIIIIIIIII\n"
    buf = ctypes.create_string_buffer(fastq)

    def call(opts=None, r2=buf, n2=len(fastq), stats_size=None, table_cap=0, caps=(0, 0, 0, 0), r1=buf):
        s = scfq.RepairStats()
        s.struct_size = ctypes.sizeof(s) if stats_size is None else stats_size
        outs = []
        for c in caps:
            outs += [None, c]
        return L.scfq_repair_buffers(r1, len(fastq), r2, n2, 0, ctypes.byref(opts) if opts is not None else None, None, table_cap, *outs, 0, ctypes.byref(s))

    for kw, text in ((dict(flags=1), b"unknown flag bits 0x1"), (dict(flags=0x80000000), b"unknown flag bits 0x80000000"), (dict(hash_bits=65), b"hash_bits 65"),
                     (dict(reserved=(0, 0, 7, 0)), b"reserved"), (dict(reserved=(0, 0, 0, 1)), b"reserved")):
        assert call(scfq.repair_opts(**kw)) == scfq.SCFQ_EARG and text in detail(), (kw, detail())
    # without text: sizes that are not the structs', a capacity or a size without memory
    assert call(stats_size=184) == scfq.SCFQ_EARG and detail() == b""
    bad = scfq.repair_opts()
    bad.struct_size = 40
    assert call(bad) == scfq.SCFQ_EARG and detail() == b""
    assert call(table_cap=4) == scfq.SCFQ_EARG and detail() == b""
    for k in range(4):
        assert call(caps=tuple(4 if j == k else 0 for j in range(4))) == scfq.SCFQ_EARG and detail() == b""
    assert call(r2=None) == scfq.SCFQ_EARG and call(r1=None) == scfq.SCFQ_EARG and detail() == b""
    s = scfq.RepairStats()
    s.struct_size = ctypes.sizeof(s)
    assert L.scfq_repair_files(b"x.fq", None, None, None, -1, -1, -1, -1, -1, ctypes.byref(s)) == scfq.SCFQ_EARG and b"two files" in detail()
    assert L.scfq_repair_files(None, b"x.fq", None, None, -1, -1, -1, -1, -1, ctypes.byref(s)) == scfq.SCFQ_EARG
    o = scfq.repair_opts(flags=2)
    assert L.scfq_repair_files(b"x.fq", b"y.fq", ctypes.byref(o), None, -1, -1, -1, -1, -1, ctypes.byref(s)) == scfq.SCFQ_EARG and b"flag bits" in detail()
    assert L.scfq_repair_files(b"x.fq", b"y.fq", None, None, -1, -1, -1, -1, -1, None) == scfq.SCFQ_EARG
    import torch
    if not torch.cuda.is_available():
        for opts in (None, scfq.repair_opts(hash_bits=64), scfq.repair_opts(hash_bits=1)):
            with pytest.raises(scfq.ScfqError) as e:
                scfq.repair_host(fastq, fastq, opts=opts)
            assert e.value.rc == scfq.SCFQ_EHIP


# ---- the command ------------------------------------------------------------------------------------------------------------
def test_cli_without_a_device(tmp_path):
    r = run("fq-repair", "--help")
    assert r.returncode == 0 and r.stderr == "" and "fq-repair [options] --out1=PATH --out2=PATH [--singles1=PATH] [--singles2=PATH] R1.fq R2.fq" in r.stdout
    for opt in ("--check", "--per-read=PATH", "--out1=PATH", "--out2=PATH", "--singles1=PATH", "--singles2=PATH", "-t, --header", "-b, --basename", "-a, --absolute",
                "-h, --help"):
        assert opt in r.stdout, opt
    assert run("fq-repair").stdout == r.stdout and run("fq-repair", "-h").stdout == r.stdout
    assert "fq-repair" not in run("--help").stdout                                           # listed in its own help only
    r1, r2 = os.path.join(REPAIR, "r1.fq"), os.path.join(REPAIR, "r2.fq")
    r = run("fq-repair", "does_not_exist.fq", r2)
    assert (r.returncode, r.stderr, r.stdout) == (2, "\x1b[31mError 2: Unable to open file: does_not_exist.fq\x1b[0m\n", "")
    r = run("fq-repair", r1, "does_not_exist.fq")
    assert (r.returncode, r.stderr, r.stdout) == (2, "\x1b[31mError 2: Unable to open file: does_not_exist.fq\x1b[0m\n", "")
    r = run("fq-repair", "-t")
    assert (r.returncode, r.stderr) == (3, "\x1b[31mError 3: No FASTQ specified\x1b[0m\n")
    usage = ["--bogus", "--check=1", "--out1=", "--per-read=", "--hash-bits=8", "--out=x.fq", "--singles1="]
    forms = [(r1,), (r1, r2, r1), (r1, r2, "--out1=x.fq"), (r1, r2, "--out2=y.fq"), (r1, r2, "--check", "--out1=x.fq", "--out2=y.fq"),
             (r1, r2, "--check", "--singles1=x.fq"), (r1, r2, "--check", "--singles2=x.fq")]
    for bad in [(u, r1, r2) for u in usage] + forms:
        r = subprocess.run([SC, "fq-repair"] + list(bad), capture_output=True, text=True, stdin=subprocess.DEVNULL, cwd=str(tmp_path))
        assert r.returncode == 1 and "Error" in r.stderr and "Usage:" in r.stdout, bad
    # an input that cannot be read is found before an output is made
    r = subprocess.run([SC, "fq-repair", "--out1=x.fq", "--out2=y.fq", r1, "none.fq"], capture_output=True, text=True, stdin=subprocess.DEVNULL, cwd=str(tmp_path))
    assert r.returncode == 2
    assert os.listdir(str(tmp_path)) == []


# ---- the caller cases -------------------------------------------------------------------------------------------------------
def test_caller_case_inputs_are_out_of_step():
    """every worker seed but the single-pair one has pairs that moved and singles on both sides; a decoy has the byte lengths of the real
    input, file by file, and differs from it in every part that is compared"""
    for seed in T.WORKER_SEEDS:
        real, decoy = JOB.make(seed), JOB.make(seed, True)
        assert [a.size for a in real] == [a.size for a in decoy] == [a.size for a in T.fastq(seed)[:2]]
        w, other = JOB.wanted(real), JOB.wanted(decoy)
        assert all(w[p] != other[p] for p in JOB.parts), (seed, [p for p in JOB.parts if w[p] == other[p]])
        s = w["stats"]
        if seed == T.SINGLE:
            assert (s["reads1"], s["pairs"], s["in_step"]) == (1, 1, 1)
        else:
            assert s["in_step"] == 0 and 0 < s["singles1"] == s["singles2"] < s["reads1"] // 4 and s["moved"] == s["pairs"] > 0 and s["repeated1"] > 0, (seed, s)
        assert set(name for name, _ in JOB.outs) == {"table"} | set(OUTPUTS) and set(JOB.parts) <= set(w)

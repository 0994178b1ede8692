"""CPU checks of the duplicate-marking surface (dcn_anchor_map_duplicates_enable / _reset / _info, dcn_mark_duplicates_batch):
declared, exported and bound at ABI 1.20, the layout of the parameters in ctypes and C99, the definition stated once, the
argument errors that are found before a device is looked at, in their order, `deacon-hip markdup`'s usage errors and its
--help, the end and key rule of csrc/dcn_duplicates.h compiled for the host under the sanitizers, and the model of the GPU
tests (tests/_duplicates_worker.py) alone on cases whose answers are written out here."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _duplicates_worker as DW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "deacon-server_amd", "bin", "deacon-hip")
NAMES = ["dcn_anchor_map_duplicates_enable", "dcn_anchor_map_duplicates_reset", "dcn_anchor_map_duplicates_info", "dcn_mark_duplicates_batch"]


def test_symbols_are_declared_exported_and_bound(dcn):
    N = dcn._native
    L = C.CDLL(N.LIB_PATH)
    for name, n_args in zip(NAMES, (2, 1, 4, 10)):
        assert name in N.declared_symbols() and name in N._SIGNATURES and hasattr(L, name), name
        assert len(N._SIGNATURES[name][1]) == n_args
    assert len(N.declared_symbols()) >= 103
    assert tuple(N.ABI) >= (1, 20)
    major, minor = C.c_uint32(), C.c_uint32()
    assert N.lib().dcn_abi_version(C.byref(major), C.byref(minor)) == 0 and (major.value, minor.value) >= (1, 20)
    header = open(N.HEADER_PATH).read()
    assert len(re.findall(r"1\.20 = dcn_anchor_map_duplicates_enable / _reset / _info, dcn_mark_duplicates_batch\.", header)) == 1
    assert int(re.search(r"#define DCN_ABI_MINOR (\d+)", header).group(1)) >= 20
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert int(re.search(r"pub const DCN_ABI_MINOR: u32 = (\d+); +//", md).group(1)) >= 20
    for name in NAMES:
        assert re.search(r"pub fn %s\(" % name, md), name
    assert "pub struct dcn_duplicate_params {" in md
    for method in ("duplicates_enable", "duplicates_disable", "duplicates_reset", "duplicates_info", "mark_duplicates"):
        assert callable(getattr(dcn.AnchorMap, method))
    sig = inspect.signature(dcn.AnchorMap.mark_duplicates).parameters
    assert [(k, v.default) for k, v in sig.items()][1:] == [("offsets", inspect.Parameter.empty), ("rows", inspect.Parameter.empty), ("row_offsets", None),
                                                           ("paired", False), ("both_ends", False)]
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "DCN_DUPLICATE_TABLE_SLOTS" in readme and "deacon-hip markdup" in readme


def test_the_definition_is_stated_once(dcn):
    flat = " ".join(open(dcn._native.HEADER_PATH).read().replace(" *", " ").split())
    assert flat.count("THE DEFINITION OF A DUPLICATE") == 1
    for i in range(1, 8):
        assert len(re.findall(r"\bD%d\." % i, flat)) == 1, i
    body = flat.split("THE DEFINITION OF A DUPLICATE")[1].split("typedef struct dcn_duplicate_params")[0]
    for words in ("pos5 = ref_start - read_start on a forward row, ref_end + read_start on a reverse row",
                  "pos3 = ref_end + (L - read_end) on a forward row, ref_start - (L - read_end) on a reverse row",
                  "no decision rests on a hash alone", "First seen wins", "A lone mate is not matched against the ends of pairs",
                  "its first is UINT64_MAX", "keyed or not"):
        assert words in body, words
    assert "48 bytes per unit" in flat and "8 bytes per slot" in flat and "DCN_DUPLICATE_TABLE_SLOTS" in flat


PARAM_OFFSETS = dict(row_stride=0, paired=4, both_ends=8, reserved=12)


def test_struct_layout_agrees(tmp_path, dcn):
    N = dcn._native
    P = N.DuplicateParams
    assert C.sizeof(P) == 16
    assert {f: getattr(P, f).offset for f, _ in P._fields_} == PARAM_OFFSETS and [f for f, _ in P._fields_] == list(PARAM_OFFSETS)
    checks = " && ".join("offsetof(dcn_duplicate_params, %s) == %d" % kv for kv in PARAM_OFFSETS.items())
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "deacon_hip.h"\n'
                   "int (*f0)(dcn_index *, int) = dcn_anchor_map_duplicates_enable;\n"
                   "int (*f1)(dcn_index *) = dcn_anchor_map_duplicates_reset;\n"
                   "int (*f2)(const dcn_index *, uint64_t *, uint64_t *, uint64_t *) = dcn_anchor_map_duplicates_info;\n"
                   "int (*f3)(dcn_index *, const uint64_t *, uint32_t, const void *, const uint64_t *, const void *, uint64_t, uint8_t *, uint64_t *,\n"
                   "          uint64_t *) = dcn_mark_duplicates_batch;\n"
                   "int main(void){ dcn_duplicate_params p = {48, 1, 1, 0};\n"
                   "  return sizeof p == 16 && p.both_ends == 1 && DCN_ABI_MINOR >= 20 && " + checks + " ? 0 : 1; }\n")
    inc = os.path.dirname(N.HEADER_PATH)
    libdir = os.path.dirname(N.LIB_PATH)  # (the function pointers are initialised and never called)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, str(src), "-o", str(tmp_path / "t"), "-L", libdir,
                           "-ldeacon_hip", f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined"])
    assert subprocess.call([str(tmp_path / "t")]) == 0


def test_argument_errors_that_need_no_device(dcn):
    """in the order of the header: params NULL, reserved, paired, both_ends, row_stride, then the map"""
    N, L = dcn._native, dcn._native.lib()

    def prm(row_stride=48, paired=0, both_ends=0, reserved=0):
        return C.byref(N.DuplicateParams(row_stride, paired, both_ends, reserved))

    n_dup = C.c_uint64(77)
    offsets = np.array([0, 10], np.uint64)
    for p, word in ((None, b"params is NULL"),
                    (prm(row_stride=40, paired=2, both_ends=2, reserved=1), b"params.reserved must be 0"),
                    (prm(row_stride=40, paired=2, both_ends=2), b"params.paired must be 0 or 1"),
                    (prm(row_stride=40, both_ends=2), b"params.both_ends must be 0 or 1"),
                    (prm(row_stride=40), b"params.row_stride must be at least 48 and a multiple of 8"),
                    (prm(row_stride=52), b"params.row_stride must be at least 48 and a multiple of 8"),
                    (prm(row_stride=0, paired=1, both_ends=1), b"params.row_stride must be at least 48 and a multiple of 8"),
                    (prm(paired=1, both_ends=1), b"map is NULL"),
                    (prm(row_stride=80), b"map is NULL")):
        assert L.dcn_mark_duplicates_batch(None, offsets.ctypes.data_as(C.c_void_p), 1, p, None, None, 1, None, None, C.byref(n_dup)) == N.DCN_ERR_ARG
        assert word in L.dcn_last_error(), (word, L.dcn_last_error())
    assert n_dup.value == 77  # (nothing is written by a refused call)
    # the row_stride message is dcn_verify_batch's own
    assert L.dcn_verify_batch(None, None, None, None, 0, C.byref(N.VerifyParams(0, 0, 40, 0)), None, None, 0, None) == N.DCN_ERR_ARG
    assert b"params.row_stride must be at least 48 and a multiple of 8" in L.dcn_last_error()
    for call in (lambda: L.dcn_anchor_map_duplicates_enable(None, 1), lambda: L.dcn_anchor_map_duplicates_enable(None, 0),
                 lambda: L.dcn_anchor_map_duplicates_reset(None), lambda: L.dcn_anchor_map_duplicates_info(None, None, None, None)):
        assert call() == N.DCN_ERR_ARG and b"map is NULL" in L.dcn_last_error()


def test_key_rule_on_the_host(tmp_path):
    """tests/cpp/duplicate_key_test.cpp: dcn_duplicates.h's ends and keys under the address and undefined-behaviour sanitizers"""
    exe = tmp_path / "duplicate_key_test"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "deacon-server_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "duplicate_key_test.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and re.search(r"duplicate key rule ok: \d{4} checks", out.stdout) and out.stderr == "", \
        (out.stdout[-2000:], out.stderr[-2000:])


def test_the_shared_header_has_no_floating_point_and_no_device_only_code():
    src = open(os.path.join(ROOT, "deacon-server_amd", "csrc", "dcn_duplicates.h")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert not re.search(r"\b(float|double)\b", code) and "hip/" not in code and "atomic" not in code


MARKDUP_ERRORS = [
    (["markdup"], "the following required arguments were not provided: <REF>"),
    (["markdup", "ref.fa"], "nothing to write: give at least one of -o <OUTPUT>, --variants <FILE>, --pileup <FILE>, --sites <FILE>, --vcf <FILE>, "
                            "--duplicates <FILE>, -s <SUMMARY>"),
    (["markdup", "ref.fa", "--keep-duplicates", "--both-ends"],
     "nothing to write: give at least one of -o <OUTPUT>, --variants <FILE>, --pileup <FILE>, --sites <FILE>, --vcf <FILE>, --duplicates <FILE>, -s <SUMMARY>"),
    (["markdup", "ref.fa", "--duplicates"], "missing value for --duplicates"),
    (["markdup", "ref.fa", "--ploidy", "3"], "invalid value for --ploidy: must be 1..2"),
    (["markdup", "ref.fa", "--min-gq", "100"], "invalid value for --min-gq: must be 0..99"),
    (["markdup", "ref.fa", "--min-baseq", "256"], "invalid value for --min-baseq: must be 0..255"),
    (["markdup", "ref.fa", "in1", "in2"], "markdup takes one input: mates are independent here, run it once per file (unexpected argument 'in2')"),
    (["markdup", "--nope"], "unexpected argument '--nope'"),
    (["markdup", "ref.fa", "--paired"], "unexpected argument '--paired'"),
    (["markdup", "ref.fa", "--verified-only"], "unexpected argument '--verified-only'"),
]


@pytest.mark.parametrize("args,message", MARKDUP_ERRORS, ids=[" ".join(e[0]) for e in MARKDUP_ERRORS])
def test_markdup_error_exit_code_and_text(args, message):
    p = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    assert (p.returncode, p.stdout, p.stderr) == (1, "", "Error: " + message + "\n")


def test_markdup_refuses_fasta_and_names_the_record(tmp_path):
    reads = tmp_path / "reads.fa"
    reads.write_text(">read7 some words\nACGTACGT\n")
    message = "Error: markdup needs base qualities, and record 'read7' has none (FASTA): consensus takes reads without\n"
    p = subprocess.run([CLI, "markdup", "ref.fa", str(reads), "--duplicates", str(tmp_path / "d.tsv")], capture_output=True, text=True, timeout=60,
                       stdin=subprocess.DEVNULL)
    assert (p.returncode, p.stdout, p.stderr) == (1, "", message)


def test_markdup_help_text():
    p = subprocess.run([CLI, "markdup", "--help"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    with open(os.path.join(ROOT, "tests", "golden", "cli_help", "markdup.txt")) as f:
        want = f.read()
    assert (p.returncode, p.stderr, p.stdout) == (0, "", want)
    for word in ("Usage: deacon-hip markdup [OPTIONS] <REF> [READS]", "--keep-duplicates", "--both-ends", "--duplicates <FILE>",
                 "read ordinal first record strand pos5", "duplicates_both_ends", "keep_duplicates, reads_keyed (reads with an end), duplicate_reads and",
                 "distinct_fragments", "First seen wins", "soft clips do not matter", "Pairs as units", "not of this mode", "one input",
                 "--vcf <FILE>", "--ploidy <1|2>", "--min-baseq <Q>", "--variants <FILE>", "--pileup <FILE>", "--sites <FILE>"):
        assert word in want, word
    # every option line of genotype's help is in markdup's
    with open(os.path.join(ROOT, "tests", "golden", "cli_help", "genotype.txt")) as f:
        for line in f.read().split("Options:\n")[1].split("\n\n")[0].split("\n"):
            if re.match(r"^  (-\w,|   ) --?[\w-]+", line) and "--summary" not in line:
                assert line in want, line
    top = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert (top.stdout + top.stderr).count("\n  markdup ") == 1 and (top.stdout + top.stderr).count("\n  genotype ") == 1
    for sub in ("map", "verify", "align", "pileup", "extend", "consensus", "call", "genotype"):  # the other modes do not know markdup's options
        for opt in ("--keep-duplicates", "--both-ends", "--duplicates"):
            q = subprocess.run([CLI, sub, "ref.fa", opt, "1"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
            assert (q.returncode, q.stderr) == (1, "Error: unexpected argument '%s'\n" % opt)


# ---- the model alone: THE TESTS HERE THAT PASS WITHOUT THE FEATURE ---------------------------------------------------------
def test_model_alone_on_ends_written_out():
    """D3: row = (record, reverse, read_start, read_end, ref_start, ref_end)"""
    assert DW.end_of((3, 0, 5, 90, 105, 191), 100, True) == (3, 100, 0, 201)
    assert DW.end_of((3, 1, 5, 90, 105, 191), 100, True) == (3, 196, 1, 95)
    assert DW.end_of((3, 0, 5, 90, 105, 191), 100, False) == (3, 100, 0)
    assert DW.end_of((1, 0, 7, 100, 0, 93), 100, False) == (1, -7, 0)
    assert DW.end_of((0, 1, 4, 100, 904, 1000), 100, False) == (0, 1004, 1)
    # clips do not matter: the definition's own example
    assert DW.end_of((2, 0, 0, 100, 100, 200), 100, False) == DW.end_of((2, 0, 5, 100, 105, 200), 100, False)
    # the first placed row is the one
    assert DW.read_end_of([None, (2, 0, 0, 50, 10, 60), (2, 0, 0, 50, 70, 120)], 50, False) == (2, 10, 0)
    assert DW.read_end_of([(DW.UNPLACED, 0, 0, 0, 0, 0), (2, 1, 0, 50, 10, 60)], 50, False) == (2, 60, 1)
    assert DW.read_end_of([None, None], 50, False) is None and DW.read_end_of([], 50, True) is None


def test_model_alone_on_keys_written_out():
    """D4"""
    a, b = (4, 1000, 0), (4, 1400, 1)
    assert DW.key_of([a, b], True, False) == DW.key_of([b, a], True, False) == (True, False, 2, (a, b))
    assert DW.key_of([a, None], True, False) == DW.key_of([None, a], True, False) == (True, False, 1, (a,))
    assert DW.key_of([a], False, False) != DW.key_of([a, None], True, False)  # a lone mate is not a single read
    assert DW.key_of([a], False, False) != DW.key_of([a + (1100,)], False, True)
    assert DW.key_of([None, None], True, True) is None and DW.key_of([None], False, False) is None
    assert DW.key_of([(4, 1000, 1), (4, 1000, 0)], True, False)[3] == ((4, 1000, 0), (4, 1000, 1))  # the strand behind pos5
    assert DW.key_of([(5, -3, 0), (4, 1000, 0)], True, False)[3] == ((4, 1000, 0), (5, -3, 0))      # the record first


def test_model_alone_on_calls_written_out():
    """D2, D5, D6: ordinals, first, duplicates, units without a key, how the input is cut"""
    m = DW.Model()
    r = lambda pos, rev=0, rec=0: [(rec, rev, 0, 50, pos, pos + 50)]
    dup, first = m.mark([50] * 6, [r(10), r(20), [None], r(10), r(10, rec=1), r(20)])
    assert dup == [0, 0, 0, 1, 0, 1] and first == [0, 1, DW.NO_FIRST, 0, 4, 1] and m.info() == (6, 5, 3)
    dup, first = m.mark([50] * 3, [r(20), [], r(30)])  # a duplicate of an earlier call reports that call's ordinal
    assert dup == [1, 0, 0] and first == [1, DW.NO_FIRST, 8] and m.info() == (9, 7, 4)
    # the later unit of a call is the duplicate, whatever its index; the earlier one's first is its own ordinal
    m.reset()
    assert m.info() == (0, 0, 0)
    dup, first = m.mark([50] * 2, [r(10), r(10)])
    assert dup == [0, 1] and first == [0, 0]
    # paired: three pairs, the third the first with its mates swapped; a pair with one placed mate; a pair with none
    m.reset()
    f, g = (0, 0, 0, 50, 100, 150), (0, 1, 0, 50, 300, 350)
    dup, first = m.mark([50] * 10, [[f], [g], [f], [None], [g], [f], [None], [None], [None], [f]], paired=True)
    assert dup == [0, 0, 1, 0, 1] and first == [0, 1, 0, DW.NO_FIRST, 1] and m.info() == (5, 4, 2)
    # one input cut in two gives the same flags
    lengths, rows = [50] * 8, [r(10), r(20), r(10), [None], r(20), r(10), r(40), r(40)]
    whole = DW.Model().mark(lengths, rows)
    cut = DW.Model()
    a, b = cut.mark(lengths[:3], rows[:3]), cut.mark(lengths[3:], rows[3:])
    assert (a[0] + b[0], a[1] + b[1]) == whole and whole[0] == [0, 0, 1, 0, 1, 1, 0, 1]


def test_model_alone_on_random_units():
    rng = np.random.default_rng(5)
    for paired in (False, True):
        for rate in (0.0, 0.5):
            lengths, rows = DW.random_units(rng, 400, rate, [5000, 3000], paired=paired)
            assert len(lengths) == len(rows) == (800 if paired else 400)
            dup, first = DW.Model().mark(lengths, rows, paired=paired)
            share = sum(dup) / len(dup)
            assert (share < 0.02) if rate == 0.0 else (0.3 < share < 0.6), share
            assert all((f < u) == bool(d) for u, (d, f) in enumerate(zip(dup, first)) if f != DW.NO_FIRST)
            for row_list, L in zip(rows, lengths):  # every generated row is one that dcn_verify_batch's checks accept
                for row in row_list:
                    if row is not None:
                        rec, rev, rs, re_, fs, fe = row
                        assert rev in (0, 1) and 0 <= rs <= re_ <= L and 0 <= fs <= fe <= [5000, 3000][rec]

"""CPU checks of the pileup surface (dcn_anchor_map_pileup_enable / _reset / _fetch / _call, dcn_pileup_batch): declared,
exported and bound at ABI 1.15, the argument errors that are found before a device is looked at, `deacon-hip pileup`'s usage
errors and --help, the kernel's run walk compiled for the host under the sanitizers, and the model of the GPU tests
(tests/_pileup_worker.py) alone on cases whose counts are written out here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _pileup_worker as PW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "deacon-server_amd", "bin", "deacon-hip")
SYMBOLS = {"dcn_anchor_map_pileup_enable": 2, "dcn_anchor_map_pileup_reset": 1, "dcn_pileup_batch": 11, "dcn_anchor_map_pileup_fetch": 5,
           "dcn_anchor_map_pileup_call": 10}
COLUMNS = (("A", 0), ("C", 1), ("G", 2), ("T", 3), ("N", 4), ("DEL", 5), ("INS", 6), ("REV", 7), ("COLUMNS", 8))


def test_symbols_are_declared_exported_and_bound(dcn):
    N = dcn._native
    L = C.CDLL(N.LIB_PATH)
    for name, n_args in SYMBOLS.items():
        assert name in N.declared_symbols() and name in N._SIGNATURES and hasattr(L, name), name
        assert len(N._SIGNATURES[name][1]) == n_args
    assert tuple(N.ABI) >= (1, 15)
    major, minor = C.c_uint32(), C.c_uint32()
    assert N.lib().dcn_abi_version(C.byref(major), C.byref(minor)) == 0 and (major.value, minor.value) >= (1, 15)
    header = open(N.HEADER_PATH).read()
    assert len(re.findall(r"1\.15 = dcn_anchor_map_pileup_\* / dcn_pileup_batch", header)) == 1
    assert int(re.search(r"#define DCN_ABI_MINOR (\d+)", header).group(1)) >= 15
    for name, value in COLUMNS:
        assert re.search(r"#define DCN_PILEUP_%s %d\b" % (name, value), header) and getattr(N, "PILEUP_" + name) == value
        assert getattr(dcn, "PILEUP_" + name) == value
    for name, value in (("SITE_SUB", 1), ("SITE_DEL", 2), ("SITE_INS", 4), ("NO_CODE", 7)):
        assert re.search(r"#define DCN_PILEUP_%s %du\b" % (name, value), header) and getattr(N, "PILEUP_" + name) == value
    assert (PW.A, PW.C, PW.G, PW.T, PW.N, PW.DEL, PW.INS, PW.REV) == tuple(v for _, v in COLUMNS[:8])
    assert (PW.SITE_SUB, PW.SITE_DEL, PW.SITE_INS, PW.NO_CODE) == (N.PILEUP_SITE_SUB, N.PILEUP_SITE_DEL, N.PILEUP_SITE_INS, N.PILEUP_NO_CODE)
    flat = " ".join(header.replace(" *", " ").split())
    assert flat.count("THE DEFINITION OF A PILEUP") == 1 and "nothing saturates" in flat and "One call at a time per map" in flat
    assert "conventions of the layers above, not measured optima" in flat
    assert C.sizeof(N.PileupCallParams) == 16
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert int(re.search(r"pub const DCN_ABI_MINOR: u32 = (\d+); +//", md).group(1)) >= 15
    for name in SYMBOLS:
        assert re.search(r"pub fn %s\(" % name, md), name
    assert "DCN_PILEUP_COLUMNS" in md
    for method in ("pileup_enable", "pileup_disable", "pileup_reset", "pileup_fetch", "pileup_call"):
        assert hasattr(dcn.AnchorMap, method)
    assert hasattr(dcn.Placer, "pileup_batch")


def test_header_compiles_as_c(tmp_path, dcn):
    src = tmp_path / "t.c"
    src.write_text('#include "deacon_hip.h"\n'
                   "int (*f1)(dcn_index *, int) = dcn_anchor_map_pileup_enable;\n"
                   "int (*f2)(dcn_index *) = dcn_anchor_map_pileup_reset;\n"
                   "int (*f3)(dcn_ctx *, dcn_index *, const uint8_t *, const uint64_t *, uint32_t, const void *, const uint64_t *,\n"
                   "          const void *, uint64_t, uint32_t *, uint64_t *) = dcn_pileup_batch;\n"
                   "int (*f4)(const dcn_index *, uint32_t, uint64_t, uint64_t, uint32_t *) = dcn_anchor_map_pileup_fetch;\n"
                   "int (*f5)(const dcn_index *, const void *, uint32_t, uint64_t, uint64_t, uint8_t *, uint64_t *, uint32_t *, uint64_t,\n"
                   "          uint64_t *) = dcn_anchor_map_pileup_call;\n"
                   "int main(void){ dcn_pileup_call_params p = {3, 500, {0, 0}};\n"
                   "  return sizeof p == 16 && DCN_PILEUP_A == 0 && DCN_PILEUP_T == 3 && DCN_PILEUP_DEL == 5 && DCN_PILEUP_REV == 7 &&\n"
                   "         DCN_PILEUP_COLUMNS == 8 && DCN_PILEUP_SITE_INS == 4u && DCN_ABI_MINOR >= 15 && p.min_depth == 3 ? 0 : 1; }\n")
    inc = os.path.dirname(dcn._native.HEADER_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_argument_errors_that_need_no_device(dcn):
    """dcn_pileup_batch: dcn_verify_batch's checks in its order, with its messages; the map calls: NULL, and the parameters
    of a call before the map is looked at"""
    N, L = dcn._native, dcn._native.lib()

    def prm(edits=1023, permille=200, stride=48, reserved=0):
        return C.byref(N.VerifyParams(edits, permille, stride, reserved))

    stand_in = (C.c_uint8 * 4096)()
    added = C.c_uint64(77)
    for args, word in (((None, None, None), b"params is NULL"),
                       ((None, None, prm(reserved=1)), b"reserved"),
                       ((None, None, prm(edits=1024)), b"max_edits must be 0..1023"),
                       ((None, None, prm(permille=1001)), b"max_permille must be 0..1000"),
                       ((None, None, prm(stride=40)), b"row_stride"),
                       ((None, None, prm(stride=52)), b"row_stride"),
                       ((None, None, prm()), b"ctx is NULL"),
                       ((C.cast(stand_in, C.c_void_p), None, prm(stride=64)), b"map is NULL")):
        assert L.dcn_pileup_batch(args[0], args[1], None, None, 0, args[2], None, None, 0, None, C.byref(added)) == N.DCN_ERR_ARG
        message = L.dcn_last_error()
        assert word in message, (word, message)
        assert L.dcn_verify_batch(args[0], args[1], None, None, 0, args[2], None, None, 0, None) == N.DCN_ERR_ARG
        assert L.dcn_last_error() == message
    assert added.value == 77  # (nothing is written by a refused call)
    n = C.c_uint64()
    out = (C.c_uint32 * 8)()
    for rc in (L.dcn_anchor_map_pileup_enable(None, 1), L.dcn_anchor_map_pileup_enable(None, 0), L.dcn_anchor_map_pileup_reset(None),
               L.dcn_anchor_map_pileup_fetch(None, 0, 0, 1, out),
               L.dcn_anchor_map_pileup_call(None, C.byref(N.PileupCallParams(3, 500, (C.c_uint32 * 2)(0, 0))), 0, 0, 1, None, None, None, 0, C.byref(n))):
        assert rc == N.DCN_ERR_ARG and b"map is NULL" in L.dcn_last_error()
    for params, word in ((None, b"params is NULL"), (C.byref(N.PileupCallParams(3, 1001, (C.c_uint32 * 2)(0, 0))), b"min_permille must be 0..1000"),
                         (C.byref(N.PileupCallParams(3, 500, (C.c_uint32 * 2)(1, 0))), b"reserved"),
                         (C.byref(N.PileupCallParams(3, 500, (C.c_uint32 * 2)(0, 9))), b"reserved")):
        assert L.dcn_anchor_map_pileup_call(None, params, 0, 0, 1, None, None, None, 0, C.byref(n)) == N.DCN_ERR_ARG
        assert word in L.dcn_last_error()


PILEUP_ERRORS = [
    (["pileup"], "the following required arguments were not provided: <REF>"),
    (["pileup", "ref.fa", "--min-mapq", "61"], "invalid value for --min-mapq: must be 0..60"),
    (["pileup", "ref.fa", "--min-frac", "1001"], "invalid value for --min-frac: must be 0..1000"),
    (["pileup", "ref.fa", "-e", "1024"], "invalid value for --max-edits: must be 0..1023"),
    (["pileup", "ref.fa", "in1", "in2"], "pileup takes one input: mates are independent here, run it once per file (unexpected argument 'in2')"),
    (["pileup", "--nope"], "unexpected argument '--nope'"),
    (["pileup", "ref.fa", "--verified-only"], "unexpected argument '--verified-only'"),
    (["pileup", "ref.fa", "--sites"], "missing value for --sites"),
]


@pytest.mark.parametrize("args,message", PILEUP_ERRORS, ids=[" ".join(e[0]) for e in PILEUP_ERRORS])
def test_pileup_error_exit_code_and_text(args, message):
    p = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    assert (p.returncode, p.stdout, p.stderr) == (1, "", "Error: " + message + "\n")


def test_pileup_help_text():
    p = subprocess.run([CLI, "pileup", "--help"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    with open(os.path.join(ROOT, "tests", "golden", "cli_help", "pileup.txt")) as f:
        want = f.read()
    assert (p.returncode, p.stderr, p.stdout) == (0, "", want)
    for word in ("Usage: deacon-hip pileup [OPTIONS] <REF> [READS]", "record pos ref A C G T N del ins rev", "pos is 0-based, as in PAF",
                 "--all-positions", "--sites <FILE>", "record pos ref call depth flags", "--min-depth <N>", "--min-frac <N>",
                 "--min-mapq <N>", "[default: 1, a convention]", "--all-ranks", "[default: 3, a convention]", "[default: 500, a convention]",
                 "conventions, not measured optima", "-N, --max-placements <N>", "rows_added"):
        assert word in want, word
    top = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert (top.stdout + top.stderr).count("\n  pileup ") == 1 and "\n  align " in top.stdout + top.stderr
    # the other modes of the same driver do not know pileup's options
    for sub in ("map", "verify", "align"):
        q = subprocess.run([CLI, sub, "ref.fa", "--min-mapq", "3"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
        assert (q.returncode, q.stderr) == (1, "Error: unexpected argument '--min-mapq'\n")


def test_run_walk_on_the_host(tmp_path):
    """tests/cpp/pileup_walk_test.cpp: dcn_pileup.h's walk in the kernel's shape (chunks of 64 runs, the chunk's prefix sum
    emulated serially, 64 lanes per run) into a count array of exactly n positions between guard words, against a walk step
    by step, under the address and undefined-behaviour sanitizers: a few thousand random run lists, I runs first and last, 63,
    64, 65 and 129 runs, runs of 63, 64 and 65 bases"""
    exe = tmp_path / "pileup_walk_test"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-I", os.path.join(ROOT, "deacon-server_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "pileup_walk_test.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "pileup walk ok" in out.stdout, out.stderr[-2000:]


def row(**columns):
    r = [0] * 8
    for name, v in columns.items():
        r[getattr(PW, name)] = v
    return r


HAND = [
    # (S, T, reverse, the runs, counts per position of T, why)
    (b"ACGT", b"ACGT", 0, "4=", [row(A=1), row(C=1), row(G=1), row(T=1)], "four equal bases: each in its own column"),
    (b"ACTT", b"ACGT", 0, "2=1X1=", [row(A=1), row(C=1), row(T=1), row(T=1)], "X counts the read's base"),
    (b"AGT", b"ACGT", 0, "1=1D2=", [row(A=1), row(DEL=1), row(G=1), row(T=1)], "a base of T alone: DEL there"),
    (b"ACCGT", b"AGT", 0, "1=2I2=", [row(A=1, INS=1), row(G=1), row(T=1)], "an I run of two: one INS, at the base in front"),
    (b"CCAGT", b"AGT", 0, "2I3=", [row(A=1, INS=1), row(G=1), row(T=1)], "an I run first: INS at ref_start"),
    (b"AGTCC", b"AGT", 0, "3=2I", [row(A=1), row(G=1), row(T=1, INS=1)], "an I run last: INS on the last base"),
    (b"ACTT", b"ACGT", 1, "2=1X1=", [row(A=1, REV=1), row(C=1, REV=1), row(T=1, REV=1), row(T=1, REV=1)], "a reverse row: REV beside every step"),
    (b"AGT", b"ACGT", 1, "1=1D2=", [row(A=1, REV=1), row(DEL=1, REV=1), row(G=1, REV=1), row(T=1, REV=1)], "... a D step too"),
    (b"ACNGTA", b"ACGGTA", 0, "2=1X3=", [row(A=1), row(C=1), row(N=1), row(G=1), row(T=1), row(A=1)], "a read N under X: column N"),
    (b"acgt", b"ACGT", 0, "4=", [row(A=1), row(C=1), row(G=1), row(T=1)], "case does not matter"),
]


@pytest.mark.parametrize("S,T,reverse,text,want,why", HAND, ids=["%s/%s/%d" % (h[0].decode(), h[1].decode(), h[2]) for h in HAND])
def test_model_alone_on_rows_written_out(S, T, reverse, text, want, why):
    """THE TESTS HERE THAT PASS WITHOUT THE FEATURE: they run the model only"""
    import _align_worker as AW
    d, runs = AW.align_pair(S, T)
    assert AW.cigar_text(runs) == text, why
    counts = np.zeros((len(T) + 2, 8), np.int64)  # a position on either side that nothing may reach
    assert PW.add_runs(counts, S, 1, reverse, runs) == (len(S), len(T))
    assert counts[1:-1].tolist() == want, why
    assert not counts[0].any() and not counts[-1].any()
    assert (counts[1:-1, :6].sum(axis=1) == 1).all()  # rule P4


CALLS = [
    # (counts by column name, ref, min_depth, min_permille, call, flags, call code, ref code, why)
    (dict(A=2, C=2), "C", 3, 500, "A", PW.SITE_SUB, 0, 1, "a tie A = C calls A, the first"),
    (dict(C=2, T=2), "C", 3, 500, "C", 0, 1, 1, "... C before T: the reference, no site"),
    (dict(G=3, A=1), "A", 4, 750, "G", PW.SITE_SUB, 2, 0, "best * 1000 = depth * permille: called"),
    (dict(G=2, A=1, C=1), "A", 4, 750, "N", 0, 7, 0, "one read fewer for the best: not called"),
    (dict(G=2), "A", 3, 500, "N", 0, 7, 0, "depth = min_depth - 1"),
    (dict(G=3), "A", 3, 500, "G", PW.SITE_SUB, 2, 0, "depth = min_depth"),
    (dict(DEL=3, A=1), "A", 3, 500, "-", PW.SITE_DEL, 4, 0, "a DEL majority"),
    (dict(A=1, C=1, G=1, T=1, INS=2), "A", 3, 500, "N", PW.SITE_INS, 7, 0, "an INS flag on a position without a call"),
    (dict(A=4, INS=2), "A", 3, 500, "A", PW.SITE_INS, 0, 0, "... and on a called one that equals the reference"),
    (dict(A=4, INS=1), "A", 3, 500, "A", 0, 0, 0, "INS below the fraction"),
    (dict(N=5, A=1), "A", 3, 100, "A", 0, 0, 0, "N never wins, but counts in the depth"),
    (dict(N=5), "A", 3, 0, "A", PW.SITE_INS, 0, 0, "... a depth of N alone at permille 0: the first column with no read for it, and INS with none"),
    (dict(A=3), "N", 3, 500, "A", PW.SITE_SUB, 0, 7, "a reference N differs from every call"),
    (dict(), "A", 0, 0, "N", 0, 7, 0, "depth 0 is never called, whatever min_depth says"),
    (dict(INS=3, REV=9), "A", 0, 0, "N", 0, 7, 0, "... nor flagged"),
]


@pytest.mark.parametrize("counts,ref,min_depth,min_permille,call,flags,code,ref_code,why", CALLS, ids=[c[-1] for c in CALLS])
def test_model_alone_on_calls_written_out(counts, ref, min_depth, min_permille, call, flags, code, ref_code, why):
    """... rule P6, one boundary each"""
    got = PW.call_position(row(**counts), ord(ref), min_depth, min_permille)
    assert got == (call, flags | code << 8 | ref_code << 16), why

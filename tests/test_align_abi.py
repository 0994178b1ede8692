"""CPU checks of the align surface (dcn_align_batch): declared, exported and bound at ABI 1.14, the argument errors that are
found before a device is looked at, `deacon-hip align`'s usage errors and --help, the kernel's walk back compiled for the
host under the sanitizers, and the model of the GPU tests (tests/_align_worker.py) alone on pairs whose CIGAR is written
out here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _align_worker as AW
import _verify_worker as VW
from conftest import random_reads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "deacon-server_amd", "bin", "deacon-hip")


def test_symbol_is_declared_exported_and_bound(dcn):
    N = dcn._native
    L = C.CDLL(N.LIB_PATH)
    assert "dcn_align_batch" in N.declared_symbols() and "dcn_align_batch" in N._SIGNATURES and hasattr(L, "dcn_align_batch")
    assert len(N._SIGNATURES["dcn_align_batch"][1]) == 13
    assert tuple(N.ABI) >= (1, 14)
    major, minor = C.c_uint32(), C.c_uint32()
    assert N.lib().dcn_abi_version(C.byref(major), C.byref(minor)) == 0 and (major.value, minor.value) >= (1, 14)
    header = open(N.HEADER_PATH).read()
    assert re.search(r"1\.14 = dcn_align_batch", header)
    assert int(re.search(r"#define DCN_ABI_MINOR (\d+)", header).group(1)) >= 14
    for name, value in (("INS", 1), ("DEL", 2), ("EQUAL", 7), ("DIFF", 8)):
        assert re.search(r"#define DCN_CIGAR_%s %du\b" % (name, value), header) and getattr(N, "CIGAR_" + name) == value
    assert (AW.OP_I, AW.OP_D, AW.OP_EQ, AW.OP_X) == (N.CIGAR_INS, N.CIGAR_DEL, N.CIGAR_EQUAL, N.CIGAR_DIFF)
    flat = " ".join(header.replace(" *", " ").split())
    assert flat.count("THE DEFINITION OF AN ALIGNED PLACEMENT") == 1 and "DCN_ALIGN_TRACE_BYTES" in flat
    assert "a convention, not a measured optimum" in flat and "n_ops <= 2 d + 1" in flat
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert int(re.search(r"pub const DCN_ABI_MINOR: u32 = (\d+); +//", md).group(1)) >= 14
    assert re.search(r"pub fn dcn_align_batch\(", md)
    assert hasattr(dcn.Placer, "align_batch") and dcn.cigar_string is dcn.filter.cigar_string


def test_header_compiles_as_c(tmp_path, dcn):
    src = tmp_path / "t.c"
    src.write_text('#include "deacon_hip.h"\n'
                   "int (*f)(dcn_ctx *, const dcn_index *, const uint8_t *, const uint64_t *, uint32_t, const void *, const uint64_t *,\n"
                   "         const void *, uint64_t, uint32_t *, uint64_t *, uint32_t *, uint64_t) = dcn_align_batch;\n"
                   "int main(void){ return DCN_CIGAR_INS == 1u && DCN_CIGAR_DEL == 2u && DCN_CIGAR_EQUAL == 7u && DCN_CIGAR_DIFF == 8u && "
                   "DCN_ABI_MINOR >= 14 ? 0 : 1; }\n")
    inc = os.path.dirname(dcn._native.HEADER_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_argument_errors_that_need_no_device(dcn):
    """dcn_verify_batch's checks in its order, with its messages: the parameters, then the context and the map"""
    N, L = dcn._native, dcn._native.lib()

    def prm(edits=1023, permille=200, stride=48, reserved=0):
        return C.byref(N.VerifyParams(edits, permille, stride, reserved))

    stand_in = (C.c_uint8 * 4096)()
    offs = (C.c_uint64 * 1)()

    def call(ctx, map_, params):
        return L.dcn_align_batch(ctx, map_, None, None, 0, params, None, None, 0, None, offs, None, 0)

    for args, word in (((None, None, None), b"params is NULL"),
                       ((None, None, prm(reserved=1)), b"reserved"),
                       ((None, None, prm(edits=1024)), b"max_edits must be 0..1023"),
                       ((None, None, prm(permille=1001)), b"max_permille must be 0..1000"),
                       ((None, None, prm(stride=40)), b"row_stride"),
                       ((None, None, prm(stride=0)), b"row_stride"),
                       ((None, None, prm(stride=52)), b"row_stride"),
                       ((None, None, prm()), b"ctx is NULL"),
                       ((None, None, prm(edits=0, permille=0, stride=80)), b"ctx is NULL"),
                       ((C.cast(stand_in, C.c_void_p), None, prm(stride=64)), b"map is NULL")):
        assert call(*args) == N.DCN_ERR_ARG
        assert word in L.dcn_last_error(), (word, L.dcn_last_error())
        same = L.dcn_verify_batch(args[0], args[1], None, None, 0, args[2], None, None, 0, None)
        assert same == N.DCN_ERR_ARG and word in L.dcn_last_error()


ALIGN_ERRORS = [
    (["align"], "the following required arguments were not provided: <REF>"),
    (["align", "ref.fa", "-e", "1024"], "invalid value for --max-edits: must be 0..1023"),
    (["align", "ref.fa", "--max-edits", "x"], "invalid value for --max-edits: must be 0..1023"),
    (["align", "ref.fa", "--max-div", "1001"], "invalid value for --max-div: must be 0..1000"),
    (["align", "ref.fa", "-N", "0"], "invalid value for -N: must be 1..8"),
    (["align", "ref.fa", "-e"], "missing value for -e"),
    (["align", "ref.fa", "in1", "in2"], "align takes one input: mates are independent here, run it once per file (unexpected argument 'in2')"),
    (["align", "--nope"], "unexpected argument '--nope'"),
    (["align", "ref.fa", "--cigar"], "unexpected argument '--cigar'"),
]


@pytest.mark.parametrize("args,message", ALIGN_ERRORS, ids=[" ".join(e[0]) for e in ALIGN_ERRORS])
def test_align_error_exit_code_and_text(args, message):
    p = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    assert (p.returncode, p.stdout, p.stderr) == (1, "", "Error: " + message + "\n")


def test_align_help_text():
    p = subprocess.run([CLI, "align", "--help"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    with open(os.path.join(ROOT, "tests", "golden", "cli_help", "align.txt")) as f:
        want = f.read()
    assert (p.returncode, p.stderr, p.stdout) == (0, "", want)
    for word in ("Usage: deacon-hip align [OPTIONS] <REF> [READS]", "-e, --max-edits <N>", "--max-div <N>", "--verified-only", "cg:Z:<cigar>",
                 "NM:i:<edits>", "the number of = bases", "X before I before D before =", "-N, --max-placements <N>", "cigar_ops"):
        assert word in want, word
    top = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert "\n  align " in top.stdout + top.stderr and "\n  verify " in top.stdout + top.stderr


def test_walk_back_on_the_host(tmp_path):
    """tests/cpp/align_trace_test.cpp: the kernels' wavefront step (dcn_wavefront.h) fills the triangular trace, dcn_align.h's walk back over it into
    a slot of exactly 2 d + 1 runs, and a walk over the full table by rule A3, under the address and undefined-behaviour
    sanitizers: a few thousand random pairs (three alphabets, empty sides, unrelated pairs) and d = 0, 1, 31, 32, 33, 63, 64, 65"""
    exe = tmp_path / "align_trace_test"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-I", os.path.join(ROOT, "deacon-server_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "align_trace_test.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "align trace ok" in out.stdout, out.stderr[-2000:]


HAND = [
    # (S, T, d, the runs rule A3 gives, why)
    (b"AAAA", b"AAA", 1, "3=1I", "a homopolymer with one base more in S: I is met first from the end, so it is the last run"),
    (b"AAA", b"AAAA", 1, "3=1D", "... one base more in T"),
    (b"ACGTTTTTGCA", b"ACGTTTTGCA", 1, "7=1I3=", "... inside: from the end the walk takes '=' until a gap predecessor costs one less, at the last T of the run"),
    (b"ACGACGACG", b"ACGACG", 3, "6=3I", "a tandem repeat with a unit more in S: the unit at the end is the one alone"),
    (b"ACGACG", b"ACGACGACG", 3, "6=3D", "... in T"),
    (b"AC", b"CA", 2, "2X", "X before I and D: two substitutions, not 1D1=1I"),
    (b"ACGT", b"AGT", 1, "1=1I2=", "one base of S alone"),
    (b"AGT", b"ACGT", 1, "1=1D2=", "one base of T alone"),
    (b"GATTACA", b"GCATGCT", 4, "1=1D2=1I1X1=1X", "every op in one pair"),
    (b"", b"ACG", 3, "3D", "m = 0"),
    (b"ACG", b"", 3, "3I", "n = 0"),
    (b"", b"", 0, "", "m = n = 0: no run"),
    (b"N", b"N", 1, "1X", "N against N: an invalid base equals nothing"),
    (b"ACNGT", b"ACNGT", 1, "2=1X2=", "... between equal bases"),
    (b"acgt", b"ACGT", 0, "4=", "case does not matter"),
    (b"ACGT", b"ACGT", 0, "4=", "d = 0: one run"),
    (b"AT", b"ATA", 1, "2=1D", "I / D against '=': D[i][j-1] = s - 1 wins over the diagonal"),
    (b"TAA", b"TA", 1, "2=1I", "... and I"),
]


@pytest.mark.parametrize("S,T,d,text,why", HAND, ids=["%s/%s" % (h[0].decode() or "-", h[1].decode() or "-") for h in HAND])
def test_model_alone_on_pairs_written_out(S, T, d, text, why):
    """THE TESTS HERE THAT PASS WITHOUT THE FEATURE: they run the model only, one per tie-break of rule A3"""
    got_d, runs = AW.align_pair(S, T)
    assert (got_d, AW.cigar_text(runs)) == (d, text), why
    assert got_d == VW.levenshtein(S, T) and AW.parse_cigar(text) == runs
    AW.check_sums(runs, len(S), len(T), d)


def test_model_alone_on_random_pairs():
    """the model's distance is the verify model's; rule A4's sums hold; the runs replayed over S give T's length and only
    EQUAL pairs under '='"""
    rng = np.random.default_rng(1402)
    for q in range(120):
        T = random_reads(rng, 1, 0, 200)[0]
        S = VW.mutate_mixed(rng, T, (q % 7) * 0.04)
        if q % 9 == 0:
            S = S[:len(S) // 2] + b"N" + S[len(S) // 2:]
        d, runs = AW.align_pair(S, T)
        assert d == VW.levenshtein(S, T)
        AW.check_sums(runs, len(S), len(T), d)
        s, t = VW.encode(S, -1), VW.encode(T, -2)
        i = j = 0
        for x in runs:
            ln, op = x >> 4, x & 15
            if op == AW.OP_EQ:
                assert (s[i:i + ln] == t[j:j + ln]).all()
            i, j = i + ln * (op != AW.OP_D), j + ln * (op != AW.OP_I)
        assert (i, j) == (len(S), len(T))


def test_cigar_string(dcn):
    assert dcn.cigar_string(np.array([(12 << 4) | 7, (1 << 4) | 8, (3 << 4) | 1, (2 << 4) | 2], np.uint32)) == "12=1X3I2D"
    assert dcn.cigar_string([]) == "" and dcn.cigar_string(AW.parse_cigar("5=1D7=")) == "5=1D7="

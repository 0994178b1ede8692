"""CPU checks of the verify surface (dcn_anchor_map_keep_bases, dcn_anchor_map_fetch, dcn_verify_batch): declared, exported
and bound at ABI 1.13, the params' layout, the argument errors that are found before a device is looked at,
`deacon-hip verify`'s usage errors and --help, the kernel's word helpers compiled for the host, and one test of the model
of the GPU tests (tests/_verify_worker.py) alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _verify_worker as VW
from conftest import random_reads, revcomp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "deacon-server_amd", "bin", "deacon-hip")
NAMES = ("dcn_anchor_map_keep_bases", "dcn_anchor_map_fetch", "dcn_verify_batch")


def test_symbols_are_declared_exported_and_bound(dcn):
    N = dcn._native
    L = C.CDLL(N.LIB_PATH)
    for name in NAMES:
        assert name in N.declared_symbols() and name in N._SIGNATURES and hasattr(L, name), name
    assert tuple(N.ABI) >= (1, 13)
    major, minor = C.c_uint32(), C.c_uint32()
    assert N.lib().dcn_abi_version(C.byref(major), C.byref(minor)) == 0 and (major.value, minor.value) >= (1, 13)
    header = open(N.HEADER_PATH).read()
    assert re.search(r"1\.13 = dcn_anchor_map_keep_bases / _fetch, dcn_verify_batch", header)
    assert int(re.search(r"#define DCN_ABI_MINOR (\d+)", header).group(1)) >= 13
    assert re.search(r"#define DCN_VERIFY_MAX_EDITS 1023u\b", header) and N.VERIFY_MAX_EDITS == 1023 == VW.MAX_EDITS
    assert re.search(r"#define DCN_VERIFY_OVER 0xFFFFFFFEu\b", header) and dcn.VERIFY_OVER == N.VERIFY_OVER == VW.OVER
    assert re.search(r"#define DCN_VERIFY_UNPLACED 0xFFFFFFFFu\b", header) and dcn.VERIFY_UNPLACED == N.VERIFY_UNPLACED == VW.UNPLACED
    flat = " ".join(header.replace(" *", " ").split())
    assert "THE DEFINITION OF A VERIFIED PLACEMENT" in flat and "0.375 B per base" in flat and "dcn_index_memory does not count" in flat
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert int(re.search(r"pub const DCN_ABI_MINOR: u32 = (\d+); +//", md).group(1)) >= 13
    for name in NAMES:
        assert re.search(r"pub fn %s\(" % name, md), name
    assert hasattr(dcn.Placer, "verify_batch") and hasattr(dcn.AnchorMap, "fetch")
    assert "keep_bases" in dcn.AnchorMap.__init__.__code__.co_varnames


def test_params_layout(tmp_path, dcn):
    P = dcn._native.VerifyParams
    assert C.sizeof(P) == 16
    assert (P.max_edits.offset, P.max_permille.offset, P.row_stride.offset, P.reserved.offset) == (0, 4, 8, 12)
    assert re.search(r"\}\s*dcn_verify_params;\s*/\* 16 bytes \*/", open(dcn._native.HEADER_PATH).read())
    src = tmp_path / "t.c"
    src.write_text('#include "deacon_hip.h"\n#include <stddef.h>\n'
                   "int main(void){ return sizeof(dcn_verify_params) == 16 && offsetof(dcn_verify_params, row_stride) == 8 && "
                   "offsetof(dcn_verify_params, reserved) == 12 && DCN_VERIFY_OVER == 0xFFFFFFFEu && DCN_VERIFY_UNPLACED == 0xFFFFFFFFu && "
                   "DCN_VERIFY_MAX_EDITS == 1023u ? 0 : 1; }\n")
    inc = os.path.dirname(dcn._native.HEADER_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, str(src), "-o", str(tmp_path / "t")])
    assert subprocess.call([str(tmp_path / "t")]) == 0


def test_argument_errors_that_need_no_device(dcn):
    """the parameters are judged first, then the context and the map: nothing here is dereferenced"""
    N, L = dcn._native, dcn._native.lib()

    def prm(edits=1023, permille=200, stride=48, reserved=0):
        return C.byref(N.VerifyParams(edits, permille, stride, reserved))

    stand_in = (C.c_uint8 * 4096)()

    def call(ctx, map_, params):
        return L.dcn_verify_batch(ctx, map_, None, None, 0, params, None, None, 0, None)

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
    assert L.dcn_anchor_map_keep_bases(None) == N.DCN_ERR_ARG and b"map is NULL" in L.dcn_last_error()
    assert L.dcn_anchor_map_fetch(None, 0, 0, 0, None) == N.DCN_ERR_ARG and b"map is NULL" in L.dcn_last_error()


VERIFY_ERRORS = [
    (["verify"], "the following required arguments were not provided: <REF>"),
    (["verify", "ref.fa", "-e", "1024"], "invalid value for --max-edits: must be 0..1023"),
    (["verify", "ref.fa", "--max-edits", "x"], "invalid value for --max-edits: must be 0..1023"),
    (["verify", "ref.fa", "--max-div", "1001"], "invalid value for --max-div: must be 0..1000"),
    (["verify", "ref.fa", "-N", "0"], "invalid value for -N: must be 1..8"),
    (["verify", "ref.fa", "-e"], "missing value for -e"),
    (["verify", "ref.fa", "in1", "in2"], "verify takes one input: mates are independent here, run it once per file (unexpected argument 'in2')"),
    (["verify", "--nope"], "unexpected argument '--nope'"),
    (["map", "ref.fa", "--verified-only"], "unexpected argument '--verified-only'"),  # (map keeps its options)
    (["map", "ref.fa", "-e", "5"], "unexpected argument '-e'"),
]


@pytest.mark.parametrize("args,message", VERIFY_ERRORS, ids=[" ".join(e[0]) for e in VERIFY_ERRORS])
def test_verify_error_exit_code_and_text(args, message):
    p = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    assert (p.returncode, p.stdout, p.stderr) == (1, "", "Error: " + message + "\n")


def test_verify_help_text():
    p = subprocess.run([CLI, "verify", "--help"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    with open(os.path.join(ROOT, "tests", "golden", "cli_help", "verify.txt")) as f:
        want = f.read()
    assert (p.returncode, p.stderr, p.stdout) == (0, "", want)
    for word in ("Usage: deacon-hip verify [OPTIONS] <REF> [READS]", "-e, --max-edits <N>", "[default: 1023, a convention]", "--max-div <N>",
                 "--verified-only", "ve:i:1", "NM:i:<edits>", "lower bound on the matching bases", "conventions, not measured optima",
                 "-N, --max-placements <N>", "--band <N>"):
        assert word in want, word
    top = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert "\n  verify " in top.stdout + top.stderr and "\n  map " in top.stdout + top.stderr


def test_word_helpers_on_the_host(tmp_path):
    """tests/cpp/verify_helpers_test.cpp: dcn_wavefront.h compiled for the host under the address and undefined-behaviour
    sanitizers, against naive loops: fetches, the reverse complement of a word, runs from every offset 0..31 of both streams"""
    exe = tmp_path / "verify_helpers_test"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-I", os.path.join(ROOT, "deacon-server_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "verify_helpers_test.cpp"), "-o", str(exe)])
    subprocess.check_call([str(exe)])


def test_wavefront_step_on_the_host(tmp_path):
    """tests/cpp/wavefront_test.cpp: the wavefront step that the verify, align and extend kernels share (dcn_wavefront.h)
    compiled for the host under the address and undefined-behaviour sanitizers, driven over all scores as verify_kernel
    drives it, every F_s[k] and the thresholded distance against a full Levenshtein table, under both word loads"""
    exe = tmp_path / "wavefront_test"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-I", os.path.join(ROOT, "deacon-server_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "wavefront_test.cpp"), "-o", str(exe)])
    subprocess.check_call([str(exe)])


def test_model_alone_on_planted_edits():
    """THE ONE TEST HERE THAT PASSES WITHOUT THE FEATURE: it runs the model only.  Planted substitutions, insertions and
    deletions give d <= the number planted (and exactly that for one edit); the reverse complement of both sides gives the
    same d; an N equals nothing; case does not matter; the two forms of the model agree; the threshold is rule 4's."""
    rng = np.random.default_rng(1301)
    pairs, planted = [], []
    for i in range(150):
        s = random_reads(rng, 1, 40, 300)[0]
        e = (int(rng.integers(0, 6)), int(rng.integers(0, 4)), int(rng.integers(0, 4)))
        pairs.append((s, VW.edit(rng, s, *e)))
        planted.append(sum(e))
    d = VW.levenshtein_many(pairs, chunk=40)
    assert (d <= np.array(planted)).all() and (d >= [abs(len(s) - len(t)) for s, t in pairs]).all()
    assert d.tolist() == [VW.levenshtein(s, t) for s, t in pairs]
    assert d.tolist() == VW.levenshtein_many([(revcomp(s), revcomp(t)) for s, t in pairs]).tolist()
    assert d.tolist() == VW.levenshtein_many([(s.lower(), t) for s, t in pairs]).tolist()
    s = random_reads(rng, 1, 100, 100)[0]
    for kind in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        assert VW.levenshtein(s, VW.edit(rng, s, *kind)) == 1
    assert VW.levenshtein(s, s) == 0 and VW.levenshtein(b"", s) == 100 and VW.levenshtein(s, b"") == 100 and VW.levenshtein(b"", b"") == 0
    n = s[:50] + b"N" + s[51:]
    assert VW.levenshtein(n, n) == 1 and VW.levenshtein(n, s) == 1 and VW.levenshtein(b"NNN", b"NNN") == 3
    assert VW.levenshtein(b"ACGT", b"AGT") == 1 and VW.levenshtein(b"GATTACA", b"GCATGCT") == 4
    assert VW.threshold(199, 150, 1023, 5) == 0 and VW.threshold(150, 200, 1023, 5) == 1 and VW.threshold(3000, 3000) == 600
    assert VW.threshold(10000, 9000) == 1023 and VW.threshold(100, 100, 7, 1000) == 7 and VW.threshold(100, 100, 1023, 0) == 0

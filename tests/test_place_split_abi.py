"""CPU checks of dcn_place_split_batch's boundary: declared, exported and bound at ABI 1.10, the two structs' layout, the
argument errors that are found before a device is looked at, `deacon-hip map`'s usage errors and --help, and one test of
the model of the GPU tests (tests/_place_split_worker.py) alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _place_split_worker as SW
import _place_worker as PW
from conftest import random_reads, revcomp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "deacon-server_amd", "bin", "deacon-hip")
NAME = "dcn_place_split_batch"


def test_symbol_is_declared_exported_and_bound(dcn):
    N = dcn._native
    L = C.CDLL(N.LIB_PATH)
    assert NAME in N.declared_symbols() and NAME in N._SIGNATURES and hasattr(L, NAME)
    assert tuple(N.ABI) >= (1, 10)
    major, minor = C.c_uint32(), C.c_uint32()
    assert N.lib().dcn_abi_version(C.byref(major), C.byref(minor)) == 0 and (major.value, minor.value) >= (1, 10)
    header = open(N.HEADER_PATH).read()
    assert re.search(r"1\.10 = dcn_place_split_batch", header)
    assert int(re.search(r"#define DCN_ABI_MINOR (\d+)", header).group(1)) >= 10
    assert re.search(r"#define DCN_PLACE_SPLIT_MAX 8\b", header) and N.PLACE_SPLIT_MAX == 8
    assert "NOT a calibrated probability" in " ".join(header.replace(" *", " ").split())
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert int(re.search(r"pub const DCN_ABI_MINOR: u32 = (\d+); +//", md).group(1)) >= 10
    assert re.search(r"pub fn %s\(" % NAME, md)
    assert hasattr(dcn.Placer, "place_split_batch") and hasattr(dcn.Placer, "place_split")


def test_struct_layouts(dcn):
    N = dcn._native
    P, B = N.PlaceSplitParams, N.SplitPlacement
    assert C.sizeof(P) == 32 and C.sizeof(B) == 64
    assert (P.band_bases.offset, P.min_votes.offset, P.prefix_length.offset, P.max_placements.offset, P.reserved.offset) == \
        (0, 4, 8, 16, 20)
    assert [getattr(B, f).offset for f, _ in B._fields_] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 52, 56, 60]
    dt, one = dcn.filter.SPLIT_PLACEMENT_DTYPE, dcn.filter.PLACEMENT_DTYPE
    assert dt.itemsize == 64 and list(dt.names) == [f for f, _ in B._fields_]
    assert [dt.fields[f][1] for f in dt.names] == [getattr(B, f).offset for f in dt.names]
    # the first 48 bytes are dcn_placement's, field for field
    assert list(dt.names[:len(one.names)]) == list(one.names)
    assert all(dt.fields[f] == one.fields[f] for f in one.names)
    assert list(dt.names[len(one.names):]) == ["rank", "n_placed", "rival_votes", "mapq"]
    header = open(N.HEADER_PATH).read()
    assert re.search(r"\}\s*dcn_place_split_params;\s*/\* 32 bytes \*/", header)
    assert re.search(r"\}\s*dcn_split_placement;\s*/\* 64 bytes \*/", header)


def test_header_structs_in_c(tmp_path, dcn):
    src = tmp_path / "t.c"
    src.write_text('#include "deacon_hip.h"\n#include <stddef.h>\n'
                   "int main(void){ return sizeof(dcn_place_split_params) == 32 && sizeof(dcn_split_placement) == 64 && "
                   "offsetof(dcn_place_split_params, max_placements) == 16 && offsetof(dcn_place_split_params, reserved) == 20 && "
                   "offsetof(dcn_split_placement, read_start) == offsetof(dcn_placement, read_start) && "
                   "offsetof(dcn_split_placement, ref_end) == offsetof(dcn_placement, ref_end) && "
                   "offsetof(dcn_split_placement, rank) == sizeof(dcn_placement) && offsetof(dcn_split_placement, mapq) == 60 "
                   "? 0 : 1; }\n")
    inc = os.path.dirname(dcn._native.HEADER_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, str(src), "-o", str(tmp_path / "t")])
    assert subprocess.call([str(tmp_path / "t")]) == 0


def test_argument_errors_that_need_no_device(dcn):
    """params are judged first, then the pointers: nothing here is dereferenced"""
    N, L = dcn._native, dcn._native.lib()

    def prm(band=256, votes=2, n=4, r=(0, 0, 0)):
        return C.byref(N.PlaceSplitParams(band, votes, 0, n, (C.c_uint32 * 3)(*r)))

    po = (C.c_uint64 * 2)()
    stand_in = (C.c_uint8 * 4096)()

    def call(ctx, map_, params, offsets=po):
        return L.dcn_place_split_batch(ctx, map_, None, None, 0, params, offsets, None, 0, None)

    for args, word in (((None, None, None), b"params is NULL"),
                       ((None, None, prm(r=(1, 0, 0))), b"reserved"),
                       ((None, None, prm(r=(0, 1, 0))), b"reserved"),
                       ((None, None, prm(r=(0, 0, 1))), b"reserved"),
                       ((None, None, prm(band=0)), b"band_bases"),
                       ((None, None, prm(votes=0)), b"min_votes"),
                       ((None, None, prm(n=0)), b"max_placements must be 1..8"),
                       ((None, None, prm(n=9)), b"max_placements must be 1..8"),
                       ((None, None, prm(), None), b"place_offsets is NULL"),
                       ((None, None, prm()), b"ctx is NULL"),
                       ((C.cast(stand_in, C.c_void_p), None, prm()), b"map is NULL")):
        assert call(*args) == N.DCN_ERR_ARG
        assert word in L.dcn_last_error(), (word, L.dcn_last_error())


MAP_ERRORS = [
    (["map"], "the following required arguments were not provided: <REF>"),
    (["map", "ref.fa", "-N", "0"], "invalid value for -N: must be 1..8"),
    (["map", "ref.fa", "-N", "9"], "invalid value for -N: must be 1..8"),
    (["map", "ref.fa", "--max-placements", "x"], "invalid value for -N: must be 1..8"),
    (["map", "ref.fa", "--band", "0"], "invalid value for --band: must be 1..4294967295"),
    (["map", "ref.fa", "-a", "0"], "invalid value for --min-votes: must be 1..4294967295"),
    (["map", "ref.fa", "in1", "in2"],
     "map takes one input: mates are independent here, run it once per file (unexpected argument 'in2')"),
    (["map", "--nope"], "unexpected argument '--nope'"),
]


@pytest.mark.parametrize("args,message", MAP_ERRORS, ids=[" ".join(e[0]) for e in MAP_ERRORS])
def test_map_error_exit_code_and_text(args, message):
    p = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    assert (p.returncode, p.stdout, p.stderr) == (1, "", "Error: " + message + "\n")


def test_map_help_text():
    p = subprocess.run([CLI, "map", "--help"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    with open(os.path.join(ROOT, "tests", "golden", "cli_help", "map.txt")) as f:
        want = f.read()
    assert (p.returncode, p.stderr, p.stdout) == (0, "", want)
    for word in ("Usage: deacon-hip map [OPTIONS] <REF> [READS]", "-N, --max-placements <N>", "a convention, not a calibrated probability",
                 "[default: 256, a convention]", "cm votes"):
        assert word in want, word
    top = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert "\n  map " in top.stdout + top.stderr


def test_model_alone_on_random_chimeras(oracle):
    """THE ONE TEST HERE THAT PASSES WITHOUT THE FEATURE: it runs the model only.  Chimeras of two error-free parts of 80
    to 300 bases with an N between them, from random places and strands of three random genomes (k = 31, w = 15: every key an anchor): votes never
    rise with rank, rank 0 equals AnchorModel.place, the two parts are two placements that do not intersect on the read,
    so each has no rival and mapq 60, and with max_placements = 1 the other part is the unreported last round: still no
    rival, because its interval is disjoint."""
    O, k, w = oracle, 31, 15
    genomes = random_reads(np.random.default_rng(961), 3, 20_000, 20_000)
    model = PW.AnchorModel(O, k, w, O.Index.build(genomes, k=k, w=w).keys()).add(genomes)
    assert model.info()["repeats"] == 0
    rng = np.random.default_rng(962)
    for i in range(300):
        a, b = PW.cut(rng, genomes, 80, 300, 0), PW.cut(rng, genomes, 80, 300, 1 + i % 2)
        read = (revcomp(a) if i % 3 == 0 else a) + b"N" + (revcomp(b) if i % 5 == 0 else b)  # (no k-mer spans the N)
        for n in (1, 2, 4):
            rows, (n_anchors, n_pos) = SW.place_split(model, read, max_placements=n)
            votes = [r[2] for r in rows]
            assert votes == sorted(votes, reverse=True) and [r[9] for r in rows] == list(range(len(rows)))
            assert rows[0][:9] == model.place(read) and all(r[10] == len(rows) for r in rows)
            assert len(rows) == min(n, 2) and all(r[11] == 0 and r[12] == 60 for r in rows), (i, n, rows)
            assert sum(votes) <= n_anchors <= n_pos
        rows = SW.place_split(model, read, max_placements=2)[0]
        assert {r[0] for r in rows} == {0, 1 + i % 2}
        spans = sorted((r[5], r[6]) for r in rows)
        assert spans[0][1] <= len(a) < spans[1][0]
    # a weaker cell on the same stretch as a stronger one: part b replaces as many bases of a's record as it has
    g = genomes[0]
    read = g[1000:1200] + genomes[1][500:600] + g[1300:1500]
    rows = SW.place_split(model, read, max_placements=2)[0]
    assert [r[0] for r in rows] == [0, 1] and rows[0][12] > 0 and rows[1][11] == rows[0][2] and rows[1][12] == 0
    assert rows[0][11] == rows[1][2] and rows[0][12] == 60 * (rows[0][2] - rows[1][2]) // rows[0][2]

"""CPU checks of the anchor map's and dcn_place_batch's boundary: declared, exported and bound at ABI 1.9, the two
structs' layout, the argument errors that are found before a device is looked at, and the model of the GPU tests
(tests/_place_worker.py) against what an error-free read must give."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import _place_worker as PW
from conftest import random_reads, revcomp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dcn_anchor_map_create", "dcn_anchor_map_add", "dcn_anchor_map_info", "dcn_anchor_map_anchors", "dcn_place_batch")


def test_symbols_are_declared_exported_and_bound(dcn):
    N = dcn._native
    L = C.CDLL(N.LIB_PATH)
    for name in SYMBOLS:
        assert name in N.declared_symbols() and name in N._SIGNATURES and hasattr(L, name), name
    assert tuple(N.ABI) >= (1, 9)
    major, minor = C.c_uint32(), C.c_uint32()
    assert N.lib().dcn_abi_version(C.byref(major), C.byref(minor)) == 0 and (major.value, minor.value) >= (1, 9)
    header = open(N.HEADER_PATH).read()
    assert re.search(r"1\.9 = dcn_anchor_map_create", header)
    assert int(re.search(r"#define DCN_ABI_MINOR (\d+)", header).group(1)) >= 9
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert int(re.search(r"pub const DCN_ABI_MINOR: u32 = (\d+); +//", md).group(1)) >= 9
    for name in SYMBOLS:
        assert re.search(r"pub fn %s\(" % name, md), name
    for cls in ("AnchorMap", "Placer"):
        assert getattr(dcn, cls) is getattr(dcn.filter, cls) and cls in dcn.__all__


def test_struct_layouts(dcn):
    N = dcn._native
    P, B = N.PlaceParams, N.Placement
    assert C.sizeof(P) == 24 and C.sizeof(B) == 48
    assert (P.band_bases.offset, P.min_votes.offset, P.prefix_length.offset, P.reserved.offset) == (0, 4, 8, 16)
    assert [getattr(B, f).offset for f, _ in B._fields_] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40]
    dt = dcn.filter.PLACEMENT_DTYPE
    assert dt.itemsize == 48 and [dt.fields[f][1] for f in dt.names] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40]
    assert list(dt.names) == [f for f, _ in B._fields_]
    header = open(N.HEADER_PATH).read()
    assert re.search(r"\}\s*dcn_place_params;\s*/\* 24 bytes \*/", header)
    assert re.search(r"\}\s*dcn_placement;\s*/\* 48 bytes \*/", header)


def test_header_structs_in_c(tmp_path, dcn):
    src = tmp_path / "t.c"
    src.write_text('#include "deacon_hip.h"\n#include <stddef.h>\n'
                   "int main(void){ return sizeof(dcn_place_params) == 24 && sizeof(dcn_placement) == 48 && "
                   "offsetof(dcn_place_params, prefix_length) == 8 && offsetof(dcn_place_params, reserved) == 16 && "
                   "offsetof(dcn_placement, read_start) == 20 && offsetof(dcn_placement, ref_start) == 32 ? 0 : 1; }\n")
    inc = os.path.dirname(dcn._native.HEADER_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, str(src), "-o", str(tmp_path / "t")])
    assert subprocess.call([str(tmp_path / "t")]) == 0


def test_argument_errors_that_need_no_device(dcn):
    """params are judged first, then the pointers: nothing here is dereferenced"""
    N, L = dcn._native, dcn._native.lib()

    def prm(band=256, votes=2, r0=0, r1=0):
        return C.byref(N.PlaceParams(band, votes, 0, (C.c_uint32 * 2)(r0, r1)))

    def call(ctx, map_, params):
        return L.dcn_place_batch(ctx, map_, None, None, 0, params, None)

    stand_in = (C.c_uint8 * 4096)()
    for args, word in (((None, None, None), b"params is NULL"),
                       ((None, None, prm(r0=1)), b"reserved"),
                       ((None, None, prm(r1=1)), b"reserved"),
                       ((None, None, prm(band=0)), b"band_bases"),
                       ((None, None, prm(votes=0)), b"min_votes"),
                       ((None, None, prm()), b"ctx is NULL"),
                       ((C.cast(stand_in, C.c_void_p), None, prm()), b"map is NULL")):
        assert call(*args) == N.DCN_ERR_ARG
        assert word in L.dcn_last_error(), (word, L.dcn_last_error())
    h, n = C.c_void_p(), C.c_uint64(7)
    assert L.dcn_anchor_map_create(None, C.byref(h)) == N.DCN_ERR_ARG and b"index is NULL" in L.dcn_last_error()
    assert L.dcn_anchor_map_create(None, None) == N.DCN_ERR_ARG and b"out is NULL" in L.dcn_last_error()
    assert L.dcn_anchor_map_add(None, None, None, None, 0, None) == N.DCN_ERR_ARG and b"map is NULL" in L.dcn_last_error()
    assert L.dcn_anchor_map_info(None, None, None, None, None) == N.DCN_ERR_ARG
    assert L.dcn_anchor_map_anchors(None, None, None, None, 0, C.byref(n)) == N.DCN_ERR_ARG


def test_model_places_every_error_free_read(oracle):
    """three random genomes of 20 kbp at k = 31, w = 15: a repeated canonical 31-mer has probability around 1e-10, so
    every key is an anchor, and every error-free read of 100 to 300 bases is placed on its record and strand with every
    position voting, at the coordinates it was cut from.  Cuts: both ends of every record, and 400 random ones a strand."""
    O, k, w = oracle, 31, 15
    genomes = random_reads(np.random.default_rng(921), 3, 20_000, 20_000)
    model = PW.AnchorModel(O, k, w, O.Index.build(genomes, k=k, w=w).keys()).add(genomes)
    info = model.info()
    assert info["repeats"] == 0 and info["anchors"] == info["keys"] > 5000 and info["records"] == 3
    rng = np.random.default_rng(922)
    cuts = [(R, at, ln) for R in range(3) for ln in (100, 300) for at in (0, 20_000 - ln)]
    for _ in range(400):
        ln = int(rng.integers(100, 301))
        cuts.append((int(rng.integers(0, 3)), int(rng.integers(0, 20_000 - ln + 1)), ln))
    for R, at, ln in cuts:
        fwd = genomes[R][at:at + ln]
        for reverse, read in ((0, fwd), (1, revcomp(fwd))):
            rec, rev, votes, n_anchors, n_pos, q0, q1, p0, p1 = model.place(read, W=256, min_votes=2)
            assert (rec, rev) == (R, reverse), (R, at, ln, reverse)
            assert votes == n_anchors == n_pos >= 2
            if not reverse:
                assert p0 - q0 == at and p1 - q1 == at
            else:
                assert p1 + q0 == at + ln and p0 + q1 == at + ln
            assert 0 <= q0 < q1 <= ln and at <= p0 < p1 <= at + ln

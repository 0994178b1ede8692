"""CPU checks of dcn_depth_track_batch's boundary: declared, exported and bound at ABI 1.8, the two structs' layout, the
argument errors that are found before a context or a set is looked at, and the classify command's --track flags."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "deacon-server_amd", "bin", "deacon-hip")


def test_symbol_is_declared_exported_and_bound(dcn):
    N = dcn._native
    assert "dcn_depth_track_batch" in N.declared_symbols() and "dcn_depth_track_batch" in N._SIGNATURES
    assert N._SIGNATURES["dcn_depth_track_batch"] == N._SIGNATURES["dcn_locate_batch"]  # the same shape of call
    assert hasattr(C.CDLL(N.LIB_PATH), "dcn_depth_track_batch")
    assert tuple(N.ABI) >= (1, 8)
    major, minor = C.c_uint32(), C.c_uint32()
    assert N.lib().dcn_abi_version(C.byref(major), C.byref(minor)) == 0 and (major.value, minor.value) >= (1, 8)
    header = open(N.HEADER_PATH).read()
    assert re.search(r"1\.8 = dcn_depth_track_batch", header)
    assert int(re.search(r"#define DCN_ABI_MINOR (\d+)", header).group(1)) >= 8
    assert dcn.DepthTracker is dcn.filter.DepthTracker and "DepthTracker" in dcn.__all__


def test_struct_layouts(dcn):
    N = dcn._native
    P, B = N.TrackParams, N.TrackBin
    assert C.sizeof(P) == 24 and C.sizeof(B) == 24
    assert (P.bin_bases.offset, P.member_mask.offset, P.depth_cap.offset, P.reserved.offset, P.prefix_length.offset) == (0, 4, 8, 12, 16)
    assert (B.n_positions.offset, B.n_keys.offset, B.n_observed.offset, B.max_depth.offset, B.sum_depth.offset) == (0, 4, 8, 12, 16)
    dt = dcn.filter.TRACK_BIN_DTYPE
    assert dt.itemsize == 24 and [dt.fields[f][1] for f in dt.names] == [0, 4, 8, 12, 16]
    assert list(dt.names) == ["n_positions", "n_keys", "n_observed", "max_depth", "sum_depth"]
    header = open(N.HEADER_PATH).read()
    for name in ("dcn_track_params", "dcn_track_bin"):
        assert re.search(r"\}\s*%s;\s*/\* 24 bytes \*/" % name, header)


def test_header_structs_are_24_bytes_in_c(tmp_path, dcn):
    src = tmp_path / "t.c"
    src.write_text('#include "deacon_hip.h"\n#include <stddef.h>\n'
                   "int main(void){ return sizeof(dcn_track_params) == 24 && sizeof(dcn_track_bin) == 24 && "
                   "offsetof(dcn_track_params, prefix_length) == 16 && offsetof(dcn_track_bin, sum_depth) == 16 ? 0 : 1; }\n")
    inc = os.path.dirname(dcn._native.HEADER_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, str(src), "-o", str(tmp_path / "t")])
    assert subprocess.call([str(tmp_path / "t")]) == 0


def test_argument_errors_that_need_no_set(dcn):
    """params are judged first, then the pointers: nothing here is dereferenced (the stand-in for a context is a zeroed
    buffer that the call returns in front of)"""
    N, L = dcn._native, dcn._native.lib()
    stand_in = (C.c_uint8 * 4096)()
    bo = np.zeros(2, np.uint64)
    bop = bo.ctypes.data_as(C.c_void_p)

    def call(ctx, set_, params, bin_offsets):
        return L.dcn_depth_track_batch(ctx, set_, None, None, 0, params, bin_offsets, None, 0)

    ok = N.TrackParams(1000, 1, 0, 0, 0)
    for args, word in (((None, None, None, bop), b"params is NULL"),
                       ((None, None, C.byref(N.TrackParams(1000, 1, 0, 1, 0)), bop), b"reserved"),
                       ((None, None, C.byref(N.TrackParams(1000, 0, 0, 0, 0)), bop), b"member_mask"),
                       ((None, None, C.byref(N.TrackParams(1000, 1, 65536, 0, 0)), bop), b"depth_cap"),
                       ((None, None, C.byref(ok), None), b"bin_offsets is NULL"),
                       ((None, None, C.byref(ok), bop), b"ctx is NULL"),
                       ((C.cast(stand_in, C.c_void_p), None, C.byref(ok), bop), b"set is NULL")):
        assert call(*args) == N.DCN_ERR_ARG
        assert word in L.dcn_last_error(), (word, L.dcn_last_error())
    assert not bo.any()


def test_classify_help_lists_the_track_flags():
    out = subprocess.run([CLI, "classify", "--help"], capture_output=True, text=True, timeout=60)
    text = out.stdout + out.stderr
    for flag in ("--track <FASTX>", "--track-out <PATH>", "--track-bin <N>", "--track-cap <N>"):
        assert flag in text

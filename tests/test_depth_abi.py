"""CPU checks of the depth surface (dcn_index_set_depth_*, ABI 1.6): the five entry points are declared, exported and
bound, argument errors return DCN_ERR_ARG with a message before any device work, and `classify --help` lists the flags.
(Without a device no set can be made: the errors of a real set -- not enabled, member or n_bins out of range -- are in
tests/test_gpu_depth.py.)"""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "deacon-server_amd", "bin", "deacon-hip")
NAMES = ("dcn_index_set_depth_enable", "dcn_index_set_depth_reset", "dcn_index_set_depth_stats",
         "dcn_index_set_depth_hist", "dcn_index_set_depth_keys")


def test_depth_entry_points_are_declared_exported_and_bound_at_abi_1_6(dcn):
    N = dcn._native
    L = C.CDLL(N.LIB_PATH)
    for name in NAMES:
        assert name in N.declared_symbols() and name in N._SIGNATURES and hasattr(L, name)
    assert tuple(N.ABI) >= (1, 6)
    header = open(N.HEADER_PATH).read()
    major = int(re.search(r"#define DCN_ABI_MAJOR (\d+)", header).group(1))
    minor = int(re.search(r"#define DCN_ABI_MINOR (\d+)", header).group(1))
    assert (major, minor) >= (1, 6)
    a, b = C.c_uint32(), C.c_uint32()
    assert N.lib().dcn_abi_version(C.byref(a), C.byref(b)) == 0 and (a.value, b.value) >= (1, 6)
    assert "1.6 = dcn_index_set_depth_enable / _reset / _stats / _hist / _keys" in header
    assert len(N.declared_symbols()) >= 65


def test_depth_argument_errors(dcn):
    L, N = dcn._native.lib(), dcn._native
    u64 = (C.c_uint64 * 4096)()
    u32 = (C.c_uint32 * 4)()
    n = C.c_uint64(7)
    calls = [
        lambda: L.dcn_index_set_depth_enable(None, 1),
        lambda: L.dcn_index_set_depth_enable(None, 0),
        lambda: L.dcn_index_set_depth_reset(None),
        lambda: L.dcn_index_set_depth_stats(None, u64, u64, u64),
        lambda: L.dcn_index_set_depth_stats(None, None, None, None),
        lambda: L.dcn_index_set_depth_hist(None, 0, 256, u64),
        lambda: L.dcn_index_set_depth_hist(None, 0xFFFFFFFF, 1, None),
        lambda: L.dcn_index_set_depth_hist(None, 40, 5000, u64),
        lambda: L.dcn_index_set_depth_keys(None, 0, u64, u32, 4, C.byref(n)),
        lambda: L.dcn_index_set_depth_keys(None, 0xFFFFFFFF, None, None, 0, None),
    ]
    for call in calls:
        assert call() == N.DCN_ERR_ARG
        assert b"set is NULL" in L.dcn_last_error()


def test_python_binding_raises(dcn):
    s = dcn.IndexSet.__new__(dcn.IndexSet)  # a set object without a handle: the library refuses it, nothing aborts
    s._h, s.n = None, 3
    for call in (s.enable_depth, s.reset_depth, s.depth_stats, s.depth_hist, lambda: s.depth_hist(1, 2), s.depth_keys,
                 lambda: s.depth_keys(2)):
        try:
            call()
        except dcn.DeaconHipError as e:
            assert e.code == dcn._native.DCN_ERR_ARG and "NULL" in e.message
        else:
            raise AssertionError("no error")


def test_classify_help_lists_depth():
    p = subprocess.run([CLI, "classify", "--help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0
    assert "--depth " in p.stdout and "--depth-hist" in p.stdout

"""CPU checks of the coverage surface (dcn_index_set_coverage*): argument errors return DCN_ERR_ARG with a message and
never abort, and `classify --help` lists --coverage."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "deacon-server_amd", "bin", "deacon-hip")


def test_coverage_entry_points_are_bound_at_abi_1_3(dcn):
    N = dcn._native
    for name in ("dcn_index_set_coverage_enable", "dcn_index_set_coverage_reset", "dcn_index_set_coverage",
                 "dcn_index_set_coverage_keys"):
        assert name in N.declared_symbols() and name in N._SIGNATURES
    assert tuple(N.ABI) >= (1, 3)


def test_coverage_argument_errors(dcn):
    L, N = dcn._native.lib(), dcn._native
    obs, keys = (C.c_uint64 * 32)(), (C.c_uint64 * 32)()
    n = C.c_uint64(7)
    out = (C.c_uint64 * 4)()
    calls = [
        lambda: L.dcn_index_set_coverage_enable(None, 1),
        lambda: L.dcn_index_set_coverage_enable(None, 0),
        lambda: L.dcn_index_set_coverage_reset(None),
        lambda: L.dcn_index_set_coverage(None, obs, keys),
        lambda: L.dcn_index_set_coverage(None, None, None),
        lambda: L.dcn_index_set_coverage_keys(None, 0, out, 4, C.byref(n)),
        lambda: L.dcn_index_set_coverage_keys(None, 0xFFFFFFFF, None, 0, None),
    ]
    for call in calls:
        assert call() == N.DCN_ERR_ARG
        assert b"set is NULL" in L.dcn_last_error()


def test_python_binding_raises(dcn):
    s = dcn.IndexSet.__new__(dcn.IndexSet)  # a set object without a handle: the library refuses it, nothing aborts
    s._h, s.n = None, 3
    for call in (s.enable_coverage, s.reset_coverage, s.coverage, s.observed_keys, lambda: s.observed_keys(2)):
        try:
            call()
        except dcn.DeaconHipError as e:
            assert e.code == dcn._native.DCN_ERR_ARG and "NULL" in e.message
        else:
            raise AssertionError("no error")


def test_classify_help_lists_coverage():
    p = subprocess.run([CLI, "classify", "--help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0
    assert "--coverage" in p.stdout

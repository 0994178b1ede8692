"""CPU checks of the set-algebra surface (no GPU): dcn_index_set_select, dcn_index_set_overlap and dcn_index_intersect are
declared, exported and bound at ABI 1.5, refuse bad arguments with a code and a message instead of aborting, fail loudly
without a GPU, and `deacon-hip index intersect / compare / select` are listed, document their options and name what is
wrong with a command line before they touch a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CLI = os.path.join(ROOT, "deacon-server_amd", "bin", "deacon-hip")
CALLS = ("dcn_index_set_select", "dcn_index_set_overlap", "dcn_index_intersect")


def test_symbols_declared_exported_bound_and_abi_minor(dcn):
    N = dcn._native
    L = C.CDLL(N.LIB_PATH)
    for name in CALLS:
        assert name in N.declared_symbols(), name
        assert name in N._SIGNATURES, name
        assert hasattr(L, name), name
    a, b = C.c_uint32(), C.c_uint32()
    assert N.lib().dcn_abi_version(C.byref(a), C.byref(b)) == 0
    assert a.value == 1 and b.value >= 5
    assert tuple(N.ABI) >= (1, 5)
    assert hasattr(dcn.Index, "intersect") and hasattr(dcn.IndexSet, "select") and hasattr(dcn.IndexSet, "overlap")


def test_header_history_names_the_new_calls(dcn):
    text = open(dcn._native.HEADER_PATH).read()
    assert "1.5 = dcn_index_set_select / _overlap, dcn_index_intersect" in text


def test_null_and_argument_errors_do_not_abort(dcn):
    """everything here is decided before an index is looked at: no device work, no GPU needed"""
    N = dcn._native
    L = N.lib()
    n = C.c_uint64(7)
    h = C.c_void_p(1)
    arr = np.zeros(4, np.uint64)
    p = arr.ctypes.data_as(C.c_void_p)
    # select
    assert L.dcn_index_set_select(None, 0, 0, 0, 0, 0, None, None) == N.DCN_ERR_ARG
    assert b"both NULL" in L.dcn_last_error()
    assert L.dcn_index_set_select(None, 0, 0, 0, 0, 0, C.byref(n), C.byref(h)) == N.DCN_ERR_ARG
    assert b"set is NULL" in L.dcn_last_error()
    assert n.value == 0 and not h.value  # outputs are cleared on failure
    assert L.dcn_index_set_select(None, 0, 0, 0, 3, 2, C.byref(n), None) == N.DCN_ERR_ARG
    assert b"min_members" in L.dcn_last_error()
    # overlap
    assert L.dcn_index_set_overlap(None, None, None, None) == N.DCN_ERR_ARG
    assert b"all NULL" in L.dcn_last_error()
    assert L.dcn_index_set_overlap(None, p, p, p) == N.DCN_ERR_ARG
    assert b"set is NULL" in L.dcn_last_error()
    # intersect
    one = (C.c_void_p * 1)(None)
    assert L.dcn_index_intersect(one, 1, None) == N.DCN_ERR_ARG
    assert b"out is NULL" in L.dcn_last_error()
    h = C.c_void_p(1)
    assert L.dcn_index_intersect(None, 1, C.byref(h)) == N.DCN_ERR_ARG and not h.value
    assert L.dcn_index_intersect(one, 0, C.byref(h)) == N.DCN_ERR_ARG
    assert L.dcn_index_intersect(one, 1, C.byref(h)) == N.DCN_ERR_ARG
    assert b"at least one input" in L.dcn_last_error()


def test_python_mask_arguments(dcn):
    """masks are ints or iterables of member numbers; what cannot be a u32 mask is refused before the library is called"""
    s = object.__new__(dcn.IndexSet)  # (no set without a GPU: _mask needs none)
    s._h = None
    assert s._mask(0) == 0 and s._mask(5) == 5 and s._mask([0, 2]) == 5 and s._mask({31}) == 1 << 31 and s._mask(()) == 0
    for bad in (-1, 1 << 32, [32], [-1]):
        with pytest.raises(ValueError):
            s._mask(bad)


def test_no_gpu_means_loud_failure_not_fallback(dcn):
    L = dcn._native.lib()
    n = C.c_int(-1)
    rc = L.dcn_device_count(C.byref(n))
    if rc == 0 and n.value > 0:
        pytest.skip("a GPU is present")
    # no index can exist without a device, so the three calls are reached through the ones that make their operands:
    # each ends in an error code with a message, not in a host-side answer
    keys = np.arange(1, 100, dtype=np.uint64)
    for make in (lambda: dcn.Index.intersect([dcn.Index.from_keys(keys)]),
                 lambda: dcn.IndexSet([dcn.Index.from_keys(keys)]).select(count_only=True),
                 lambda: dcn.IndexSet([dcn.Index.from_keys(keys)]).overlap()):
        with pytest.raises(dcn.DeaconHipError) as e:
            make()
        assert e.value.code in (dcn._native.DCN_ERR_HIP, dcn._native.DCN_ERR_ARG) and e.value.message


def _run(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=120)


def test_help_lists_the_subcommands_and_their_options():
    p = _run("index", "--help")
    assert p.returncode == 0
    for word in ("intersect", "compare", "select", "union", "diff"):
        assert word in p.stdout, word
    p = _run("index", "intersect", "--help")
    assert p.returncode == 0 and "Usage: deacon-hip index intersect" in p.stdout and "-o, --output" in p.stdout
    p = _run("index", "compare", "--help")
    assert p.returncode == 0 and "Usage: deacon-hip index compare" in p.stdout
    for word in ("-s, --summary", "containment", "jaccard", "2 to 32"):
        assert word in p.stdout, word
    p = _run("index", "select", "--help")
    assert p.returncode == 0 and "Usage: deacon-hip index select" in p.stdout
    for opt in ("-x, --index", "--all <LIST>", "--any <LIST>", "--none <LIST>", "--min-members", "--max-members", "-o, --output",
                "--all 0 --max-members 1", "--min-members m"):
        assert opt in p.stdout, opt


def test_command_line_errors_name_the_problem(tmp_path):
    a, b = str(tmp_path / "a.idx"), str(tmp_path / "b.idx")
    for bad in ("0,x", "0,,1", "2", "-1", "1,", ""):
        p = _run("index", "select", "-x", a, "-x", b, "--all", bad, "-o", str(tmp_path / "o.idx"))
        assert p.returncode != 0 and "--all" in p.stderr, (bad, p.stderr)
    p = _run("index", "select", "-x", a, "--none", "7")
    assert p.returncode != 0 and "--none" in p.stderr and "position 7" in p.stderr
    p = _run("index", "select", "--all", "0")
    assert p.returncode != 0 and "-x" in p.stderr
    p = _run("index", "select", "-x", a, "--min-members", "3", "--max-members", "2")
    assert p.returncode != 0 and "--min-members" in p.stderr
    p = _run("index", "compare", a)
    assert p.returncode != 0 and "2 to 32" in p.stderr
    p = _run("index", "compare", *([a] * 33))
    assert p.returncode != 0 and "2 to 32" in p.stderr
    p = _run("index", "intersect")
    assert p.returncode != 0 and "<INDEX>" in p.stderr
    p = _run("index", "intersect", a, "--frobnicate")
    assert p.returncode != 0 and "--frobnicate" in p.stderr

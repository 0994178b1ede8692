"""CPU checks of the index builder's surface (no GPU): the seven dcn_index_builder_* entry points are declared, exported,
bound at ABI 1.7 and present in INTEGRATION.md; every argument error returns DCN_ERR_ARG with a message before any device
work; the Python class raises on them; `deacon-hip index build --help` lists the three options."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CLI = os.path.join(ROOT, "deacon-server_amd", "bin", "deacon-hip")
CALLS = tuple("dcn_index_builder_" + s for s in ("create", "add", "info", "hist", "counts", "finish", "destroy"))


def test_symbols_declared_exported_bound_and_abi_minor(dcn):
    N = dcn._native
    L = C.CDLL(N.LIB_PATH)
    for name in CALLS:
        assert name in N.declared_symbols(), name
        assert name in N._SIGNATURES, name
        assert hasattr(L, name), name
    a, b = C.c_uint32(), C.c_uint32()
    assert N.lib().dcn_abi_version(C.byref(a), C.byref(b)) == 0
    assert a.value == 1 and b.value >= 7
    assert tuple(N.ABI) >= (1, 7)
    for method in ("add", "info", "hist", "counts", "finish", "close"):
        assert hasattr(dcn.IndexBuilder, method), method


def test_header_history_and_integration_md_name_the_calls(dcn):
    text = open(dcn._native.HEADER_PATH).read()
    assert "1.7 = dcn_index_builder_create / _add / _info / _hist / _counts / _finish / _destroy" in text
    assert "typedef struct dcn_index_builder dcn_index_builder;" in text
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in CALLS:
        assert f"pub fn {name}(" in md, name
    assert "pub const DCN_ABI_MINOR: u32 = 7;" in md


def test_argument_errors_come_before_any_device_work(dcn):
    """everything here is decided before a device is looked at: no GPU needed"""
    N = dcn._native
    L = N.lib()
    h = C.c_void_p(1)
    n = C.c_uint64(7)
    arr = np.zeros(8, np.uint64)
    p = arr.ctypes.data_as(C.c_void_p)
    # create: out, the k / w rule of every index, the entropy range
    assert L.dcn_index_builder_create(31, 15, 0.0, 0, 0, None) == N.DCN_ERR_ARG
    assert b"out is NULL" in L.dcn_last_error()
    assert L.dcn_index_builder_create(31, 16, 0.0, 0, 0, C.byref(h)) == N.DCN_ERR_ARG and not h.value
    assert b"odd" in L.dcn_last_error()
    for k, w in ((0, 2), (57, 15), (31, 0)):
        assert L.dcn_index_builder_create(k, w, 0.0, 0, 0, C.byref(h)) == N.DCN_ERR_ARG, (k, w)
    for e in (-0.1, 1.5, float("nan")):
        assert L.dcn_index_builder_create(31, 15, e, 0, 0, C.byref(h)) == N.DCN_ERR_ARG, e
        assert b"entropy_threshold" in L.dcn_last_error()
    # add, info
    assert L.dcn_index_builder_add(None, p, p, 1) == N.DCN_ERR_ARG
    assert b"builder is NULL" in L.dcn_last_error()
    assert L.dcn_index_builder_info(None, None, None, None, None) == N.DCN_ERR_ARG
    # hist
    assert L.dcn_index_builder_hist(None, 256, None) == N.DCN_ERR_ARG
    assert b"hist is NULL" in L.dcn_last_error()
    for bins in (0, 1, 4097):
        assert L.dcn_index_builder_hist(None, bins, p) == N.DCN_ERR_ARG
        assert b"n_bins" in L.dcn_last_error()
    assert L.dcn_index_builder_hist(None, 256, p) == N.DCN_ERR_ARG
    assert b"builder is NULL" in L.dcn_last_error()
    # counts
    assert L.dcn_index_builder_counts(None, p, p, 4, None) == N.DCN_ERR_ARG
    assert L.dcn_index_builder_counts(None, p, p, 4, C.byref(n)) == N.DCN_ERR_ARG and n.value == 0
    # finish: the bounds are judged before the builder
    assert L.dcn_index_builder_finish(None, 1, 0, None, None) == N.DCN_ERR_ARG
    assert b"both NULL" in L.dcn_last_error()
    h = C.c_void_p(1)
    n = C.c_uint64(7)
    assert L.dcn_index_builder_finish(None, 3, 2, C.byref(n), C.byref(h)) == N.DCN_ERR_ARG
    assert b"min_count 3 > max_count 2" in L.dcn_last_error()
    assert n.value == 0 and not h.value  # outputs are cleared on failure
    for lo, hi in ((65536, 0), (1, 65536)):
        assert L.dcn_index_builder_finish(None, lo, hi, C.byref(n), None) == N.DCN_ERR_ARG
        assert b"65535" in L.dcn_last_error()
    assert L.dcn_index_builder_finish(None, 1, 0, C.byref(n), None) == N.DCN_ERR_ARG
    assert b"builder is NULL" in L.dcn_last_error()
    L.dcn_index_builder_destroy(None)  # a no-op, must not crash


def test_python_class_raises(dcn):
    for kwargs in (dict(window_size=16), dict(kmer_length=57), dict(entropy_threshold=1.5), dict(entropy_threshold=-1)):
        with pytest.raises(dcn.DeaconHipError) as e:
            dcn.IndexBuilder(**kwargs)
        assert e.value.code == dcn._native.DCN_ERR_ARG and e.value.message
    with pytest.raises(ValueError):
        dcn.IndexBuilder(kmer_length=300)
    b = object.__new__(dcn.IndexBuilder)  # (no builder without a GPU: the range checks need none)
    b._h, b.device = None, 0
    for call in (lambda: b.finish(-1, 0), lambda: b.finish(1, 1 << 32), lambda: b.hist(-1)):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: b.finish(3, 2), lambda: b.finish(1, 65536), lambda: b.hist(1), lambda: b.hist(4097), lambda: b.info(),
                 lambda: b.add([b"ACGT"])):
        with pytest.raises(dcn.DeaconHipError) as e:
            call()
        assert e.value.code == dcn._native.DCN_ERR_ARG


def test_no_gpu_means_loud_failure_not_fallback(dcn):
    L = dcn._native.lib()
    n = C.c_int(-1)
    rc = L.dcn_device_count(C.byref(n))
    if rc == 0 and n.value > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(dcn.DeaconHipError) as e:
        dcn.IndexBuilder()
    assert e.value.code in (dcn._native.DCN_ERR_HIP, dcn._native.DCN_ERR_ARG) and e.value.message


def _run(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=120)


def test_help_lists_the_options_and_bad_values_are_named():
    p = _run("index", "build", "--help")
    assert p.returncode == 0 and "Usage: deacon-hip index build" in p.stdout
    for opt in ("--min-count <N>", "--max-count <N>", "--count-hist <FILE>", "batch by batch"):
        assert opt in p.stdout, opt
    for bad in ("0", "65536", "x", "-1", ""):
        p = _run("index", "build", "in.fa", "--min-count", bad)
        assert p.returncode != 0 and "--min-count" in p.stderr, (bad, p.stderr)
    p = _run("index", "build", "in.fa", "--min-count", "3", "--max-count", "2")
    assert p.returncode != 0 and "--min-count 3" in p.stderr and "--max-count 2" in p.stderr

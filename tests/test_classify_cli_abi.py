"""CPU checks of the classification surface: argument errors of the new entry points (DCN_ERR_ARG with a message, never
an abort), NULL destroys, and the `classify` subcommand's help and missing-index error."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "deacon-server_amd", "bin", "deacon-hip")


def test_index_set_argument_errors(dcn):
    L, N = dcn._native.lib(), dcn._native
    h = C.c_void_p()
    members = (C.c_void_p * 40)()
    assert L.dcn_index_set_create(members, 1, None) == N.DCN_ERR_ARG
    assert b"out is NULL" in L.dcn_last_error()
    assert L.dcn_index_set_create(None, 1, C.byref(h)) == N.DCN_ERR_ARG
    assert b"members is NULL" in L.dcn_last_error()
    assert L.dcn_index_set_create(members, 0, C.byref(h)) == N.DCN_ERR_ARG
    assert b"1 to 32 members" in L.dcn_last_error()
    assert L.dcn_index_set_create(members, 33, C.byref(h)) == N.DCN_ERR_ARG
    assert b"1 to 32 members" in L.dcn_last_error()
    assert L.dcn_index_set_create(members, 2, C.byref(h)) == N.DCN_ERR_ARG  # NULL member
    assert b"NULL" in L.dcn_last_error()
    assert not h.value
    n = C.c_uint32()
    assert L.dcn_index_set_info(None, C.byref(n), None, None, None, None) == N.DCN_ERR_ARG
    assert b"set is NULL" in L.dcn_last_error()
    L.dcn_index_set_destroy(None)  # no-op


def test_classify_argument_errors(dcn):
    L, N = dcn._native.lib(), dcn._native
    prm = N.Params(2, 0.01, 0, 0, 0)
    b = (C.c_uint8 * 4)(*b"ACGT")
    o = (C.c_uint64 * 2)(0, 4)
    m, hh, t = (C.c_uint32 * 1)(), (C.c_uint32 * 1)(), (C.c_uint32 * 1)()
    assert L.dcn_classify_batch(None, None, b, o, None, 1, C.byref(prm), m, hh, t) == N.DCN_ERR_ARG
    assert b"ctx is NULL" in L.dcn_last_error()
    assert L.dcn_classify_batch_device(None, None, b, o, None, 1, 4, 1, C.byref(prm), m, hh, t) == N.DCN_ERR_ARG
    assert b"ctx is NULL" in L.dcn_last_error()


def test_classify_help_lists_options():
    p = subprocess.run([CLI, "classify", "--help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0
    for opt in ("-x, --index", "-a, --abs-threshold", "-r, --rel-threshold", "-p, --prefix-length", "--per-read",
                "-s, --summary", "-t, --threads", "-q, --quiet", "[INPUT2]"):
        assert opt in p.stdout, opt
    top = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert "classify" in top.stderr + top.stdout


def test_classify_missing_index_fails_loudly(tmp_path):
    fq = tmp_path / "reads.fq"
    fq.write_text("@r1\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n")
    p = subprocess.run([CLI, "classify", "-x", str(tmp_path / "missing.idx"), str(fq)], capture_output=True, text=True,
                       timeout=60)
    assert p.returncode != 0
    assert "missing.idx" in p.stderr
    p = subprocess.run([CLI, "classify", str(fq)], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "-x" in p.stderr

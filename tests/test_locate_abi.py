"""CPU checks of the locate surface (no GPU): dcn_locate_batch is exported and bound, refuses bad arguments with a code and
a message instead of aborting, and `deacon-hip mask` is listed, documents its options and names what is wrong with a
command line before it touches a device."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT

CLI = os.path.join(ROOT, "deacon-server_amd", "bin", "deacon-hip")


def test_symbol_binding_and_abi_minor(dcn):
    N = dcn._native
    assert "dcn_locate_batch" in N.declared_symbols() and "dcn_locate_batch" in N._SIGNATURES
    a, b = C.c_uint32(), C.c_uint32()
    assert N.lib().dcn_abi_version(C.byref(a), C.byref(b)) == 0
    assert a.value == 1 and b.value >= 4
    assert tuple(N.ABI) >= (1, 4)
    assert hasattr(dcn, "Locator")


def test_struct_layouts_match_the_header(dcn, tmp_path):
    P = dcn._native.LocateParams
    assert C.sizeof(P) == 24
    assert (P.max_gap.offset, P.min_hits.offset, P.member_mask.offset, P.reserved.offset, P.prefix_length.offset) == (0, 4, 8, 12, 16)
    S = dcn.filter.SEGMENT_DTYPE
    assert S.itemsize == 16 and S.names == ("start", "end", "n_hits", "members")
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "deacon_hip.h"\n'
                   "int main(void){ dcn_locate_params p; dcn_segment s; (void)p; (void)s;\n"
                   "  return sizeof(dcn_locate_params) == 24 && offsetof(dcn_locate_params, prefix_length) == 16 &&\n"
                   "         sizeof(dcn_segment) == 16 && offsetof(dcn_segment, members) == 12 ? 0 : 1; }\n")
    inc = os.path.dirname(dcn._native.HEADER_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, str(src), "-o", str(tmp_path / "t")])
    assert subprocess.call([str(tmp_path / "t")]) == 0


def test_argument_errors_do_not_abort(dcn):
    N = dcn._native
    L = N.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    bases = np.frombuffer(b"ACGT" * 30, np.uint8).copy()
    offsets = np.array([0, len(bases)], np.uint64)
    so = np.zeros(2, np.uint64)
    good = N.LocateParams(29, 1, 0xFFFFFFFF, 0, 0)
    fake = C.c_void_p(0)  # there is no context without a GPU: every refusal below comes before one is looked at

    def call(ctx, index, params, seg_offsets):
        return L.dcn_locate_batch(ctx, index, ptr(bases), ptr(offsets), 1, params, seg_offsets, None, 0)

    assert call(None, None, C.byref(good), ptr(so)) == N.DCN_ERR_ARG
    assert b"ctx is NULL" in L.dcn_last_error()
    assert call(fake, None, None, ptr(so)) == N.DCN_ERR_ARG
    assert b"params is NULL" in L.dcn_last_error()
    assert call(None, None, C.byref(good), None) == N.DCN_ERR_ARG
    assert b"seg_offsets is NULL" in L.dcn_last_error()
    assert call(None, None, C.byref(N.LocateParams(29, 0, 0xFFFFFFFF, 0, 0)), ptr(so)) == N.DCN_ERR_ARG
    assert b"min_hits" in L.dcn_last_error()
    assert call(None, None, C.byref(N.LocateParams(29, 1, 0xFFFFFFFF, 1, 0)), ptr(so)) == N.DCN_ERR_ARG
    assert b"reserved" in L.dcn_last_error()


def _run(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=120)


def test_help_lists_mask_and_its_options():
    p = _run("--help")
    assert p.returncode == 0 and "mask" in p.stdout + p.stderr
    p = _run("mask", "--help")
    assert p.returncode == 0
    for opt in ("-x, --index", "-o, --output", "--bed", "--soft", "-g, --max-gap", "-a, --min-hits", "-p, --prefix-length",
                "-s, --summary", "-t, --threads", "-q, --quiet"):
        assert opt in p.stdout, opt
    assert "default: 2" in p.stdout and "2*w - 1" in p.stdout


def test_command_line_errors_name_the_problem(tmp_path):
    missing = str(tmp_path / "missing.idx")
    fq = tmp_path / "r.fq"
    fq.write_text("@r\nACGT\n+\nIIII\n")
    p = _run("mask", "-x", missing, str(fq), "-o", str(tmp_path / "o.fq"))
    assert p.returncode != 0 and "missing.idx" in p.stderr
    p = _run("mask", "-x", missing, str(fq))
    assert p.returncode != 0 and "-o" in p.stderr and "--bed" in p.stderr and "-s" in p.stderr
    p = _run("mask", str(fq), "-o", str(tmp_path / "o.fq"))
    assert p.returncode != 0 and "-x" in p.stderr
    p = _run("mask", "-x", missing, str(fq), str(fq), "-o", str(tmp_path / "o.fq"))
    assert p.returncode != 0 and "one input" in p.stderr
    p = _run("mask", "-x", missing, str(fq), "-a", "0", "-o", str(tmp_path / "o.fq"))
    assert p.returncode != 0 and "--min-hits" in p.stderr
    p = _run("mask", "-x", missing, str(fq), "--frobnicate")
    assert p.returncode != 0 and "--frobnicate" in p.stderr

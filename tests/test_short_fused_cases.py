"""CPU: the batches of tests/test_gpu_short_fused.py hold every case they are there for, by the oracle alone; and the ASCII
-> 2-bit / invalid-bit helpers that pack.hip and scan.hip share (csrc/dcn_pack.h) against a byte-by-byte model."""
import os
import subprocess

import numpy as np
import pytest

import _short_fused_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def world(oracle):
    g = SC.genome()
    return g, oracle.Index.build([g], k=SC.K, w=SC.W)


def test_seam_batch_holds_its_cases(oracle, world):
    g, oidx = world
    reads = SC.seam_batch(g)
    lens = np.array([len(r) for r in reads])
    assert len(reads) == 2 * 2048 + 17 and lens.max() == SC.LMAX
    for ln in (0, 10, 30, 31, 44, 45, 46, 100, SC.LMAX):
        assert (lens == ln).any(), ln
    tiled = lens >= SC.L
    for b0 in range(0, len(reads), SC.PLAN_BLOCK):  # every planning block: reads without a tile, and a range that is no multiple of 64
        blk = tiled[b0:b0 + SC.PLAN_BLOCK]
        assert (~blk).any() and blk.any()
    assert any(tiled[b0:b0 + SC.PLAN_BLOCK].sum() % 64 for b0 in range(0, len(reads), SC.PLAN_BLOCK))
    assert tiled.sum() % 64 != 0  # the last wave is partial
    assert tiled[600:760].sum() < 64  # a wave of several runs
    b, o = oracle.concat_reads(reads)
    for abs_t, rel_t, deplete in SC.THRESHOLDS:
        keep, hits, total = oracle.filter_batch(oidx, b, o, abs_threshold=abs_t, rel_threshold=rel_t, deplete=deplete, threads=4)
        assert keep[tiled].any() and not keep[tiled].all(), (abs_t, rel_t, deplete)
    _, hits, total = oracle.filter_batch(oidx, b, o, threads=4)
    assert total.max() > 40  # more minimizers than a lane's list holds between flushes
    assert hits[2000] == total[2000] > 0
    assert any(r[:1] == b"N" for r in reads) and any(r[-1:] == b"N" for r in reads)
    assert any(r[:2].islower() for r in reads if len(r) > 3) and any(r[-2:].islower() for r in reads if len(r) > 3)


def test_newline_batch_holds_its_cases(oracle, world):
    g, oidx = world
    reads = SC.newline_batch(g)
    b, o = oracle.concat_reads(reads)
    assert b[-1] == ord("\n")
    assert max(len(r) for r in reads) == SC.LMAX
    keep, hits, total = oracle.filter_batch(oidx, b, o, threads=4)
    assert len(reads[10]) == SC.L + 1 and total[10] == 1      # one window left
    for i in (11, 70):
        assert len(reads[i]) == SC.L and total[i] == 0        # planned with a tile, dropped to zero windows
    assert len(reads[12]) == SC.K and total[12] == 0
    assert b"\n" in reads[13][1:-1] and total[13] > 0
    for i in (14, 15):
        assert len(reads[i]) == SC.LMAX and reads[i].endswith(b"\n") and total[i] > 0
    assert keep.any() and not keep.all()
    # the newline matters: without it the window count differs
    _, _, t2 = oracle.filter_batch(oidx, *oracle.concat_reads([reads[10][:-1] + b"A"]), threads=1)
    assert t2[0] >= 1


def test_shared_pack_helpers_on_the_host(tmp_path):
    """tests/cpp/pack_helpers_test.cpp: dcn_pack4 / dcn_invalid4 compiled for the host, all 256 byte values in all four byte lanes"""
    exe = tmp_path / "pack_helpers_test"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-I", os.path.join(ROOT, "deacon-server_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "pack_helpers_test.cpp"), "-o", str(exe)])
    subprocess.check_call([str(exe)])

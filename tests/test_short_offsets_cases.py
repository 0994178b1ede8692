"""CPU: the batches of tests/test_gpu_short_offsets.py hold every case they are there for, by the oracle alone; and the window
count and chunk span of a lane of the short path (csrc/dcn_short_lane.h, shared by plan.hip and scan.hip) against a plain
model."""
import os
import subprocess

import numpy as np
import pytest

import _short_fused_cases as SC
import _short_offsets_cases as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LCAP_FLUSH = 25  # a lane past this many list entries makes its wave flush in mid-scan (DCN_LCAP - w, scan.hip)


@pytest.fixture(scope="module")
def world(oracle):
    g = SC.genome()
    return g, oracle.Index.build([g], k=SC.K, w=SC.W)


def run(oracle, oidx, reads, **kw):
    b, o = oracle.concat_reads(reads)
    return oracle.filter_batch(oidx, b, o, threads=4, **kw)


def test_edge_batches_hold_their_cases(oracle, world):
    g, oidx = world
    seen = set()
    for n in OC.EDGE_SIZES:
        reads = OC.edge_batch(g, n)
        assert len(reads) == n
        keep, hits, total = run(oracle, oidx, reads)
        pos = OC.edge_positions(n)
        assert 0 in pos and n - 1 in pos and (63 in pos) and (n == 64 or 64 in pos)
        for p in pos:
            assert total[p] == 0, (n, p)
            kind = {0: "empty", 30: "below_k", OC.L - 1: "below_l", OC.L: "newline"}[len(reads[p])]
            assert (kind == "newline") == reads[p].endswith(b"\n")
            seen.add((kind, p % 64))
        others = np.setdiff1d(np.arange(n), pos)
        assert (total[others] > 0).all() and keep[others].any() and not keep[others].all()
    for kind in OC.NO_WINDOW_KINDS:  # every kind at a wave's first and at a wave's last lane
        assert (kind, 0) in seen and (kind, 63) in seen, kind
    assert len(OC.no_window_read(g, "newline", 0)) == OC.L  # l - 1 bases and the newline: a window by its length alone


def test_idle_wave_and_empty_batch(oracle, world):
    g, oidx = world
    reads = OC.idle_wave_batch(g)
    keep, hits, total = run(oracle, oidx, reads)
    lens = [len(r) for r in reads[64:128]]
    assert len(reads) == 192 and lens[0] == 0 and lens[-1] == OC.L - 1 and sorted(lens) == lens
    assert (total[64:128] == 0).all() and (total[:64] > 0).all() and (total[128:] > 0).all()
    reads = OC.empty_batch()
    assert len(reads) == 70 and sum(len(r) for r in reads) == 0
    keep, hits, total = run(oracle, oidx, reads)
    assert (total == 0).all()


def test_counters_batch_holds_its_cases(oracle, world):
    g, oidx = world
    reads = OC.counters_batch(g)
    lens = np.array([len(r) for r in reads])
    nl = np.array([r.endswith(b"\n") for r in reads])
    assert 900 <= len(reads) <= 1100 and lens.max() <= OC.LMAX
    for abs_t, rel_t, deplete in SC.THRESHOLDS:
        keep, hits, total = run(oracle, oidx, reads, abs_threshold=abs_t, rel_threshold=rel_t, deplete=deplete)
        nowin = total == 0
        for sel, what in ((~nowin & ~nl, "plain"), (~nowin & nl, "newline-terminated")):
            assert keep[sel].any() and not keep[sel].all(), (what, abs_t, rel_t, deplete)
        for ln in (0, 30, OC.L - 1):
            assert nowin[lens == ln].all() and (lens == ln).any()
        assert (nowin & nl & (lens == OC.L)).any()
        # reads without a window are kept by one threshold and dropped by another: both sides of the counters see them
        assert keep[nowin].all() or not keep[nowin].any()
    kept_nowin = {bool(run(oracle, oidx, reads, abs_threshold=a, rel_threshold=r, deplete=d)[0][0]) for a, r, d in SC.THRESHOLDS}
    assert kept_nowin == {True, False} and lens[0] == 0
    keep, hits, total = run(oracle, oidx, reads)
    assert total[500] > LCAP_FLUSH and hits[500] == 0      # the flush, by a read without hits
    assert 448 <= 501 < 512 and hits[501] == total[501] > 0  # an exported unit in the same wave


def test_overflow_batch_holds_its_cases(oracle, world):
    g, _ = world
    oidx = oracle.Index.build([OC.overflow_genome(g)], k=SC.K, w=SC.W)
    reads = OC.overflow_batch(g)
    assert 190 <= len(reads) <= 210
    keep, hits, total = run(oracle, oidx, reads)
    for i in (OC.OVERFLOW_WAVE_LANE0, OC.OVERFLOW_WAVE_LANE63):
        assert reads[i] == OC.POLY_A and total[i] == 108 and hits[i] == 1
        assert total[i] > (OC.LMAX >> 2) + 1  # one hit per window against a run of one slot per four bases
    assert OC.OVERFLOW_WAVE_LANE0 % 64 == 0 and OC.OVERFLOW_WAVE_LANE63 % 64 == 63
    assert OC.OVERFLOW_WAVE_LANE0 // 64 != OC.OVERFLOW_WAVE_LANE63 // 64
    i = OC.IN_WAVE_POLY_A
    assert reads[i] == b"A" * 60 and total[i] == 16 and hits[i] == 1 and total[i] <= LCAP_FLUSH
    wave = slice(64 * (i // 64), 64 * (i // 64) + 64)
    assert total[wave].max() <= LCAP_FLUSH  # no flush in its wave: resolved there
    assert keep.any() and not keep.all()


def test_stale_plan_holds_its_cases(oracle, world):
    g, oidx = world
    plan = OC.stale_plan(g)
    assert [len(r) for r, _ in plan] == [900, 100, 40, 65] and [s for _, s in plan] == [True, True, False, True]
    for reads, short in plan:
        assert (max(len(r) for r in reads) <= OC.LMAX) is short
        keep, hits, total = run(oracle, oidx, reads)
        assert keep.any() and not keep.all()
    _, hits, total = run(oracle, oidx, plan[0][0])
    assert total[500] > LCAP_FLUSH and hits[501] > 0  # the first batch leaves a tile and a pending unit behind


def test_short_lane_header_on_the_host(tmp_path):
    """tests/cpp/short_lane_test.cpp: dcn_short_lane / dcn_window_count compiled for the host, lengths 0..153 with and without a
    trailing newline at all 16 alignments"""
    exe = tmp_path / "short_lane_test"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-I", os.path.join(ROOT, "deacon-server_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "short_lane_test.cpp"), "-o", str(exe)])
    subprocess.check_call([str(exe)])

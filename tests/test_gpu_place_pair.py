"""Paired placements on the GPU against the model of tests/_place_pair_worker.py, all 80 bytes of every row field for
field.  Integers only, no tolerance.  The models, the pairs and the maps are built once per case and left unchanged."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _place_pair_worker as PPW
import _place_worker as PW
from _place_pair_worker import F, assert_pairs, place_pair_all

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# k = 31 at w = 15 and w = 1, k = 32 (a k-mer can be its own reverse complement), k = 33 (128-bit k-mers)
CASES = [(31, 15), (31, 1), (32, 16), (33, 15)]
NS = (1, 2, 4, 8)


@pytest.fixture(scope="module")
def records():
    return PW.make_records(PW.make_genomes())


@pytest.fixture(scope="module")
def models(oracle, records):
    """(model, pairs, reads) per case: the CPU side alone"""
    out = {}
    for k, w in CASES:
        model = PW.AnchorModel(oracle, k, w, oracle.Index.build(records, k=k, w=w).keys()).add(records)
        pairs = PPW.pair_reads(model, records)
        out[(k, w)] = (model, pairs, [m for _, a, b in pairs for m in (a, b)])
    return out


@pytest.fixture(scope="module")
def built(oracle, dcn, records, models):
    """(map, batch, a Placer) per case"""
    out = {}
    for k, w in CASES:
        model, _, reads = models[(k, w)]
        _, amap = PW.build_map(oracle, dcn, records, k, w)
        placer = dcn.Placer(amap, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
        out[(k, w)] = (amap, oracle.concat_reads(reads), placer)
    yield out
    for amap, _, placer in out.values():
        placer.close()
        amap.close()


@pytest.mark.parametrize("k,w", CASES)
def test_pair_placements_equal_the_model(dcn, models, built, k, w):
    """first, on the model alone, the batch holds every kind of pair; then every max_placements on one context, the
    histogram with it, and the invariant of rule 5: a pair without a concordant combination gives each mate the rank-0
    row of place_split_batch, or none"""
    model, pairs, reads = models[(k, w)]
    _, seen = PPW.kinds_hold(model, pairs)
    assert all(seen.get(kind, 0) >= 1 for kind in PPW.ALL_KINDS), [kind for kind in PPW.ALL_KINDS if not seen.get(kind)]
    assert seen["subst"] == sum(1 for p in pairs if p[0] == "subst")
    amap, (b, o), placer = built[(k, w)]
    for n in NS:
        rows, hist = placer.place_pair_batch(b, o, max_placements=n)
        assert rows.dtype == dcn.filter.PAIR_PLACEMENT_DTYPE and hist.dtype == np.uint64 and len(hist) == 256
        want = place_pair_all(model, reads, max_placements=n)
        assert_pairs((rows, hist), want, (k, w, n))
        proper = (rows["flags"] & PPW.PROPER).astype(bool)
        assert int(hist.sum()) == int(proper.sum()) // 2 > 60
        assert (rows["pair_votes"][proper][0::2] == rows["votes"][proper][0::2] + rows["votes"][proper][1::2]).all()
        assert (rows["pair_votes"][proper][0::2] == rows["pair_votes"][proper][1::2]).all()
        assert (rows["tlen"][proper][0::2] == -rows["tlen"][proper][1::2]).all() and (rows["tlen"][~proper] == 0).all()
        assert int((rows["flags"] & PPW.RESCUED).astype(bool).sum()) >= 8 and (rows["mapq"] <= 60).all()
        # rule 5: without a concordant combination a mate's row is the split call's rank-0 row, or it has none
        po, split_rows, counts = placer.place_split_batch(b, o, max_placements=n)
        per = np.diff(po.astype(np.int64))
        assert (rows["n_anchors"] == counts[:, 0]).all() and (rows["n_positions"] == counts[:, 1]).all()
        lone = ~proper
        assert ((rows["record"][lone] != PPW.UNPLACED) == (per[lone] > 0)).all()
        placed = lone & (rows["record"] != PPW.UNPLACED)
        first = split_rows[po[:-1][placed].astype(np.int64)]
        for f in dcn.filter.SPLIT_PLACEMENT_DTYPE.names:
            assert (first[f] == rows[f][placed]).all(), (k, w, n, f)
        assert (rows["pair_votes"][placed] == rows["votes"][placed]).all() and int(placed.sum()) > 40
        assert (rows["n_placed"][proper] == per[proper]).all()
        if n >= 2:
            assert int((rows["rank"] == 1).sum()) >= 8
    again = placer.place_pair_batch(b, o, max_placements=8)
    assert again[0].tobytes() == rows.tobytes() and again[1].tolist() == hist.tolist()


@pytest.mark.parametrize("k,w", [(31, 15), (31, 1)])
def test_prefix_band_min_votes_and_max_insert(oracle, dcn, models, built, k, w):
    model, _, reads = models[(k, w)]
    amap = built[(k, w)][0]
    PPW.check_pairs(dcn, oracle, model, amap, reads, (k, w), prefix_length=60)
    for W, votes, n, I, hbin in ((1, 1, 8, 1000, 8), (31, 3, 4, 400, 1), (64, 5, 2, 2000, 16), (1 << 20, 2, 4, 300, 3),
                                 (0xFFFFFFFF, 2, 2, 0xFFFFFFFF, 0xFFFFFFFF)):
        PPW.check_pairs(dcn, oracle, model, amap, reads, (k, w), max_placements=n, band_bases=W, min_votes=votes, max_insert=I,
                        hist_bin_bases=hbin)


def test_histogram_is_optional_and_overwritten(dcn, models, built):
    model, _, reads = models[(31, 15)]
    amap, (b, o), placer = built[(31, 15)]
    want = place_pair_all(model, reads)
    rows, hist = placer.place_pair_batch(b, o, want_hist=False)
    assert hist is None
    assert_pairs((rows, None), want)
    with_hist = placer.place_pair_batch(b, o)
    assert with_hist[0].tobytes() == rows.tobytes()
    assert_pairs(with_hist, want)  # (not the sum of two calls: every call overwrites)
    # through the C ABI: a histogram full of ones is overwritten, rows of 0xAB are fully written
    N = dcn._native
    n = len(reads)
    raw = np.frombuffer(bytearray(b"\xAB" * (80 * n)), dcn.filter.PAIR_PLACEMENT_DTYPE)
    h = np.ones(256, np.uint64)
    prm = N.PlacePairParams(256, 2, 0, 4, 1000, 8, (C.c_uint32 * 3)(0, 0, 0))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert N.lib().dcn_place_pair_batch(placer._h, amap._h, ptr(b), ptr(o), n, C.byref(prm), ptr(raw), ptr(h)) == N.DCN_OK
    assert raw.tobytes() == rows.tobytes() and h.tolist() == list(want[1])
    assert N.lib().dcn_place_pair_batch(placer._h, amap._h, ptr(b), ptr(o), n - 1, C.byref(prm), ptr(raw), ptr(h)) == N.DCN_ERR_ARG
    assert b"even" in N.lib().dcn_last_error()
    assert N.lib().dcn_place_pair_batch(placer._h, amap._h, ptr(b), ptr(o), n, C.byref(prm), None, ptr(h)) == N.DCN_ERR_ARG
    assert b"rows is NULL" in N.lib().dcn_last_error()
    plain = dcn.Index.from_keys(np.arange(1, 100, dtype=np.uint64), 31, 15)
    try:
        assert N.lib().dcn_place_pair_batch(placer._h, plain._h, ptr(b), ptr(o), n, C.byref(prm), ptr(raw), ptr(h)) == N.DCN_ERR_ARG
        assert b"not an anchor map" in N.lib().dcn_last_error()
    finally:
        plain.close()


def test_no_reads_and_lists(dcn, models, built):
    model, pairs, reads = models[(31, 15)]
    amap, _, placer = built[(31, 15)]
    rows, hist = placer.place_pair_batch(np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    assert len(rows) == 0 and hist.tolist() == [0] * 256
    N = dcn._native
    h = np.ones(256, np.uint64)
    prm = N.PlacePairParams(256, 2, 0, 4, 1000, 8, (C.c_uint32 * 3)(0, 0, 0))
    assert N.lib().dcn_place_pair_batch(placer._h, amap._h, None, None, 0, C.byref(prm), None, h.ctypes.data_as(C.c_void_p)) == N.DCN_OK
    assert not h.any()
    assert N.lib().dcn_place_pair_batch(placer._h, amap._h, None, None, 0, C.byref(prm), None, None) == N.DCN_OK
    got = placer.place_pairs([p[1] for p in pairs[:20]], [p[2] for p in pairs[:20]], max_placements=2)
    assert_pairs(got, place_pair_all(model, reads[:40], max_placements=2))
    with pytest.raises(ValueError):
        placer.place_pairs([b"ACGT"], [])


def test_one_context_serves_place_split_pair_locate_in_turn(oracle, dcn, models, built):
    """place_batch, place_split_batch, place_pair_batch, dcn_locate_batch and place_pair_batch again on ONE context:
    each call gives its own answer, the six counters stay as they were, and profiling covers the new call"""
    N = dcn._native
    model, _, reads = models[(31, 15)]
    amap, (b, o), placer = built[(31, 15)]
    n = len(reads)
    want = place_pair_all(model, reads)
    stats = placer.stats()
    one = placer.place_batch(b, o)
    split = placer.place_split_batch(b, o)
    assert_pairs(placer.place_pair_batch(b, o), want)
    loc = dcn.Locator(amap, max_gap=0, min_hits=1, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    try:
        so_want, segs_want = loc.locate_batch(b, o)
    finally:
        loc.close()
    prm = N.LocateParams(max_gap=0, min_hits=1, member_mask=0xFFFFFFFF, reserved=0, prefix_length=0)
    so = np.zeros(n + 1, np.uint64)
    segs = np.zeros(max(len(segs_want), 1), dcn.filter.SEGMENT_DTYPE)
    N.check(N.lib().dcn_locate_batch(placer._h, amap._h, b.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p), n,
                                     C.byref(prm), so.ctypes.data_as(C.c_void_p), segs.ctypes.data_as(C.c_void_p), len(segs)))
    assert so.tolist() == so_want.tolist() and segs[:len(segs_want)].tobytes() == segs_want.tobytes()
    placer.set_profiling(True)
    assert_pairs(placer.place_pair_batch(b, o), want)
    ms, batches = placer.profile()
    assert batches == 1 and ms["distinct"] > 0 and ms["finish"] > 0
    placer.set_profiling(False)
    assert placer.place_batch(b, o).tobytes() == one.tobytes()
    again = placer.place_split_batch(b, o)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(again, split))
    assert placer.stats() == stats


WORKER = os.path.join(ROOT, "tests", "_place_pair_worker.py")
ENV_CASES = [("seams", {"DCN_TILE_WINDOWS": "16"}),
             ("switch", {"DCN_PLACE_LANE_BASES": "100"}),
             ("partitions", {"DCN_PLACE_LDS_CELLS": "16", "DCN_PLACE_LANE_BASES": "200"})]


@pytest.mark.parametrize("case,env", ENV_CASES, ids=[c for c, _ in ENV_CASES])
def test_environment_hooks_in_a_process_of_their_own(case, env):
    """tiles of 16 windows; one mate on the workgroup path and one on the lane path, in both orders; the partitioned LDS
    count for one mate (the hooks are read at call time, so each case runs in a fresh process)"""
    p = subprocess.run([sys.executable, WORKER, case], env={**os.environ, **env}, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "ok" in p.stdout

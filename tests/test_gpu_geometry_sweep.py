"""Every consumer of the minimizer dump at every kernel geometry: for each (k, w) of tests/_geometry_cases.py, on ONE
context, depth track, host filter, classify with depth and coverage, locate on a plain index and on the set, anchor add,
place and place split, and the counting index builder beside them -- against the models of the per-feature tests over
the CPU oracle.  Three of the geometries run a second time with tiles of 16 windows, two table slots per key and the
workgroup form of the vote with its smallest LDS set.  Integers only, compared exactly; nothing is compared with another
output of the code under test.  test_cases_are_not_vacuous needs no GPU: it holds the inputs to what the sweep is for."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import _depth_worker as DW
import _geometry_cases as G
from _depth_track_worker import assert_track
from _index_builder_worker import assert_counts, selected
from _place_split_worker import assert_split
from _place_worker import assert_map, assert_placements
from test_gpu_locate import assert_same

CASES = [(kw, False) for kw in G.GEOMETRIES] + [(kw, True) for kw in G.TIGHT]
CASE_IDS = [G.kw_id(kw) + ("-tight" if tight else "") for kw, tight in CASES]


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("kw", G.GEOMETRIES, ids=G.kw_id)
def test_cases_are_not_vacuous(oracle, kw):
    G.assert_not_vacuous(oracle, *kw)


@pytest.mark.gpu
@pytest.mark.parametrize("kw,tight", CASES, ids=CASE_IDS)
def test_every_consumer_at_this_geometry(oracle, dcn, kw, tight, monkeypatch):
    k, w = kw
    if tight:
        for name, value in G.TIGHT_ENV.items():
            monkeypatch.setenv(name, value)
    wd = G.world(oracle, k, w)
    what = (k, w, "tight" if tight else "default")
    N = dcn._native
    lib = N.lib()
    reads, b, o, mkeys, gap = wd["reads"], wd["b"], wd["o"], wd["mkeys"], wd["gap"]
    n = len(reads)
    gl = [dcn.Index.from_keys(x.keys(), k, w) for x in wd["ol"]]
    s = dcn.IndexSet(gl)
    s.enable_depth()
    s.enable_coverage()
    map_index = dcn.Index.from_keys(wd["union_keys"], k, w)
    amap = dcn.AnchorMap(map_index)
    map_index.close()
    clf = dcn.Classifier(s, max_batch_bases=1 << 17, max_batch_reads=1 << 9)
    ctx = clf._h
    depth = Counter()

    def track(bin_bases, want):
        prm = N.TrackParams(bin_bases, 7, 0, 0, 0)
        bo = np.zeros(n + 1, np.uint64)
        bins = np.zeros(int(want[0][-1]), dcn.filter.TRACK_BIN_DTYPE)
        N.check(lib.dcn_depth_track_batch(ctx, s._h, ptr(b), ptr(o), n, C.byref(prm), ptr(bo), ptr(bins), len(bins)))
        assert_track((bo, bins), want, what + ("bin_bases", bin_bases))

    def host_filter():
        prm = N.Params(2, 0.01, 0, 0, 0)
        keep, hits, total = np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        N.check(lib.dcn_filter_batch(ctx, ptr(b), ptr(o), None, n, C.byref(prm), ptr(keep), ptr(hits), ptr(total)))
        wk, wh, wt = wd["filter"]
        assert total.tolist() == wt and hits.tolist() == wh and keep.astype(bool).tolist() == wk, what + ("filter",)

    def classify():
        match, hits, total = clf.classify_batch(b, o)
        for j, (keep, h, t) in enumerate(wd["classify"]):
            assert total.tolist() == t.tolist() and hits[:, j].tolist() == h.tolist(), what + ("classify", j)
            assert ((match >> j) & 1).astype(bool).tolist() == keep.tolist(), what + ("match", j)
        depth.update(wd["occurrences"])
        DW.assert_depths(s, depth, mkeys, bins=(256,))
        for j in (None, 0, 1, 2):
            assert set(s.observed_keys(j).tolist()) == set(DW.expected(depth, mkeys, j)), what + ("observed", j)

    def locate(index, want, min_hits=1, mask=0xFFFFFFFF):
        prm = N.LocateParams(gap, min_hits, mask, 0, 0)
        so = np.zeros(n + 1, np.uint64)
        segs = np.zeros(sum(len(x) for x in want) + 1, dcn.filter.SEGMENT_DTYPE)
        N.check(lib.dcn_locate_batch(ctx, index._h, ptr(b), ptr(o), n, C.byref(prm), ptr(so), ptr(segs), len(segs)))
        assert_same([[tuple(int(x) for x in q) for q in segs[int(so[r]):int(so[r + 1])]] for r in range(n)], want)

    def add(i):
        rb, ro = oracle.concat_reads(wd["adds"][i])
        first = C.c_uint32()
        N.check(lib.dcn_anchor_map_add(amap._h, ctx, ptr(rb), ptr(ro), len(wd["adds"][i]), C.byref(first)))
        assert first.value == sum(len(x) for x in wd["adds"][:i])
        assert_map(amap, wd["anchors"][i], what + ("add", i))

    def place(i):
        prm = N.PlaceParams(256, 2, 0, (C.c_uint32 * 2)(0, 0))
        out = np.zeros(n, dcn.filter.PLACEMENT_DTYPE)
        N.check(lib.dcn_place_batch(ctx, amap._h, ptr(b), ptr(o), n, C.byref(prm), ptr(out)))
        assert_placements(out, wd["place"][i], what + ("place", i))

    def place_split():
        prm = N.PlaceSplitParams(256, 2, 0, 4, (C.c_uint32 * 3)(0, 0, 0))
        po = np.zeros(n + 1, np.uint64)
        rows = np.zeros(n * 4, dcn.filter.SPLIT_PLACEMENT_DTYPE)
        counts = np.zeros((n, 2), np.uint32)
        N.check(lib.dcn_place_split_batch(ctx, amap._h, ptr(b), ptr(o), n, C.byref(prm), ptr(po), ptr(rows), len(rows), ptr(counts)))
        assert_split((po, rows[:int(po[n])], counts), wd["split"], what + ("split",))

    try:
        # the order of tests/test_gpu_dump_consumers.py's track_first, then the second add and what depends on it
        track(100, wd["track_before"])
        host_filter()
        classify()
        locate(gl[0], wd["locate_plain"])
        add(0)
        locate(s, wd["locate_set"])
        place(0)
        add(1)
        locate(s, wd["locate_masked"], min_hits=2, mask=0b101)
        track(0, wd["track_after"])
        track(100, wd["track_after_100"])
        place(1)
        place_split()
        host_filter()
    finally:
        clf.close()
        amap.close()
        s.close()
        for g in gl:
            g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kw", G.GEOMETRIES, ids=G.kw_id)
def test_index_builder_at_this_geometry(oracle, dcn, kw, monkeypatch):
    """the counting build with and without the entropy floor, whole and in pieces of 4,096 bases: at k > 32 the floor reads
    k-mers longer than 32 bases, at l - 1 = 148 the seam between two pieces crosses five bitmap words"""
    k, w = kw
    bw = G.builder_world(oracle, k, w)
    for chunk in (None, "4096"):
        if chunk:
            monkeypatch.setenv("DCN_BUILD_CHUNK_BASES", chunk)
            assert bw["shared"] >= 1 or w == 1
        else:
            monkeypatch.delenv("DCN_BUILD_CHUNK_BASES", raising=False)
        for thr in (0.0, 0.5):
            model = bw["models"][thr]
            b = dcn.IndexBuilder(k, w, entropy_threshold=thr)
            try:
                b.add(bw["seqs"])
                assert_counts(b, model, bins=(3, 256))
                assert b.info()["n_bases"] == sum(len(x) for x in bw["seqs"]), (k, w, chunk, thr)
                idx = b.finish(2, 0)
                assert sorted(idx.keys().tolist()) == selected(model, 2, 0), (k, w, chunk, thr, "finish")
                idx.close()
            except AssertionError as e:
                raise AssertionError((k, w, "chunk", chunk, "thr", thr) + tuple(e.args)) from e
            finally:
                b.close()

"""Every consumer of the minimizer dump on ONE context, in two orders, twice over: host filter, classify against a set
with depth and coverage, locate on a plain index and on the set, depth track, anchor add and place.  They share the front
end, the tail of the call, the position bitmap and the word per base (ctx.hip), which whichever call comes first
allocates; the second pass runs a smaller batch whose hits lie elsewhere, so a bitmap or a word one call left behind would
show in the next.  Every expected value comes from the models of the per-feature tests over the CPU oracle, never from
the code under test.  Integers only, no tolerance."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import _depth_worker as DW
from _depth_track_worker import Model as TrackModel
from _depth_track_worker import assert_track
from _place_worker import AnchorModel, assert_map, assert_placements
from test_gpu_locate import assert_same, model_batch, plain_label, set_label

pytestmark = pytest.mark.gpu

K, W = 31, 15
GAP = 2 * W - 1
ORDERS = {  # the first call of a context allocates the bitmap and the word per base: track's, or place's
    "track_first": ("track", "filter", "classify", "locate_plain", "add", "locate_set", "place"),
    "place_first": ("place", "add", "locate_set", "classify", "track", "filter", "locate_plain"),
}


@pytest.fixture(scope="module")
def world(oracle, dcn):
    """genomes, the three members (oracle indexes, key sets, device indexes), their union, and the two batches with the
    call-independent expected values of each"""
    genomes = DW.make_genomes()
    ol = [oracle.Index.build(seqs, k=K, w=W) for seqs in DW.member_seqs(genomes)]
    mkeys = [set(o.keys().tolist()) for o in ol]
    union_keys = np.unique(np.concatenate([o.keys() for o in ol]))
    union = oracle.Index(union_keys, K, W)
    batches = []
    for seed, n in ((811, 200), (812, 120)):  # the second batch is smaller, of other places of the genomes
        rng = np.random.default_rng(seed)
        reads = DW.sample(rng, genomes, n, K, 400, p_n=0.0)
        # below k + w - 1, one window, a read of several tiles at 256 windows a tile, a read with N
        reads[3], reads[4] = genomes[0][900:900 + K + W - 3], genomes[1][77:77 + K + W - 1]
        at = int(rng.integers(0, 15_000))
        reads[7] = genomes[seed % 3][at:at + 3000]
        reads[11] = genomes[2][at:at + 120] + b"NN" + genomes[2][at + 122:at + 300]
        b, o = oracle.concat_reads(reads)
        keep, hits, total = oracle.filter_batch(union, b, o, None, abs_threshold=2, rel_threshold=0.01, deplete=False, threads=4)
        batches.append({
            "reads": reads, "b": b, "o": o,
            "filter": (keep.tolist(), hits.tolist(), total.tolist()),
            "classify": [oracle.filter_batch(oj, b, o, None, abs_threshold=2, rel_threshold=0.01, deplete=False, threads=4)
                         for oj in ol],
            "locate_plain": model_batch(oracle, reads, K, W, plain_label(ol[0]), 0, GAP, 1),
            "locate_set": model_batch(oracle, reads, K, W, set_label(ol), 0, GAP, 1),
            "occurrences": DW.occurrences(oracle, reads, K, W),
        })
    assert len(batches[0]["b"]) > len(batches[1]["b"])
    for bt in batches:
        assert sum(1 for s in bt["locate_set"] if s) > 50 and any(len(r) > 256 * 8 for r in bt["reads"])
    return {"genomes": genomes, "ol": ol, "mkeys": mkeys, "union_keys": union_keys, "batches": batches,
            "gl": [dcn.Index.from_keys(o.keys(), K, W) for o in ol]}


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("pack_ahead", [False, True])
@pytest.mark.parametrize("order", sorted(ORDERS))
def test_every_consumer_on_one_context(oracle, dcn, world, order, pack_ahead, monkeypatch):
    N = dcn._native
    lib = N.lib()
    ol, mkeys, genomes = world["ol"], world["mkeys"], world["genomes"]
    if pack_ahead:  # a device-pointer filter batch then packs on a side stream, after the events every call's tail records
        torch = pytest.importorskip("torch")
        monkeypatch.setenv("DCN_PACK_AHEAD", "1")
    s = dcn.IndexSet(world["gl"])
    s.enable_depth()
    s.enable_coverage()
    map_index = dcn.Index.from_keys(world["union_keys"], K, W)
    amap = dcn.AnchorMap(map_index)
    map_index.close()
    anchors = AnchorModel(oracle, K, W, world["union_keys"])
    depth = Counter()  # what the classify calls so far have counted
    clf = dcn.Classifier(s, max_batch_bases=1 << 17, max_batch_reads=1 << 9)
    ctx = clf._h
    fprm = N.Params(2, 0.01, 0, 0, 0)

    def device_filter(batches):
        """device-pointer filter batches queued back to back, then one synchronize"""
        dev = torch.device("cuda:0")
        outs = []
        for bt in batches:
            n = len(bt["reads"])
            d_b, d_o = torch.from_numpy(bt["b"]).to(dev), torch.from_numpy(bt["o"].view(np.int64)).to(dev)
            k = torch.zeros(n, dtype=torch.uint8, device=dev)
            h, t = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()  # (the arrays are made on torch's stream)
            N.check(lib.dcn_filter_batch_device(ctx, d_b.data_ptr(), d_o.data_ptr(), None, n, len(bt["b"]), n, C.byref(fprm),
                                                k.data_ptr(), h.data_ptr(), t.data_ptr()))
            outs.append((d_b, d_o, k, h, t))
        N.check(lib.dcn_ctx_synchronize(ctx))
        for bt, (_, _, k, h, t) in zip(batches, outs):
            got = (k.cpu().numpy().astype(bool).tolist(), h.cpu().numpy().tolist(), t.cpu().numpy().tolist())
            assert got == bt["filter"]

    def run_filter(bt, _):
        n = len(bt["reads"])
        keep, hits, total = np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        N.check(lib.dcn_filter_batch(ctx, ptr(bt["b"]), ptr(bt["o"]), None, n, C.byref(fprm), ptr(keep), ptr(hits), ptr(total)))
        assert (keep.astype(bool).tolist(), hits.tolist(), total.tolist()) == bt["filter"]

    def run_classify(bt, _):
        match, hits, total = clf.classify_batch(bt["b"], bt["o"])
        for j, (keep, h, t) in enumerate(bt["classify"]):
            assert hits[:, j].tolist() == h.tolist() and total.tolist() == t.tolist()
            assert ((match >> j) & 1).astype(bool).tolist() == keep.tolist()
        depth.update(bt["occurrences"])
        DW.assert_depths(s, depth, mkeys, bins=(256,))
        for j in (None, 0, 1, 2):
            assert set(s.observed_keys(j).tolist()) == set(DW.expected(depth, mkeys, j))

    def run_locate(index, want, bt):
        n = len(bt["reads"])
        prm = N.LocateParams(GAP, 1, 0xFFFFFFFF, 0, 0)
        so = np.zeros(n + 1, np.uint64)
        segs = np.zeros(sum(len(x) for x in want) + 1, dcn.filter.SEGMENT_DTYPE)
        N.check(lib.dcn_locate_batch(ctx, index._h, ptr(bt["b"]), ptr(bt["o"]), n, C.byref(prm), ptr(so), ptr(segs), len(segs)))
        assert_same([[tuple(int(x) for x in q) for q in segs[int(so[r]):int(so[r + 1])]] for r in range(n)], want)

    def run_track(bt, i):
        n = len(bt["reads"])
        bin_bases = (100, 0)[i]  # bins one lane walks; then one bin a read, the 3000-base read's cut into pieces
        want = TrackModel(oracle, bt["reads"], K, W, mkeys, depth).bins(bin_bases, 7)
        prm = N.TrackParams(bin_bases, 7, 0, 0, 0)
        bo = np.zeros(n + 1, np.uint64)
        bins = np.zeros(int(want[0][-1]), dcn.filter.TRACK_BIN_DTYPE)
        N.check(lib.dcn_depth_track_batch(ctx, s._h, ptr(bt["b"]), ptr(bt["o"]), n, C.byref(prm), ptr(bo), ptr(bins), len(bins)))
        assert_track((bo, bins), want, (order, i))

    def run_add(_, i):
        records = [genomes[:2], genomes[2:]][i]
        b, o = oracle.concat_reads(records)
        first = C.c_uint32()
        N.check(lib.dcn_anchor_map_add(amap._h, ctx, ptr(b), ptr(o), len(records), C.byref(first)))
        assert first.value == len(anchors.records)
        anchors.add(records)
        assert_map(amap, anchors, (order, i))

    def run_place(bt, i):
        n = len(bt["reads"])
        prm = N.PlaceParams(256, 2, 0, (C.c_uint32 * 2)(0, 0))
        out = np.zeros(n, dcn.filter.PLACEMENT_DTYPE)
        N.check(lib.dcn_place_batch(ctx, amap._h, ptr(bt["b"]), ptr(bt["o"]), n, C.byref(prm), ptr(out)))
        assert_placements(out, anchors.place_all(bt["reads"]), (order, i))

    calls = {"filter": run_filter, "classify": run_classify, "track": run_track, "add": run_add, "place": run_place,
             "locate_plain": lambda bt, _: run_locate(world["gl"][0], bt["locate_plain"], bt),
             "locate_set": lambda bt, _: run_locate(s, bt["locate_set"], bt)}
    try:
        if pack_ahead:  # (the side stream and its events are made by the first device-pointer batch)
            device_filter(world["batches"][:1])
        for i, bt in enumerate(world["batches"]):
            for name in ORDERS[order]:
                calls[name](bt, i)
        assert len(anchors.anchors()) > 1000 and sum(depth.values()) > 1000
        if pack_ahead:
            device_filter(world["batches"])
    finally:
        clf.close()
        amap.close()
        s.close()


STATS = {"total_seqs", "filtered_seqs", "total_bp", "output_bp", "filtered_bp", "output_seq_counter"}
STAGES = {"pack", "plan", "scan", "distinct", "finish"}


def test_context_owners(oracle, dcn):
    """The five classes that are a context and the AnchorMap that holds one: stats() and profile() keep their keys, close()
    twice is harmless and leaves `_h` None; the map's context is re-created once for a batch longer than it, and kept for a
    shorter one after"""
    rng = np.random.default_rng(813)
    alpha = np.frombuffer(b"ACGT", np.uint8)
    genome = alpha[rng.integers(0, 4, 1500)].tobytes()
    keys = oracle.Index.build([genome], k=K, w=W).keys()
    assert 50 < len(keys) < 400
    index = dcn.Index.from_keys(keys, K, W)
    s = dcn.IndexSet([index])
    s.enable_depth()
    amap = dcn.AnchorMap(index)
    b, o = oracle.concat_reads([genome[100:300], genome[700:900]])
    small = dict(max_batch_bases=1 << 12, max_batch_reads=1 << 4)
    owners = [(dcn.FilterProcessor(index, **small), lambda x: x.filter_batch(b, o)),
              (dcn.Classifier(s, **small), lambda x: x.classify_batch(b, o)),
              (dcn.Locator(index, **small), lambda x: x.locate_batch(b, o)),
              (dcn.DepthTracker(s, **small), lambda x: x.track_batch(b, o)),
              (dcn.Placer(amap, **small), lambda x: x.place_batch(b, o))]
    try:
        # the map: no context before the first add; the floor of 1 Mi bases / 1 Ki reads; grow only
        assert amap._ctx is None
        assert amap.add(b, o) == 0
        first = amap._ctx
        assert (first.max_batch_bases, first.max_batch_reads) == (1 << 20, 1 << 10) and first._h
        long_record = alpha[rng.integers(0, 4, 2_000_000)].tobytes()
        assert amap.add_records([long_record]) == 2
        second = amap._ctx
        assert second is not first and first._h is None and second._h
        assert (second.max_batch_bases, second.max_batch_reads) == (2_000_000, 1 << 10)
        handle = second._h.value
        assert amap.add(b, o) == 3
        assert amap._ctx is second and second._h.value == handle and second.max_batch_bases == 2_000_000
        assert amap.info()["records"] == 5
        for obj, call in owners:
            assert (obj.max_batch_bases, obj.max_batch_reads) == (1 << 12, 1 << 4)
            obj.set_profiling(True)
            call(obj)
            obj.synchronize()
            stage_ms, n_batches = obj.profile()
            assert set(stage_ms) == STAGES and all(isinstance(v, float) for v in stage_ms.values()), type(obj)
            assert isinstance(n_batches, int) and n_batches >= 1, type(obj)
            st = obj.stats()
            assert set(st) == STATS and all(isinstance(v, int) for v in st.values()), type(obj)
            obj.close()
            assert obj._h is None
            obj.close()
            assert obj._h is None
        amap.close()
        assert amap._ctx is None and amap._h is None and second._h is None
        amap.close()
    finally:
        for obj, _ in owners:
            obj.close()
        amap.close()
        s.close()
        index.close()

"""Anchor maps and placement on the GPU against the model of tests/_place_worker.py (the definitions of
include/deacon_hip.h over oracle.minimizer_hashes_and_positions and plain dicts).  Integers only, no tolerance."""
import ctypes as C

import numpy as np
import pytest

import _place_worker as PW
from _place_worker import AnchorModel, assert_map, assert_placements, build_map, parity_reads, place

pytestmark = pytest.mark.gpu

# k = 31 at w = 15 and w = 1, k = 32 (a k-mer can be its own reverse complement), k = 33 (128-bit k-mers)
CASES = [(31, 15), (31, 1), (32, 16), (33, 15)]


@pytest.fixture(scope="module")
def records():
    return PW.make_records(PW.make_genomes())


@pytest.fixture(scope="module")
def built(oracle, dcn, records):
    """(model, map, reads, placements of the model at the defaults) per case, built once and left unchanged"""
    out = {}
    for k, w in CASES:
        model, amap = build_map(oracle, dcn, records, k, w)
        reads = parity_reads(model, records)
        out[(k, w)] = (model, amap, reads, model.place_all(reads))
    yield out
    for _, amap, _, _ in out.values():
        amap.close()


@pytest.mark.parametrize("k,w", CASES)
def test_info_and_anchors_equal_the_model(built, k, w):
    model, amap, _, _ = built[(k, w)]
    assert_map(amap, model, (k, w))
    info = model.info()
    assert info["repeats"] >= 40 and info["anchors"] > 7000 and info["records"] == 6  # the stretch held twice, the shared one


@pytest.mark.parametrize("k,w", CASES)
def test_placements_equal_the_model(oracle, dcn, built, k, w):
    model, amap, reads, want = built[(k, w)]
    got = place(dcn, amap, reads, oracle)
    assert got.dtype == dcn.filter.PLACEMENT_DTYPE
    assert_placements(got, want, (k, w))
    placed = got["record"] != PW.UNPLACED
    assert int(placed.sum()) > 600 and int((~placed).sum()) > 20 and int(got["reverse"].sum()) > 150
    assert int((got["n_anchors"] > got["votes"])[placed].sum()) >= 2  # the chimeras, at least
    # the two-record chimera whose halves tie is the read before the 20 random ones: it goes to the smaller record
    tie = got[len(reads) - 21]
    assert tie["record"] == 0 and tie["n_anchors"] >= 2 * tie["votes"]


@pytest.mark.parametrize("k,w", [(31, 15), (31, 1)])
def test_prefix_band_and_min_votes(oracle, dcn, built, k, w):
    model, amap, reads, _ = built[(k, w)]
    assert_placements(place(dcn, amap, reads, oracle, prefix_length=60), model.place_all(reads, prefix=60), (k, w, "prefix"))
    for W, votes in ((1, 1), (31, 3), (1 << 20, 2), (0xFFFFFFFF, 2)):
        assert_placements(place(dcn, amap, reads, oracle, band_bases=W, min_votes=votes),
                          model.place_all(reads, W=W, min_votes=votes), (k, w, W, votes))


def test_a_second_placer_agrees_and_place_takes_lists(oracle, dcn, built):
    model, amap, reads, want = built[(31, 15)]
    a = dcn.Placer(amap, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    b = dcn.Placer(amap, max_batch_bases=1 << 19, max_batch_reads=1 << 11)
    try:
        ga, gb = a.place(reads), b.place(reads)
        assert ga.tobytes() == gb.tobytes()
        assert_placements(ga, want)
        assert_placements(a.place(reads[:7]), want[:7])  # a context is used again
        assert len(a.place([])) == 0
        a.set_profiling(True)
        a.place(reads)
        ms, n = a.profile()
        assert n == 1 and ms["distinct"] > 0 and ms["finish"] > 0
    finally:
        a.close()
        b.close()


def anchors_by_sequence(amap, order):
    """the anchors with record numbers translated to the records' identity through `order`"""
    keys, rec, pos = amap.anchors()
    return {int(h): (order[int(r)], int(p)) for h, r, p in zip(keys, rec, pos)}


@pytest.mark.parametrize("w", [15, 1])
def test_add_does_not_depend_on_how_the_records_arrive(oracle, dcn, records, w):
    """one call, one record per call, and reversed within a call: the same anchors modulo record numbering"""
    k = 31
    keys = oracle.Index.build(records, k=k, w=w).keys()
    idx = dcn.Index.from_keys(keys, k, w)
    model = AnchorModel(oracle, k, w, keys).add(records)
    want = model.anchors()
    n = len(records)
    one, each, rev = dcn.AnchorMap(idx), dcn.AnchorMap(idx), dcn.AnchorMap(idx)
    idx.close()  # (a map owns its table)
    try:
        assert one.add_records(records) == 0 and one.add_records([]) == n
        for i, r in enumerate(records):
            assert each.add_records([r]) == i
        assert rev.add_records(records[::-1]) == 0
        ident = list(range(n))
        assert anchors_by_sequence(one, ident) == want
        assert anchors_by_sequence(each, ident) == want
        assert anchors_by_sequence(rev, ident[::-1]) == want
        assert one.info() == each.info() == rev.info() == model.info()
        # a record added again turns every anchor of it into a repeat
        assert one.add_records([records[3]]) == n
        again = AnchorModel(oracle, k, w, keys).add(records + [records[3]])
        assert_map(one, again)
        assert again.info()["repeats"] > model.info()["repeats"] + 100
    finally:
        for m in (one, each, rev):
            m.close()


def test_a_map_anchors_only_the_keys_it_has(oracle, dcn, records):
    """the map is built from the reference's index minus the keys of record 1 (dcn_index_diff): record 1 places nothing"""
    k, w = 31, 15
    full = dcn.Index.from_keys(oracle.Index.build(records, k=k, w=w).keys(), k, w)
    host = dcn.Index.from_keys(oracle.Index.build([records[1]], k=k, w=w).keys(), k, w)
    part = full.diff(host)
    keys = part.keys()
    assert 0 < len(keys) < full.n_keys
    model = AnchorModel(oracle, k, w, keys).add(records)
    amap = dcn.AnchorMap(part)
    for i in (full, host, part):
        i.close()
    amap.add_records(records)
    assert_map(amap, model)
    assert 1 not in {r for r, _ in model.anchors().values()}
    reads = parity_reads(AnchorModel(oracle, k, w, oracle.Index.build(records, k=k, w=w).keys()).add(records), records)
    got = place(dcn, amap, reads, oracle)
    assert_placements(got, model.place_all(reads))
    assert not (got["record"] == 1).any() and (got["record"] == 0).any()
    amap.close()


def test_a_map_is_an_index_and_its_clone_is_a_plain_one(oracle, dcn, built):
    model, amap, reads, _ = built[(31, 15)]
    N, L = dcn._native, dcn._native.lib()
    assert amap.n_keys == len(model.keys) and sorted(amap.keys().tolist()) == sorted(model.keys)
    before = amap.table_bytes
    clone = amap.clone(amap.device)
    assert type(clone) is dcn.Index and clone.n_keys == amap.n_keys and clone.table_bytes == before
    n = C.c_uint64()
    assert L.dcn_anchor_map_info(clone._h, None, None, None, None) == N.DCN_ERR_ARG and b"not an anchor map" in L.dcn_last_error()
    assert L.dcn_anchor_map_anchors(clone._h, None, None, None, 0, C.byref(n)) == N.DCN_ERR_ARG
    with pytest.raises(dcn.DeaconHipError):
        dcn.Placer(clone, max_batch_bases=1 << 16, max_batch_reads=16).place([reads[0]])
    # every call that reads an index sees the map's keys: a filter context over it counts the same hits
    b, o = oracle.concat_reads(reads[:200])
    pa, pb = (dcn.FilterProcessor(i, max_batch_bases=1 << 20, max_batch_reads=1 << 10) for i in (amap, clone))
    assert [x.tolist() for x in pa.filter_batch(b, o)] == [x.tolist() for x in pb.filter_batch(b, o)]
    pa.close(), pb.close(), clone.close()
    # capacity: the count alone, then too small a buffer
    assert L.dcn_anchor_map_anchors(amap._h, None, None, None, 0, C.byref(n)) == N.DCN_ERR_CAPACITY
    assert n.value == model.info()["anchors"]
    keys, rec, pos = (np.full(5, 77, t) for t in (np.uint64, np.uint32, np.uint32))
    ptr = [a.ctypes.data_as(C.c_void_p) for a in (keys, rec, pos)]
    assert L.dcn_anchor_map_anchors(amap._h, *ptr, 5, C.byref(n)) == N.DCN_ERR_CAPACITY and n.value == model.info()["anchors"]
    assert (keys == 77).all() and (rec == 77).all()


def test_argument_errors_with_a_device(oracle, dcn, built):
    model, amap, reads, _ = built[(31, 15)]
    other = dcn.Index.from_keys(np.arange(1, 50, dtype=np.uint64), 31, 1)
    p = dcn.Placer(amap, max_batch_bases=1 << 16, max_batch_reads=4)
    q = dcn.FilterProcessor(other, max_batch_bases=1 << 16, max_batch_reads=4)
    N, L = dcn._native, dcn._native.lib()
    b, o = oracle.concat_reads(reads[:2])
    prm = N.PlaceParams(256, 2, 0, (C.c_uint32 * 2)(0, 0))
    out = np.zeros(8, dcn.filter.PLACEMENT_DTYPE)

    def ptr(a):
        return a.ctypes.data_as(C.c_void_p)

    assert L.dcn_place_batch(q._h, amap._h, ptr(b), ptr(o), 2, C.byref(prm), ptr(out)) == N.DCN_ERR_ARG  # another w
    assert b"differ" in L.dcn_last_error()
    assert L.dcn_anchor_map_add(amap._h, q._h, ptr(b), ptr(o), 2, None) == N.DCN_ERR_ARG
    assert L.dcn_place_batch(p._h, amap._h, ptr(b), ptr(o), 2, C.byref(prm), None) == N.DCN_ERR_ARG
    b5, o5 = oracle.concat_reads(reads[:5])
    assert L.dcn_place_batch(p._h, amap._h, ptr(b5), ptr(o5), 5, C.byref(prm), ptr(out)) == N.DCN_ERR_CAPACITY
    bad = np.array([0, 50, 40], np.uint64)
    before = amap.info()
    assert L.dcn_anchor_map_add(amap._h, p._h, ptr(b), ptr(bad), 2, None) == N.DCN_ERR_ARG  # a refused batch adds nothing
    assert amap.info() == before
    assert L.dcn_place_batch(p._h, amap._h, ptr(b), ptr(o), 2, C.byref(prm), ptr(out)) == 0
    assert_placements(out[:2], model.place_all(reads[:2]))
    p.close(), q.close(), other.close()

"""Split placements on the GPU against the model of tests/_place_split_worker.py, field for field.  Integers only, no
tolerance.  The maps, the reads and the model's rounds are built once per case and left unchanged."""
import ctypes as C

import numpy as np
import pytest

import _place_split_worker as SW
import _place_worker as PW
from _place_split_worker import assert_split, place_split_all

pytestmark = pytest.mark.gpu

# k = 31 at w = 15 and w = 1, k = 32 (a k-mer can be its own reverse complement), k = 33 (128-bit k-mers)
CASES = [(31, 15), (31, 1), (32, 16), (33, 15)]
NS = (1, 2, 4, 8)


@pytest.fixture(scope="module")
def records():
    return PW.make_records(PW.make_genomes())


@pytest.fixture(scope="module")
def built(oracle, dcn, records):
    """(model, map, reads, batch, a Placer) per case"""
    out = {}
    for k, w in CASES:
        model, amap = PW.build_map(oracle, dcn, records, k, w)
        reads = SW.split_reads(model, records) + PW.parity_reads(model, records)[::3]
        placer = dcn.Placer(amap, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
        out[(k, w)] = (model, amap, reads, oracle.concat_reads(reads), placer)
    yield out
    for _, amap, _, _, placer in out.values():
        placer.close()
        amap.close()


@pytest.mark.parametrize("k,w", CASES)
def test_split_placements_equal_the_model(dcn, built, k, w):
    """every max_placements on one context; rank 0 of every read is place_batch's placement of the same batch, and
    read_counts its n_anchors / n_positions, unplaced reads included"""
    model, amap, reads, (b, o), placer = built[(k, w)]
    one = placer.place_batch(b, o)
    for n in NS:
        got = placer.place_split_batch(b, o, max_placements=n)
        po, rows, counts = got
        assert rows.dtype == dcn.filter.SPLIT_PLACEMENT_DTYPE and rows.dtype.itemsize == 64
        assert_split(got, place_split_all(model, reads, max_placements=n), (k, w, n))
        placed = one["record"] != PW.UNPLACED
        assert (np.diff(po.astype(np.int64)) > 0).tolist() == placed.tolist()
        first = rows[po[:-1][placed].astype(np.int64)]
        assert (first["rank"] == 0).all()
        for f in dcn.filter.PLACEMENT_DTYPE.names:
            assert (first[f] == one[f][placed]).all(), (k, w, n, f)
        assert (counts[:, 0] == one["n_anchors"]).all() and (counts[:, 1] == one["n_positions"]).all()
        assert int((~placed).sum()) > 15 and (rows["mapq"] <= 60).all()
        if n >= 2:
            per = np.diff(po.astype(np.int64))
            assert int((per >= 2).sum()) > 100 and int((rows["mapq"] == 60).sum()) > 200 and int((rows["rival_votes"] > 0).sum()) > 20
        if n == 8:
            assert int(per.max()) >= 4
    assert placer.place_batch(b, o).tobytes() == one.tobytes()  # and place_batch after place_split_batch


@pytest.mark.parametrize("k,w", [(31, 15), (31, 1)])
def test_prefix_band_and_min_votes(oracle, dcn, built, k, w):
    model, amap, reads, _, _ = built[(k, w)]
    SW.check_split(dcn, oracle, model, amap, reads, (k, w), prefix_length=60)
    for W, votes, n in ((1, 1, 8), (31, 3, 4), (64, 5, 2), (1 << 20, 2, 4), (0xFFFFFFFF, 2, 2)):
        SW.check_split(dcn, oracle, model, amap, reads, (k, w), max_placements=n, band_bases=W, min_votes=votes)


def test_capacity(dcn, built):
    """a count-only call, the exact capacity, and one short: DCN_ERR_CAPACITY with complete offsets and nothing written"""
    N = dcn._native
    model, amap, reads, (b, o), placer = built[(31, 15)]
    want = place_split_all(model, reads, max_placements=4)
    total = want[0][-1]
    n = len(reads)
    prm = N.PlaceSplitParams(256, 2, 0, 4, (C.c_uint32 * 3)(0, 0, 0))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    po, counts = np.zeros(n + 1, np.uint64), np.zeros((n, 2), np.uint32)
    call = lambda rows, cap, cnt: N.lib().dcn_place_split_batch(placer._h, amap._h, ptr(b), ptr(o), n, C.byref(prm), ptr(po),  # noqa: E731
                                                                 ptr(rows) if rows is not None else None, cap, cnt)
    assert call(None, 0, None) == N.DCN_ERR_CAPACITY
    assert str(total) in N.lib().dcn_last_error().decode() and po.tolist() == want[0]
    rows = np.frombuffer(bytearray(b"\xAB" * (64 * total)), dcn.filter.SPLIT_PLACEMENT_DTYPE)
    po[:] = 0
    assert call(rows, total - 1, ptr(counts)) == N.DCN_ERR_CAPACITY
    assert po.tolist() == want[0] and rows.tobytes() == b"\xAB" * (64 * total)
    assert call(rows, total, ptr(counts)) == N.DCN_OK
    assert_split((po, rows, counts), want)
    with pytest.raises(dcn.DeaconHipError) as e:
        placer.place_split_batch(b, o, max_placements=4, capacity=total - 1)
    assert e.value.code == N.DCN_ERR_CAPACITY
    assert_split(placer.place_split_batch(b, o, max_placements=4, capacity=total), want)


def test_no_reads_and_lists(dcn, built):
    model, amap, reads, _, placer = built[(31, 15)]
    po, rows, counts = placer.place_split_batch(np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    assert po.tolist() == [0] and len(rows) == 0 and counts.shape == (0, 2)
    per = placer.place_split(reads[:9], max_placements=2)
    want = [SW.place_split(model, r, max_placements=2)[0] for r in reads[:9]]
    assert [[tuple(int(x[f]) for f in SW.SPLIT_FIELDS) for x in rows] for rows in per] == want
    assert placer.place_split([]) == []


def test_one_context_serves_place_split_locate_in_turn(oracle, dcn, built):
    """place_batch, place_split_batch, dcn_locate_batch and place_split_batch again on ONE context (the position bitmap
    is shared with locate): each call gives its own answer, and profiling covers the new call"""
    N = dcn._native
    model, amap, reads, (b, o), placer = built[(31, 15)]
    n = len(reads)
    want = place_split_all(model, reads, max_placements=4)
    one = placer.place_batch(b, o)
    assert_split(placer.place_split_batch(b, o), want)
    loc = dcn.Locator(amap, max_gap=0, min_hits=1, max_batch_bases=1 << 20, max_batch_reads=1 << 12)  # the same keys on a context of its own
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
    assert_split(placer.place_split_batch(b, o), want)
    ms, batches = placer.profile()
    assert batches == 1 and ms["distinct"] > 0 and ms["finish"] > 0
    placer.set_profiling(False)
    assert placer.place_batch(b, o).tobytes() == one.tobytes()

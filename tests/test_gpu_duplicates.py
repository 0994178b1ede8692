"""dcn_mark_duplicates_batch / AnchorMap.mark_duplicates against the dict model of tests/_duplicates_worker.py, on rows built
by hand: flags, `first` and the three numbers of `info`, in single and paired mode, with and without both_ends, over the three
row strides, with and without row_offsets, on a map that keeps bases and on one that does not; the same input cut into 1, 2
and 7 uneven calls; reset; enabling twice; a map without a set; a bad row; optional outputs.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import _duplicates_worker as DW

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def maps(dcn, oracle):
    with_bases, without = DW.make_map(oracle, dcn, True), DW.make_map(oracle, dcn, False)
    yield with_bases, without
    with_bases.close()
    without.close()


@pytest.fixture
def amap(maps):
    """the map that keeps bases, with a set that is empty"""
    maps[0].duplicates_enable()
    maps[0].duplicates_reset()
    return maps[0]


@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
@pytest.mark.parametrize("stride", [0, 1, 2], ids=["48", "64", "80"])
def test_flags_first_and_info_against_the_model(dcn, amap, stride, paired):
    rng = np.random.default_rng(100 + stride * 2 + paired)
    dtype = DW.dtypes(dcn)[stride]
    for both_ends in (False, True):
        amap.duplicates_reset()
        model = DW.Model()
        lengths, rows = DW.random_units(rng, 300, 0.3, DW.REC_LENS, paired=paired)
        dup, first = DW.check(dcn, amap, model, dtype, lengths, rows, paired, both_ends)
        assert 40 < sum(dup) < 150 and (paired or DW.NO_FIRST in first)  # the model alone: duplicates and units without a key are there
        # ... and a second call against what the first left, one row per read and no row_offsets
        lengths2 = lengths[:200]
        rows2 = [[next((x for x in r if x is not None), None)] for r in rows[:200]]
        dup2, _ = DW.check(dcn, amap, model, dtype, lengths2, rows2, paired, both_ends, with_row_offsets=False)
        assert sum(dup2) > 50


def test_a_map_that_keeps_no_bases(dcn, maps):
    """D1: neither kept bases nor a pileup.  Such a map has no record lengths, so a ref_end past any record is taken"""
    amap = maps[1]
    assert not amap.keeps_bases
    amap.duplicates_enable()
    amap.duplicates_reset()
    model = DW.Model()
    rng = np.random.default_rng(3)
    lengths, rows = DW.random_units(rng, 300, 0.3, [10 ** 7, 10 ** 7, 10 ** 7])
    dup, _ = DW.check(dcn, amap, model, DW.dtypes(dcn)[1], lengths, rows)
    assert sum(dup) > 40
    big = [(2, 1, 3, 100, 2 ** 40, 2 ** 40 + 97)]
    assert DW.check(dcn, amap, model, DW.dtypes(dcn)[0], [100, 100], [big, big], both_ends=True) == ([0, 1], [300, 300])
    with pytest.raises(dcn.DeaconHipError) as e:  # the number of records is still known
        DW.mark(dcn, amap, DW.dtypes(dcn)[0], [100], [[(3, 0, 0, 100, 0, 100)]])
    assert e.value.code == dcn._native.DCN_ERR_ARG and "row 0: record 3 of 3 added" in e.value.message
    amap.duplicates_disable()


@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
def test_the_same_units_in_one_two_and_seven_uneven_calls(dcn, amap, paired):
    rng = np.random.default_rng(11 + paired)
    per = 2 if paired else 1
    lengths, rows = DW.random_units(rng, 300, 0.4, DW.REC_LENS, paired=paired)
    dtype = DW.dtypes(dcn)[1]
    results = []
    for cuts in ([], [137], [1, 2, 65, 66, 200, 299]):
        amap.duplicates_reset()
        model = DW.Model()
        dup, first = [], []
        for part_lengths, part_rows in DW.split(lengths, rows, cuts, per):
            d, f = DW.check(dcn, amap, model, dtype, part_lengths, part_rows, paired, True)
            dup += d
            first += f
        results.append((dup, first, amap.duplicates_info()))
    assert results[0] == results[1] == results[2] and sum(results[0][0]) > 60 and results[0][2][0] == 300


def test_reset_restarts_the_ordinals_and_enabling_twice_is_a_no_op(dcn, amap):
    dtype = DW.dtypes(dcn)[0]
    r = lambda pos: [(0, 0, 0, 50, pos, pos + 50)]
    assert DW.mark(dcn, amap, dtype, [50] * 3, [r(10), r(20), r(10)]) == ([0, 0, 1], [0, 1, 0])
    assert amap.duplicates_info() == (3, 3, 2)
    amap.duplicates_enable()  # again: nothing changes
    assert amap.duplicates_info() == (3, 3, 2)
    assert DW.mark(dcn, amap, dtype, [50] * 2, [r(20), r(30)]) == ([1, 0], [1, 4])
    assert amap.duplicates_info() == (5, 5, 3)
    amap.duplicates_reset()
    assert amap.duplicates_info() == (0, 0, 0)
    assert DW.mark(dcn, amap, dtype, [50] * 2, [r(20), r(10)]) == ([0, 0], [0, 1])  # nothing of before is remembered
    assert amap.duplicates_info() == (2, 2, 2)
    amap.duplicates_disable()  # off and on again: an empty set
    amap.duplicates_disable()
    amap.duplicates_enable()
    assert amap.duplicates_info() == (0, 0, 0)
    assert DW.mark(dcn, amap, dtype, [50], [r(20)]) == ([0], [0])


def test_a_map_without_a_set_and_an_index_that_is_no_map(dcn, oracle, maps):
    N = dcn._native
    amap = maps[0]
    amap.duplicates_disable()
    for call in (lambda: amap.duplicates_info(), lambda: amap.duplicates_reset(),
                 lambda: DW.mark(dcn, amap, DW.dtypes(dcn)[0], [50], [[(0, 0, 0, 50, 0, 50)]])):
        with pytest.raises(dcn.DeaconHipError) as e:
            call()
        assert e.value.code == N.DCN_ERR_ARG and "the map keeps no duplicate set (dcn_anchor_map_duplicates_enable)" in e.value.message
    plain = amap.clone(amap.device)  # a clone is a plain index, and it has no set
    try:
        for enable in (1, 0):
            assert N.lib().dcn_anchor_map_duplicates_enable(plain._h, enable) == N.DCN_ERR_ARG
            assert b"the index is not an anchor map" in N.lib().dcn_last_error()
    finally:
        plain.close()
    amap.duplicates_enable()
    clone = amap.clone(amap.device)
    clone.close()
    assert amap.duplicates_info() == (0, 0, 0)


def test_a_refused_call_changes_nothing_that_info_reports(dcn, amap):
    """dcn_verify_batch's checks in its order and with its messages, and the paired ones; the set and seen stay as they were"""
    N = dcn._native
    dtype = DW.dtypes(dcn)[1]
    model = DW.Model()
    good = [(0, 0, 0, 50, 10, 60)]
    DW.check(dcn, amap, model, dtype, [50] * 3, [good, [(1, 1, 0, 50, 10, 60)], good])
    before = amap.duplicates_info()
    assert before == (3, 3, 2)
    bad_rows = [((3, 0, 0, 50, 10, 60), "row 1: record 3 of 3 added"),
                ((0, 2, 0, 50, 10, 60), "row 1: reverse must be 0 or 1"),
                ((0, 0, 9, 8, 10, 60), "row 1: read_start is behind read_end"),
                ((0, 0, 0, 51, 10, 60), "row 1: read_end 51 is past the read's 50 bases"),
                ((0, 0, 0, 50, 61, 60), "row 1: ref_start is behind ref_end"),
                ((0, 0, 0, 50, 990, 1001), "row 1: ref_end 1001 is past the record's 1000 bases")]
    for row, message in bad_rows:
        with pytest.raises(dcn.DeaconHipError) as e:
            DW.mark(dcn, amap, dtype, [50] * 3, [good, [row], good])
        assert e.value.code == N.DCN_ERR_ARG and message in e.value.message, (message, e.value.message)
        assert amap.duplicates_info() == before
    offsets, rows, _ = DW.pack(dcn, dtype, [50] * 3, [good, good, good])

    def raw(offsets=offsets, n_reads=3, row_offsets=None, rows=rows, n_rows=3, paired=0):
        p = N.DuplicateParams(dtype.itemsize, paired, 0, 0)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
        rc = N.lib().dcn_mark_duplicates_batch(amap._h, ptr(offsets), n_reads, C.byref(p), ptr(row_offsets), ptr(rows), n_rows, None, None, None)
        return rc, N.lib().dcn_last_error()

    ro = lambda *x: np.array(x, np.uint64)
    for kwargs, message in ((dict(n_rows=2), b"without row_offsets row r belongs to read r: n_rows must equal n_reads"),
                            (dict(paired=1), b"n_reads must be even"),
                            (dict(offsets=None), b"offsets is NULL"),
                            (dict(offsets=ro(1, 50, 100, 150)), b"offsets[0] must be 0"),
                            (dict(offsets=ro(0, 50, 40, 150)), b"offsets must be non-decreasing"),
                            (dict(row_offsets=ro(1, 1, 2, 3)), b"row_offsets[0] must be 0"),
                            (dict(row_offsets=ro(0, 2, 1, 3)), b"row_offsets must be non-decreasing"),
                            (dict(row_offsets=ro(0, 1, 2, 2)), b"row_offsets must end at n_rows"),
                            (dict(rows=None), b"rows is NULL")):
        rc, text = raw(**kwargs)
        assert rc == N.DCN_ERR_ARG and message in text, (kwargs, text)
        assert amap.duplicates_info() == before
    # ... and the next good call goes on from there
    assert DW.check(dcn, amap, model, dtype, [50] * 2, [good, [(2, 0, 0, 50, 10, 60)]]) == ([1, 0], [0, 4])


def test_null_outputs_and_empty_calls(dcn, amap):
    N = dcn._native
    dtype = DW.dtypes(dcn)[2]
    r = lambda pos: [(1, 1, 0, 50, pos, pos + 50)]
    offsets, rows, _ = DW.pack(dcn, dtype, [50] * 4, [r(10), r(10), r(30), r(10)])
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    p = N.DuplicateParams(dtype.itemsize, 0, 1, 0)
    n_dup = C.c_uint64(99)
    assert N.lib().dcn_mark_duplicates_batch(amap._h, ptr(offsets), 4, C.byref(p), None, ptr(rows), 4, None, None, C.byref(n_dup)) == 0
    assert n_dup.value == 2 and amap.duplicates_info() == (4, 4, 2)
    dup, first = np.full(4, 9, np.uint8), np.full(4, 9, np.uint64)
    assert N.lib().dcn_mark_duplicates_batch(amap._h, ptr(offsets), 4, C.byref(p), None, ptr(rows), 4, ptr(dup), None, None) == 0
    assert dup.tolist() == [1, 1, 1, 1] and amap.duplicates_info() == (8, 8, 2)
    assert N.lib().dcn_mark_duplicates_batch(amap._h, ptr(offsets), 4, C.byref(p), None, ptr(rows), 4, None, ptr(first), C.byref(n_dup)) == 0
    assert first.tolist() == [0, 0, 2, 0] and n_dup.value == 4 and amap.duplicates_info() == (12, 12, 2)
    # no reads: nothing happens; reads without rows: units without keys, which consume ordinals
    assert N.lib().dcn_mark_duplicates_batch(amap._h, None, 0, C.byref(p), None, None, 0, None, None, C.byref(n_dup)) == 0
    assert n_dup.value == 0 and amap.duplicates_info() == (12, 12, 2)
    ro = np.zeros(4, np.uint64)
    assert N.lib().dcn_mark_duplicates_batch(amap._h, ptr(offsets), 3, C.byref(p), ptr(ro), None, 0, ptr(dup), ptr(first), C.byref(n_dup)) == 0
    assert dup[:3].tolist() == [0, 0, 0] and first[:3].tolist() == [DW.NO_FIRST] * 3 and n_dup.value == 0
    assert amap.duplicates_info() == (15, 12, 2)


def test_adding_records_stays_allowed_and_nothing_else_moves(dcn, oracle):
    """dcn_anchor_map_add while a set is kept; the map's own info and its kept bases are what they were"""
    from conftest import random_reads
    amap = DW.make_map(oracle, dcn, True, rec_lens=[500, 400], seed=5)
    try:
        amap.duplicates_enable()
        dtype = DW.dtypes(dcn)[0]
        before = amap.fetch(1, 0, 400)
        with pytest.raises(dcn.DeaconHipError):
            DW.mark(dcn, amap, dtype, [50], [[(2, 0, 0, 50, 0, 50)]])
        assert DW.mark(dcn, amap, dtype, [50], [[(1, 0, 0, 50, 0, 50)]]) == ([0], [0])
        amap.add_records([random_reads(np.random.default_rng(6), 1, 300, 300)[0]])
        assert amap.info()["records"] == 3 and amap.fetch(1, 0, 400) == before
        assert DW.mark(dcn, amap, dtype, [50] * 2, [[(2, 0, 0, 50, 0, 50)], [(1, 0, 5, 50, 5, 50)]]) == ([0, 1], [1, 0])
        assert amap.duplicates_info() == (3, 3, 2)
    finally:
        amap.close()

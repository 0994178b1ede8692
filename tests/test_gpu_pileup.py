"""dcn_pileup_batch on the rows the three placement calls return, against the model of tests/_pileup_worker.py (the runs of
a full table walked step by step into a numpy array: no wavefront, no prefix sums, no planes): the reads of
tests/test_gpu_align.py at (k, w) = (31, 15) and (31, 1).  How a batch is cut and ordered, select, reset, fetch of
sub-ranges, enable and disable, n_added, edits, and one context serving align, pileup, verify and pileup again.  Every
comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import _align_worker as AW
import _pileup_worker as PW
import _verify_worker as VW
from test_gpu_align import make_reads, make_records

pytestmark = pytest.mark.gpu

CASES = [(31, 15), (31, 1)]
OVER, UNPLACED = VW.OVER, VW.UNPLACED


@pytest.fixture(scope="module")
def built(dcn, oracle):
    records = make_records()
    reads = make_reads(records)
    out = {}
    for k, w in CASES:
        amap = VW.build_map(oracle, dcn, records, k, w)
        amap.pileup_enable()
        placer = dcn.Placer(amap, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
        out[(k, w)] = (amap, placer)
    yield records, reads, oracle.concat_reads(reads), out
    for amap, placer in out.values():
        placer.close()
        amap.close()


@pytest.mark.parametrize("k,w", CASES)
def test_rows_of_the_three_placement_calls(built, dcn, k, w):
    records, reads, (b, o), maps = built
    amap, placer = maps[(k, w)]
    po, srows, _ = placer.place_split_batch(b, o, max_placements=4)
    prows, _ = placer.place_pair_batch(b, o)
    for rows, ro in ((placer.place_batch(b, o), None), (srows, po), (prows, None)):
        amap.pileup_reset()
        edits, n_added = placer.pileup_batch(b, o, rows, row_offsets=ro)
        counts = PW.new_counts(records)
        want_edits, want_added = PW.pile_rows(counts, reads, records, rows, row_offsets=ro)
        assert edits.tolist() == want_edits.tolist() == placer.verify_batch(b, o, rows, row_offsets=ro).tolist()
        assert n_added == want_added == (edits < OVER).sum() and 60 < n_added <= len(rows)
        assert ro is not None or (edits == UNPLACED).sum() >= 5  # (one row per read: the unplaced reads have rows too)
        PW.assert_counts(amap, records, counts)
        total = sum(c.sum(axis=0) for c in counts)
        assert all(total[col] > 0 for col in range(PW.COLUMNS)), total  # every column is met, N and REV included
        assert any((c[:, :6].sum(axis=1) > 1).any() for c in counts)  # reads overlap: positions with several adds
        for R in range(3):
            PW.assert_calls(amap, records, counts, R)
            PW.assert_calls(amap, records, counts, R, 1000, 9000, min_depth=1, min_permille=900)


def test_cut_and_order_do_not_matter(built, dcn):
    """one batch = the same rows in three calls = the rows in reverse order (rule P5)"""
    records, reads, (b, o), maps = built
    amap, placer = maps[(31, 15)]
    po, srows, _ = placer.place_split_batch(b, o, max_placements=4)
    po = po.astype(np.int64)
    amap.pileup_reset()
    _, whole_added = placer.pileup_batch(b, o, srows, row_offsets=po)
    whole = [amap.pileup_fetch(R).copy() for R in range(3)]
    amap.pileup_reset()
    added = 0
    for lo, hi in ((0, 17), (17, 18), (18, len(reads))):
        cb, co = dcn.concat_reads(reads[lo:hi])
        added += placer.pileup_batch(cb, co, srows[po[lo]:po[hi]], row_offsets=po[lo:hi + 1] - po[lo])[1]
    assert added == whole_added
    assert all(np.array_equal(amap.pileup_fetch(R), whole[R]) for R in range(3))
    # one row per read (dcn_place_batch's), forwards and backwards
    rows = placer.place_batch(b, o)
    amap.pileup_reset()
    placer.pileup_batch(b, o, rows)
    forwards = [amap.pileup_fetch(R).copy() for R in range(3)]
    amap.pileup_reset()
    rb, ro = dcn.concat_reads(reads[::-1])
    placer.pileup_batch(rb, ro, rows[::-1].copy())
    assert all(np.array_equal(amap.pileup_fetch(R), forwards[R]) for R in range(3))
    # without a reset the counters go on: twice the rows, twice the counts
    placer.pileup_batch(b, o, rows)
    assert all(np.array_equal(amap.pileup_fetch(R), 2 * forwards[R]) for R in range(3))


def test_select_reset_and_fetch(built, dcn):
    records, reads, (b, o), maps = built
    amap, placer = maps[(31, 15)]
    rows = placer.place_batch(b, o)
    keep = np.random.default_rng(1511).random(len(rows)) < 0.6
    before = rows.copy()
    amap.pileup_reset()
    edits, n_added = placer.pileup_batch(b, o, rows, select=keep)
    assert rows.tobytes() == before.tobytes()  # the mask is applied in a copy
    assert (edits[~keep] == UNPLACED).all()
    selected = [amap.pileup_fetch(R).copy() for R in range(3)]
    amap.pileup_reset()
    assert all(not amap.pileup_fetch(R).any() for R in range(3))
    sb, so = dcn.concat_reads([r for r, k_ in zip(reads, keep) if k_])
    _, left_added = placer.pileup_batch(sb, so, rows[keep])  # the same rows, the others left out
    assert left_added == n_added > 20
    assert all(np.array_equal(amap.pileup_fetch(R), selected[R]) for R in range(3))
    counts = PW.new_counts(records)
    assert PW.pile_rows(counts, reads, records, rows, select=keep)[1] == n_added
    PW.assert_counts(amap, records, counts)
    # sub-ranges, position-major, and n = 0
    full = PW.as_u32(counts[1])
    for start, n in ((0, 1), (0, 31), (31, 2), (4999, 301), (19_999, 1), (20_000, 0), (0, 0), (7, 0)):
        got = amap.pileup_fetch(1, start, n)
        assert got.shape == (n, 8) and np.array_equal(got, full[start:start + n]), (start, n)
    N = dcn._native
    assert N.lib().dcn_anchor_map_pileup_fetch(amap._h, 1, 0, 0, None) == 0  # n_bases = 0 needs no buffer
    for args, word in (((3, 0, 1), b"record 3 of 3 added"), ((1, 20_000, 1), b"past the record's 20000 bases"), ((1, 0, 20_001), b"past the record's")):
        out = np.zeros((8, 8), np.uint32)
        assert N.lib().dcn_anchor_map_pileup_fetch(amap._h, *args, out.ctypes.data_as(C.c_void_p)) == N.DCN_ERR_ARG
        assert word in N.lib().dcn_last_error()
    assert N.lib().dcn_anchor_map_pileup_fetch(amap._h, 1, 0, 4, None) == N.DCN_ERR_ARG and b"counts is NULL" in N.lib().dcn_last_error()


def test_enable_and_disable(built, dcn, oracle):
    records, reads, (b, o), maps = built
    N = dcn._native
    L = N.lib()
    # a map that keeps no bases has no pileup; neither has an index that is no map
    plain = VW.build_map(oracle, dcn, records[:1], keep_bases=False)
    with pytest.raises(dcn.DeaconHipError) as e:
        plain.pileup_enable()
    assert e.value.code == N.DCN_ERR_ARG and "keeps no bases" in e.value.message
    index = plain.clone(0)
    assert L.dcn_anchor_map_pileup_enable(index._h, 1) == N.DCN_ERR_ARG and b"not an anchor map" in L.dcn_last_error()
    index.close()
    plain.close()
    amap = VW.build_map(oracle, dcn, records[:2])
    placer = dcn.Placer(amap, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    rows = placer.place_batch(b, o)
    for call in (lambda: placer.pileup_batch(b, o, rows), lambda: amap.pileup_fetch(0, 0, 4), amap.pileup_reset, lambda: amap.pileup_call(0, 0, 4)):
        with pytest.raises(dcn.DeaconHipError) as e:
            call()
        assert e.value.code == N.DCN_ERR_ARG and "no pileup" in e.value.message
    amap.pileup_disable()  # (nothing to free)
    amap.pileup_enable()
    _, n_added = placer.pileup_batch(b, o, rows)
    held = amap.pileup_fetch(0).copy()
    assert n_added > 20 and held.any()
    amap.pileup_enable()  # again: nothing changes
    assert np.array_equal(amap.pileup_fetch(0), held)
    with pytest.raises(dcn.DeaconHipError) as e:
        amap.add_records(records[2:])
    assert e.value.code == N.DCN_ERR_ARG and "pileup" in e.value.message and amap.info()["records"] == 2
    clone = amap.clone(0)  # an index without the words, the bases and the pileup
    out = np.zeros((4, 8), np.uint32)
    assert L.dcn_anchor_map_pileup_fetch(clone._h, 0, 0, 4, out.ctypes.data_as(C.c_void_p)) == N.DCN_ERR_ARG
    clone.close()
    amap.pileup_disable()
    with pytest.raises(dcn.DeaconHipError):
        amap.pileup_fetch(0, 0, 4)
    assert amap.add_records(records[2:]) == 2  # without a pileup the map takes records as before
    amap.pileup_enable()  # ... and a new pileup covers them, from zero
    assert amap.pileup_fetch(2).shape == (20_000, 8) and not amap.pileup_fetch(0).any()
    placer.close()
    amap.close()


def test_one_context_serves_every_call(built, dcn):
    """align, pileup, verify and pileup again on one context; align's results are what they are on a map without a pileup;
    the six counters stay; profiling sees pack and finish"""
    records, reads, (b, o), maps = built
    amap, placer = maps[(31, 15)]
    po, srows, _ = placer.place_split_batch(b, o)
    want = AW.align_rows(reads, records, srows, row_offsets=po)
    first = placer.align_batch(b, o, srows, row_offsets=po)
    AW.assert_same(first, want, srows)
    amap.pileup_reset()
    edits, n_added = placer.pileup_batch(b, o, srows, row_offsets=po)
    once = [amap.pileup_fetch(R).copy() for R in range(3)]
    assert edits.tolist() == first[0].tolist() == placer.verify_batch(b, o, srows, row_offsets=po).tolist()
    again = placer.align_batch(b, o, srows, row_offsets=po)
    assert all(np.array_equal(x, y) for x, y in zip(first, again))
    before = placer.stats()
    placer.set_profiling(True)
    assert placer.pileup_batch(b, o, srows, row_offsets=po)[1] == n_added
    ms, n = placer.profile()
    placer.set_profiling(False)
    assert n == 1 and ms["pack"] > 0 and ms["finish"] > 0 and placer.stats() == before
    assert all(np.array_equal(amap.pileup_fetch(R), 2 * once[R]) for R in range(3))
    # the same map without its pileup: dcn_align_batch byte for byte
    amap.pileup_disable()
    bare = placer.align_batch(b, o, srows, row_offsets=po)
    amap.pileup_enable()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(first, bare))
    # the argument errors of this call alone come behind dcn_verify_batch's, whose messages it carries
    bad = srows.copy()
    bad["ref_end"][3] = 20_001
    with pytest.raises(dcn.DeaconHipError) as e:
        placer.pileup_batch(b, o, bad, row_offsets=po)
    assert e.value.code == dcn._native.DCN_ERR_ARG and "row 3: ref_end 20001 is past the record's 20000 bases" in e.value.message
    assert not any(amap.pileup_fetch(R).any() for R in range(3))  # (fresh from enable, and the refused call added nothing)

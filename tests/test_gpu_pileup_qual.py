"""The quality-aware pileup on the rows the placement calls return, against the model of tests/_quality_worker.py (the runs of
the unmasked read walked one step at a time: no lanes, no planes, no prefix sums): the reads of tests/test_gpu_align.py with
random qualities, at (k, w) = (31, 15) and (31, 1), with the rows of place_batch, place_split_batch and extend_batch, at
thresholds 0, 20 and 255.  Threshold 0 against dcn_pileup_batch, edits against dcn_verify_batch, how a batch is cut and
ordered, select, reset, keep and its refusals, disable, clone, the ledger beside it, dcn_align_batch beside it, and a map
without sums.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import _align_worker as AW
import _insertion_worker as IW
import _pileup_worker as PW
import _quality_worker as QW
import _verify_worker as VW
from test_gpu_align import make_reads, make_records

pytestmark = pytest.mark.gpu

CASES = [(31, 15), (31, 1)]


@pytest.fixture(scope="module")
def built(dcn, oracle):
    records = make_records()
    reads = make_reads(records)
    quals = QW.random_quals(np.random.default_rng(1801), reads)
    out = {}
    for k, w in CASES:
        amap = VW.build_map(oracle, dcn, records, k, w)
        amap.pileup_enable()
        amap.pileup_keep_insertions()
        amap.pileup_keep_qualities()
        placer = dcn.Placer(amap, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
        out[(k, w)] = (amap, placer)
    yield records, reads, quals, QW.concat(oracle, reads, quals), out
    for amap, placer in out.values():
        placer.close()
        amap.close()


def fetched(amap, n_records=3):
    """counters and sums as bytes: what two maps fed the same rows and qualities must agree on"""
    return [(amap.pileup_fetch(R).tobytes(), amap.pileup_fetch_qualities(R).tobytes()) for R in range(n_records)]


@pytest.mark.parametrize("k,w", CASES)
def test_rows_of_the_placement_calls(built, dcn, k, w):
    records, reads, quals, (b, o, q), maps = built
    amap, placer = maps[(k, w)]
    po, srows, _ = placer.place_split_batch(b, o, max_placements=4)
    xrows, _ = placer.extend_batch(b, o, srows, row_offsets=po)
    for rows, ro in ((placer.place_batch(b, o), None), (srows, po), (xrows, po)):
        for threshold in (0, 20, 255):
            amap.pileup_reset()
            assert not amap.pileup_fetch_qualities(0).any()
            edits, n_added = placer.pileup_batch(b, o, rows, row_offsets=ro, quals=q, min_base_qual=threshold)
            counts, sums, ledger = PW.new_counts(records), QW.new_sums(records), IW.new_ledger(records)
            want_edits, want_added = QW.pile_rows(counts, sums, ledger, reads, quals, records, rows, row_offsets=ro, min_base_qual=threshold)
            assert edits.tolist() == want_edits.tolist() and n_added == want_added > 60
            assert edits.tolist() == placer.verify_batch(b, o, rows, row_offsets=ro).tolist()  # rule Q6
            PW.assert_counts(amap, records, counts)
            QW.assert_sums(amap, records, sums)
            # calls and consensus read the counters (P6, L6, L7 unchanged)
            IW.assert_ledger(amap, records, counts, ledger, fills=(False,))
            n_low = sum(int(c[:, PW.N].sum()) for c in counts)
            total = sum(int(s.sum()) for s in sums)
            if threshold == 255:
                assert total == 0 and all(not c[:, :4].any() for c in counts)  # (no quality reaches 255 at offset 33)
            else:
                assert total > 10_000 and (n_low > 1000) == (threshold == 20)


def test_threshold_zero_is_the_plain_call(built, dcn, oracle):
    """rule Q3: with min_base_qual = 0 the eight counters are dcn_pileup_batch's on a second map, and so is the ledger"""
    records, reads, quals, (b, o, q), maps = built
    amap, placer = maps[(31, 15)]
    po, srows, _ = placer.place_split_batch(b, o)
    amap.pileup_reset()
    edits, n_added = placer.pileup_batch(b, o, srows, row_offsets=po, quals=q, min_base_qual=0)
    plain = VW.build_map(oracle, dcn, records)
    plain.pileup_enable()
    plain.pileup_keep_insertions()
    other = dcn.Placer(plain, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    e2, n2 = other.pileup_batch(b, o, srows, row_offsets=po)
    assert edits.tolist() == e2.tolist() and n_added == n2 > 60
    for R in range(3):
        assert np.array_equal(amap.pileup_fetch(R), plain.pileup_fetch(R))
        assert [x.tobytes() if hasattr(x, "tobytes") else x for x in amap.insertions_fetch(R)] == \
               [x.tobytes() if hasattr(x, "tobytes") else x for x in plain.insertions_fetch(R)]  # rule Q5
    assert amap.insertions_info() == plain.insertions_info() and amap.insertions_info()[0] > 20
    # the same at threshold 20: the events do not depend on the qualities
    amap.pileup_reset()
    placer.pileup_batch(b, o, srows, row_offsets=po, quals=q, min_base_qual=20)
    for R in range(3):
        assert [x.tobytes() if hasattr(x, "tobytes") else x for x in amap.insertions_fetch(R)] == \
               [x.tobytes() if hasattr(x, "tobytes") else x for x in plain.insertions_fetch(R)]
        assert np.array_equal(amap.pileup_fetch(R)[:, 5:], plain.pileup_fetch(R)[:, 5:])  # DEL, INS, REV are P3's
        assert np.array_equal(amap.pileup_fetch(R)[:, :5].sum(axis=1), plain.pileup_fetch(R)[:, :5].sum(axis=1))  # P4
    # a map without sums still takes the call: rule Q3 alone
    plain.pileup_reset()
    e3, n3 = other.pileup_batch(b, o, srows, row_offsets=po, quals=q, min_base_qual=20)
    assert e3.tolist() == edits.tolist() and n3 == n_added
    for R in range(3):
        assert np.array_equal(amap.pileup_fetch(R), plain.pileup_fetch(R))
    with pytest.raises(dcn.DeaconHipError) as e:
        plain.pileup_fetch_qualities(0)
    assert e.value.code == dcn._native.DCN_ERR_ARG and "keeps no quality sums" in e.value.message
    other.close()
    plain.close()


def test_cut_and_order_do_not_matter(built, dcn):
    """one batch = the same rows in three calls = the rows in reverse order (rule Q6), and select"""
    records, reads, quals, (b, o, q), maps = built
    amap, placer = maps[(31, 15)]
    po, srows, _ = placer.place_split_batch(b, o, max_placements=4)
    po = po.astype(np.int64)
    amap.pileup_reset()
    placer.pileup_batch(b, o, srows, row_offsets=po, quals=q, min_base_qual=20)
    whole = fetched(amap)
    amap.pileup_reset()
    for lo, hi in ((0, 17), (17, 18), (18, len(reads))):
        cb, co, cq = QW.concat(dcn, reads[lo:hi], quals[lo:hi])
        placer.pileup_batch(cb, co, srows[po[lo]:po[hi]], row_offsets=po[lo:hi + 1] - po[lo], quals=cq, min_base_qual=20)
    assert fetched(amap) == whole
    rows = placer.place_batch(b, o)
    amap.pileup_reset()
    placer.pileup_batch(b, o, rows, quals=q, min_base_qual=20)
    forwards = fetched(amap)
    amap.pileup_reset()
    rb, ro, rq = QW.concat(dcn, reads[::-1], quals[::-1])
    placer.pileup_batch(rb, ro, rows[::-1].copy(), quals=rq.tobytes(), min_base_qual=20)  # (bytes are taken as well)
    assert fetched(amap) == forwards
    keep = np.random.default_rng(1711).random(len(rows)) < 0.6
    amap.pileup_reset()
    placer.pileup_batch(b, o, rows, select=keep, quals=q, min_base_qual=20)
    selected = fetched(amap)
    amap.pileup_reset()
    sb, so, sq = QW.concat(dcn, [r for r, k_ in zip(reads, keep) if k_], [x for x, k_ in zip(quals, keep) if k_])
    placer.pileup_batch(sb, so, rows[keep], quals=sq, min_base_qual=20)
    assert fetched(amap) == selected != forwards
    for bad in (q[:-1], q.astype(np.uint16), "IIII", np.zeros((2, len(q) // 2), np.uint8)):
        with pytest.raises(ValueError):
            placer.pileup_batch(b, o, rows, quals=bad)
    assert fetched(amap) == selected


def test_keep_reset_disable_and_clone(built, dcn, oracle):
    records, reads, quals, (b, o, q), maps = built
    N = dcn._native
    L = N.lib()
    amap = VW.build_map(oracle, dcn, records)
    placer = dcn.Placer(amap, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    rows = placer.place_batch(b, o)
    with pytest.raises(dcn.DeaconHipError) as e:
        amap.pileup_keep_qualities()
    assert e.value.code == N.DCN_ERR_ARG and "no pileup" in e.value.message
    amap.pileup_enable()
    with pytest.raises(dcn.DeaconHipError) as e:
        amap.pileup_fetch_qualities(0)
    assert e.value.code == N.DCN_ERR_ARG and "keeps no quality sums" in e.value.message
    amap.pileup_keep_qualities(False)  # (nothing to free)
    _, n_added = placer.pileup_batch(b, o, rows)
    bare = [amap.pileup_fetch(R).copy() for R in range(3)]
    with pytest.raises(dcn.DeaconHipError) as e:  # rule Q1: a row has added
        amap.pileup_keep_qualities()
    assert e.value.code == N.DCN_ERR_ARG and "%d rows have added" % n_added in e.value.message
    amap.pileup_reset()
    memory = amap.table_bytes
    amap.pileup_keep_qualities()  # fine after a reset
    assert amap.table_bytes == memory  # (dcn_index_memory does not count the sums)
    amap.pileup_keep_qualities()  # again: nothing changes
    assert amap.pileup_fetch_qualities(0).shape == (len(records[0]), 4) and not amap.pileup_fetch_qualities(0).any()
    assert amap.pileup_fetch_qualities(1, 5, 0).shape == (0, 4)
    with pytest.raises(dcn.DeaconHipError) as e:
        amap.pileup_fetch_qualities(0, len(records[0]), 1)
    assert e.value.code == N.DCN_ERR_ARG and "pileup fetch" in e.value.message
    # plain pileup_batch is refused while sums are kept, and names the call that is not
    with pytest.raises(dcn.DeaconHipError) as e:
        placer.pileup_batch(b, o, rows)
    assert e.value.code == N.DCN_ERR_ARG and "dcn_pileup_batch_qual" in e.value.message and "quality sums" in e.value.message
    assert all(not amap.pileup_fetch(R).any() for R in range(3))
    placer.pileup_batch(b, o, rows, quals=q, min_base_qual=0)
    assert all(np.array_equal(amap.pileup_fetch(R), bare[R]) for R in range(3))
    held = fetched(amap)
    assert sum(int(amap.pileup_fetch_qualities(R).sum()) for R in range(3)) > 10_000
    # the parameters and quals: checked behind dcn_pileup_batch's own, and nothing is touched
    vp = N.VerifyParams(1023, 200, rows.dtype.itemsize, 0)
    edits, added = np.zeros(len(rows), np.uint32), C.c_uint64(77)

    def call(qp, qptr, the_rows=rows):
        return L.dcn_pileup_batch_qual(placer._h, amap._h, b.ctypes.data, qptr, o.ctypes.data, len(o) - 1, C.byref(vp), qp, None,
                                       the_rows.ctypes.data, len(the_rows), edits.ctypes.data, C.byref(added))

    good = C.byref(N.PileupQualParams(33, 20, (C.c_uint32 * 2)(0, 0)))
    for qp, word in ((None, b"qual_params is NULL"), (C.byref(N.PileupQualParams(33, 20, (C.c_uint32 * 2)(0, 1))), b"qual_params.reserved"),
                     (C.byref(N.PileupQualParams(256, 20, (C.c_uint32 * 2)(0, 0))), b"qual_offset must be 0..255"),
                     (C.byref(N.PileupQualParams(33, 256, (C.c_uint32 * 2)(0, 0))), b"min_base_qual must be 0..255")):
        assert call(qp, q.ctypes.data) == N.DCN_ERR_ARG and word in L.dcn_last_error(), word
    assert call(good, None) == N.DCN_ERR_ARG and b"quals is NULL" in L.dcn_last_error()
    bad = rows.copy()
    bad["ref_end"][3] = 20_001
    assert call(None, None, bad) == N.DCN_ERR_ARG and b"row 3: ref_end 20001" in L.dcn_last_error()  # (the row's error comes first)
    assert added.value == 77 and fetched(amap) == held
    clone = amap.clone(0)  # an index without the sums
    out4 = (C.c_uint32 * 4)()
    assert L.dcn_anchor_map_pileup_fetch_qualities(clone._h, 0, 0, 1, out4) == N.DCN_ERR_ARG
    clone.close()
    # reset zeroes the sums too
    amap.pileup_reset()
    assert all(not amap.pileup_fetch_qualities(R).any() and not amap.pileup_fetch(R).any() for R in range(3))
    placer.pileup_batch(b, o, rows, quals=q, min_base_qual=0)
    assert fetched(amap) == held
    # keep = False frees the sums and leaves the counters: the plain call works again
    amap.pileup_keep_qualities(False)
    assert all(np.array_equal(amap.pileup_fetch(R), bare[R]) for R in range(3))
    with pytest.raises(dcn.DeaconHipError):
        amap.pileup_fetch_qualities(0)
    with pytest.raises(dcn.DeaconHipError):
        amap.pileup_keep_qualities()  # (rows have added)
    placer.pileup_batch(b, o, rows)
    assert all(np.array_equal(amap.pileup_fetch(R), 2 * bare[R]) for R in range(3))
    # disable frees them with the pileup; a new pileup has none
    amap.pileup_reset()
    amap.pileup_keep_qualities()
    amap.pileup_disable()
    amap.pileup_enable()
    with pytest.raises(dcn.DeaconHipError) as e:
        amap.pileup_fetch_qualities(0)
    assert "keeps no quality sums" in e.value.message
    placer.pileup_batch(b, o, rows)
    assert all(np.array_equal(amap.pileup_fetch(R), bare[R]) for R in range(3))
    placer.close()
    amap.close()


def test_align_beside_it(built, dcn):
    """dcn_align_batch is byte-identical before and after a quality call on the same context"""
    records, reads, quals, (b, o, q), maps = built
    amap, placer = maps[(31, 15)]
    po, srows, _ = placer.place_split_batch(b, o)
    want = AW.align_rows(reads, records, srows, row_offsets=po)
    amap.pileup_reset()
    first = placer.align_batch(b, o, srows, row_offsets=po)
    AW.assert_same(first, want, srows)
    placer.pileup_batch(b, o, srows, row_offsets=po, quals=q, min_base_qual=20)
    again = placer.align_batch(b, o, srows, row_offsets=po)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(first, again))

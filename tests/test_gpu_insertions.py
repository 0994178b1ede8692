"""The insertion ledger on the rows the placement calls return, against the model of tests/_insertion_worker.py (the runs of a
full table walked one at a time into a Python list: no buckets, no scans, no lanes): the reads of tests/test_gpu_align.py,
whose edited reads carry insertions, at (k, w) = (31, 15) and (31, 1), with the rows of place_batch, place_split_batch and
extend_batch.  How a batch is cut and ordered, select, reset, keep and its refusal, disable, clone, info, that the eight
counters and dcn_align_batch are what they are without a ledger, and the end-to-end case.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import _align_worker as AW
import _insertion_worker as IW
import _pileup_worker as PW
import _verify_worker as VW
from test_gpu_align import make_reads, make_records

pytestmark = pytest.mark.gpu

CASES = [(31, 15), (31, 1)]


@pytest.fixture(scope="module")
def built(dcn, oracle):
    records = make_records()
    reads = make_reads(records)
    out = {}
    for k, w in CASES:
        amap = VW.build_map(oracle, dcn, records, k, w)
        amap.pileup_enable()
        amap.pileup_keep_insertions()
        placer = dcn.Placer(amap, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
        out[(k, w)] = (amap, placer)
    yield records, reads, oracle.concat_reads(reads), out
    for amap, placer in out.values():
        placer.close()
        amap.close()


def fetched(amap, n_records=3):
    """the ledger as bytes: what two maps fed the same rows must agree on"""
    return [tuple(x.tobytes() if hasattr(x, "tobytes") else x for x in amap.insertions_fetch(R)) for R in range(n_records)]


@pytest.mark.parametrize("k,w", CASES)
def test_rows_of_the_placement_calls(built, dcn, k, w):
    records, reads, (b, o), maps = built
    amap, placer = maps[(k, w)]
    po, srows, _ = placer.place_split_batch(b, o, max_placements=4)
    xrows, _ = placer.extend_batch(b, o, srows, row_offsets=po)
    for rows, ro in ((placer.place_batch(b, o), None), (srows, po), (xrows, po)):
        amap.pileup_reset()
        assert amap.insertions_info() == (0, 0)
        edits, n_added = placer.pileup_batch(b, o, rows, row_offsets=ro)
        counts, ledger = PW.new_counts(records), IW.new_ledger(records)
        want_edits, want_added = IW.pile_rows(counts, ledger, reads, records, rows, row_offsets=ro)
        assert edits.tolist() == want_edits.tolist() and n_added == want_added > 60
        PW.assert_counts(amap, records, counts)
        total = IW.assert_ledger(amap, records, counts, ledger, settings=((3, 500), (1, 0)))
        assert total[0] >= 30 and total[1] >= total[0]
        assert any(e[4] for led in ledger for e in led) and any(not e[4] for led in ledger for e in led)  # both strands
        # a sub-range is the whole record's events cut to it
        for R, start, n in ((1, 2000, 2500), (0, 0, 1), (2, 19_999, 1), (1, 7, 0)):
            ev, bases = amap.insertions_fetch(R, start, n)
            assert IW.events_as_tuples(ev, bases) == IW.fetch_range(ledger[R], start, n)
            al, bases = amap.insertions_call(R, start, n, min_depth=1, min_permille=0)
            assert IW.alleles_as_tuples(al, bases) == IW.call_range(counts[R], ledger[R], records[R], start, n, 1, 0)
            assert amap.consensus(R, start, n, min_depth=1) == IW.consensus(counts[R], ledger[R], records[R], start, n, 1)


def test_cut_and_order_do_not_matter(built, dcn):
    """one batch = the same rows in three calls = the rows in reverse order (rule L3)"""
    records, reads, (b, o), maps = built
    amap, placer = maps[(31, 15)]
    po, srows, _ = placer.place_split_batch(b, o, max_placements=4)
    po = po.astype(np.int64)
    amap.pileup_reset()
    placer.pileup_batch(b, o, srows, row_offsets=po)
    whole, info = fetched(amap), amap.insertions_info()
    assert info[0] > 30
    amap.pileup_reset()
    for lo, hi in ((0, 17), (17, 18), (18, len(reads))):
        cb, co = dcn.concat_reads(reads[lo:hi])
        placer.pileup_batch(cb, co, srows[po[lo]:po[hi]], row_offsets=po[lo:hi + 1] - po[lo])
    assert fetched(amap) == whole and amap.insertions_info() == info
    rows = placer.place_batch(b, o)
    amap.pileup_reset()
    placer.pileup_batch(b, o, rows)
    forwards = fetched(amap)
    amap.pileup_reset()
    rb, ro = dcn.concat_reads(reads[::-1])
    placer.pileup_batch(rb, ro, rows[::-1].copy())
    assert fetched(amap) == forwards
    # select = leaving the rows out
    keep = np.random.default_rng(1711).random(len(rows)) < 0.6
    amap.pileup_reset()
    placer.pileup_batch(b, o, rows, select=keep)
    selected = fetched(amap)
    amap.pileup_reset()
    sb, so = dcn.concat_reads([r for r, k_ in zip(reads, keep) if k_])
    placer.pileup_batch(sb, so, rows[keep])
    assert fetched(amap) == selected != forwards


def test_keep_reset_disable_and_clone(built, dcn, oracle):
    records, reads, (b, o), maps = built
    N = dcn._native
    L = N.lib()
    amap = VW.build_map(oracle, dcn, records)
    placer = dcn.Placer(amap, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    rows = placer.place_batch(b, o)
    with pytest.raises(dcn.DeaconHipError) as e:
        amap.pileup_keep_insertions()
    assert e.value.code == N.DCN_ERR_ARG and "no pileup" in e.value.message
    amap.pileup_enable()
    for call in (amap.insertions_info, lambda: amap.insertions_fetch(0), lambda: amap.insertions_call(0)):
        with pytest.raises(dcn.DeaconHipError) as e:
            call()
        assert e.value.code == N.DCN_ERR_ARG and "keeps no insertion ledger" in e.value.message
    amap.pileup_keep_insertions(False)  # (nothing to drop)
    _, n_added = placer.pileup_batch(b, o, rows)
    bare = [amap.pileup_fetch(R).copy() for R in range(3)]
    with pytest.raises(dcn.DeaconHipError) as e:  # rule L1: a row has added
        amap.pileup_keep_insertions()
    assert e.value.code == N.DCN_ERR_ARG and "%d rows have added" % n_added in e.value.message
    amap.pileup_reset()
    amap.pileup_keep_insertions()  # fine after a reset
    amap.pileup_keep_insertions()  # again: nothing changes
    assert amap.insertions_info() == (0, 0) and len(amap.insertions_fetch(0)[0]) == 0 and amap.consensus(0, 0, 5) == b"NNNNN"
    placer.pileup_batch(b, o, rows)
    # the eight counters are what they are without a ledger
    assert all(np.array_equal(amap.pileup_fetch(R), bare[R]) for R in range(3))
    info, held = amap.insertions_info(), fetched(amap)
    assert info[0] == sum(int(x[:, PW.INS].sum()) for x in bare) > 20
    assert info[1] == sum(int(amap.insertions_fetch(R)[0]["len"].sum()) for R in range(3))
    with pytest.raises(dcn.DeaconHipError) as e:
        amap.add_records(records[:1])
    assert e.value.code == N.DCN_ERR_ARG and "pileup" in e.value.message
    clone = amap.clone(0)  # an index without the ledger
    n, m = C.c_uint64(), C.c_uint64()
    assert L.dcn_anchor_map_insertions_info(clone._h, C.byref(n), C.byref(m)) == N.DCN_ERR_ARG
    clone.close()
    assert fetched(amap) == held
    # keep = False leaves the counters; keeping again is refused until a reset, which empties both
    amap.pileup_keep_insertions(False)
    assert all(np.array_equal(amap.pileup_fetch(R), bare[R]) for R in range(3))
    with pytest.raises(dcn.DeaconHipError):
        amap.insertions_info()
    with pytest.raises(dcn.DeaconHipError):
        amap.pileup_keep_insertions()
    amap.pileup_reset()
    amap.pileup_keep_insertions()
    placer.pileup_batch(b, o, rows)
    assert fetched(amap) == held
    amap.pileup_reset()
    assert amap.insertions_info() == (0, 0)
    placer.pileup_batch(b, o, rows)
    assert fetched(amap) == held and amap.insertions_info() == info
    # disable frees the ledger with the pileup; a new pileup has none
    amap.pileup_disable()
    amap.pileup_enable()
    with pytest.raises(dcn.DeaconHipError) as e:
        amap.insertions_info()
    assert "keeps no insertion ledger" in e.value.message
    placer.close()
    amap.close()


def test_align_and_counters_beside_a_ledger(built, dcn, oracle):
    """dcn_align_batch is byte-identical on a map that keeps a ledger, and a refused call leaves counters and ledger alone"""
    records, reads, (b, o), maps = built
    amap, placer = maps[(31, 15)]
    po, srows, _ = placer.place_split_batch(b, o)
    want = AW.align_rows(reads, records, srows, row_offsets=po)
    amap.pileup_reset()
    first = placer.align_batch(b, o, srows, row_offsets=po)
    AW.assert_same(first, want, srows)
    placer.pileup_batch(b, o, srows, row_offsets=po)
    again = placer.align_batch(b, o, srows, row_offsets=po)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(first, again))
    held, counters = fetched(amap), [amap.pileup_fetch(R).copy() for R in range(3)]
    # a second map fed the same rows without a ledger: the eight counters are identical
    plain = VW.build_map(oracle, dcn, records)
    plain.pileup_enable()
    other = dcn.Placer(plain, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    assert other.pileup_batch(b, o, srows, row_offsets=po)[1] == int((first[0] < VW.OVER).sum())
    assert all(np.array_equal(plain.pileup_fetch(R), counters[R]) for R in range(3)) and any(x[:, PW.INS].any() for x in counters)
    other.close()
    plain.close()
    bad = srows.copy()
    bad["ref_end"][3] = 20_001
    with pytest.raises(dcn.DeaconHipError) as e:
        placer.pileup_batch(b, o, bad, row_offsets=po)
    assert e.value.code == dcn._native.DCN_ERR_ARG and "row 3: ref_end 20001" in e.value.message
    assert fetched(amap) == held and all(np.array_equal(amap.pileup_fetch(R), counters[R]) for R in range(3))


def test_end_to_end_reproduces_the_truth(dcn, oracle):
    """tests/test_insertions_abi.py's end-to-end case on the device: the consensus with fill from the reference is the truth"""
    record, truth, reads, rows = IW.truth_case()
    amap = VW.build_map(oracle, dcn, [record])
    amap.pileup_enable()
    amap.pileup_keep_insertions()
    placer = dcn.Placer(amap, max_batch_bases=1 << 16, max_batch_reads=1 << 10)
    b, o = oracle.concat_reads(reads)
    edits, n_added = placer.pileup_batch(b, o, IW.rows_as(dcn.filter.PLACEMENT_DTYPE, rows))
    assert n_added == len(reads)
    assert amap.consensus(0, fill_ref=True) == truth
    al, bases = amap.insertions_call(0)
    assert IW.alleles_as_tuples(al, bases)[0][:4] == (449, 0, 3, truth[448:451]) and len(al) == 1
    counts, ledger = PW.new_counts([record]), IW.new_ledger([record])
    IW.pile_rows(counts, ledger, reads, [record], rows)
    IW.assert_ledger(amap, [record], counts, ledger)
    placer.close()
    amap.close()

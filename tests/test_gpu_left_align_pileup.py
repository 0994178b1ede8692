"""A pileup whose rows are left-aligned first (dcn_anchor_map_pileup_left_align, rule N8): the counters, the quality sums and
both ledgers (fetch, insertion call, indel genotype) of a map with the switch on equal the model of
tests/_left_align_worker.py, which piles up the runs of rule N5; the same batch in 1, 2 and 7 calls gives the same map; the
switch is refused once a row has added and accepted again after a reset; and with the switch off the map is what
tests/_indel_worker.py's model of dcn_pileup_batch says, as before.  The rows are those of
tests/test_gpu_left_align_seams.py: homopolymers, tandem repeats and stretches over two letters, where gaps move.  Every
comparison is exact."""
import numpy as np
import pytest

import _indel_worker as DW
import _insertion_worker as IW
import _left_align_worker as LW
import _pileup_worker as PW
import _quality_worker as QW
import _verify_worker as VW
from test_gpu_left_align_seams import homopolymer_case, seam_records, two_letter_case

pytestmark = pytest.mark.gpu

LOOSE = dict(min_depth=1, min_gq=0, min_qual=0, min_count=1)
MIN_BASE_QUAL = 15


@pytest.fixture(scope="module")
def batch(dcn):
    """rows whose gaps move, with random qualities -> (records, reads, quals, rows)"""
    records = seam_records()
    a, b = homopolymer_case(dcn, records), two_letter_case(dcn, records, 2241, 90, 70, lambda q: 1 + q % 4)
    reads, rows = a.reads + b.reads, np.concatenate(a.rows + b.rows)
    return records, reads, QW.random_quals(np.random.default_rng(2242), reads, lo=5), rows


def new_map(dcn, oracle, records, left):
    amap = VW.build_map(oracle, dcn, records)
    amap.pileup_enable()
    amap.pileup_keep_insertions()
    amap.pileup_keep_deletions()
    amap.pileup_keep_qualities()
    if left:
        amap.pileup_left_align()
    return amap, dcn.Placer(amap, max_batch_bases=1 << 21, max_batch_reads=1 << 12)


def add(placer, oracle, reads, quals, rows, calls):
    cuts = np.linspace(0, len(reads), calls + 1).astype(int)
    edits, added = [], 0
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        b, o = oracle.concat_reads(reads[lo:hi])
        e, n = placer.pileup_batch(b, o, rows[lo:hi], max_permille=1000, quals=np.frombuffer(b"".join(quals[lo:hi]), np.uint8), min_base_qual=MIN_BASE_QUAL)
        edits += e.tolist()
        added += n
    return edits, added


@pytest.fixture(scope="module")
def truth(batch):
    records, reads, quals, rows = batch
    counts, sums, ins, dels = PW.new_counts(records), QW.new_sums(records), IW.new_ledger(records), DW.new_ledger(records)
    edits, n_added, info = LW.pile_rows(counts, ins, dels, reads, records, rows, max_permille=1000, quals=quals, min_base_qual=MIN_BASE_QUAL, sums=sums)
    assert info["rows_changed"] >= 120 and info["gaps_merged"] >= 3
    return counts, sums, ins, dels, edits, n_added, info


@pytest.mark.parametrize("calls", [1, 2, 7])
def test_counters_sums_and_ledgers_against_the_model(dcn, oracle, batch, truth, calls):
    records, reads, quals, rows = batch
    counts, sums, ins, dels, edits, n_added, info = truth
    amap, placer = new_map(dcn, oracle, records, left=True)
    got_edits, added = add(placer, oracle, reads, quals, rows, calls)
    assert got_edits == edits.tolist() and added == n_added
    assert amap.pileup_left_align_info() == info
    PW.assert_counts(amap, records, counts)
    QW.assert_sums(amap, records, sums)
    DW.assert_ledgers(amap, records, counts, ins, dels, settings=(DW.DEFAULTS, LOOSE))
    IW.assert_ledger(amap, records, counts, ins, settings=((3, 500), (1, 0)))  # fetch, the insertion call and the consensus
    placer.close()
    amap.close()


def test_the_switch_changes_only_on_an_empty_pileup(dcn, oracle, batch, truth):
    """rule N8: refused once a row has added, with a message that names the reset; accepted after it; the totals start again"""
    records, reads, quals, rows = batch
    counts, sums, ins, dels, edits, n_added, info = truth
    amap, placer = new_map(dcn, oracle, records, left=False)
    assert amap.pileup_left_align_info() == dict.fromkeys(LW.INFO_FIELDS, 0)
    add(placer, oracle, reads[:40], quals[:40], rows[:40], 1)
    assert amap.pileup_left_align_info() == dict.fromkeys(LW.INFO_FIELDS, 0)  # off: nothing is counted
    with pytest.raises(dcn.DeaconHipError) as e:
        amap.pileup_left_align()
    assert e.value.code == dcn._native.DCN_ERR_ARG and "rows have added to the pileup since it was enabled or reset" in str(e.value)
    assert "dcn_anchor_map_pileup_reset" in str(e.value)
    amap.pileup_left_align(False)  # (setting it to what it is always succeeds)
    amap.pileup_reset()
    amap.pileup_left_align()
    got_edits, added = add(placer, oracle, reads, quals, rows, 1)
    assert got_edits == edits.tolist() and added == n_added and amap.pileup_left_align_info() == info
    PW.assert_counts(amap, records, counts)
    with pytest.raises(dcn.DeaconHipError):
        amap.pileup_left_align(False)
    amap.pileup_reset()
    assert amap.pileup_left_align_info() == dict.fromkeys(LW.INFO_FIELDS, 0)
    amap.pileup_left_align(False)
    amap.pileup_disable()
    amap.pileup_enable()  # a new pileup begins with the switch off
    amap.pileup_keep_deletions()
    e2, _ = placer.pileup_batch(*oracle.concat_reads(reads[:40]), rows[:40], max_permille=1000)
    off = PW.new_counts(records)
    DW.pile_rows(off, IW.new_ledger(records), DW.new_ledger(records), reads[:40], records, rows[:40], max_permille=1000)
    PW.assert_counts(amap, records, off)
    placer.close()
    amap.close()


def test_with_the_switch_off_the_map_is_what_it_was(dcn, oracle, batch):
    """THIS TEST PASSES WITHOUT THE FEATURE: a map that never sets the switch against tests/_indel_worker.py's model of
    dcn_pileup_batch on rule A3's runs"""
    records, reads, quals, rows = batch
    amap = VW.build_map(oracle, dcn, records)
    amap.pileup_enable()
    amap.pileup_keep_insertions()
    amap.pileup_keep_deletions()
    amap.pileup_keep_qualities()
    placer = dcn.Placer(amap, max_batch_bases=1 << 21, max_batch_reads=1 << 12)
    got_edits, added = add(placer, oracle, reads, quals, rows, 2)
    counts, ins, dels = PW.new_counts(records), IW.new_ledger(records), DW.new_ledger(records)
    edits, n_added = DW.pile_rows(counts, ins, dels, reads, records, rows, max_permille=1000, quals=quals, min_base_qual=MIN_BASE_QUAL)
    assert got_edits == edits.tolist() and added == n_added
    PW.assert_counts(amap, records, counts)
    DW.assert_ledgers(amap, records, counts, ins, dels, settings=(DW.DEFAULTS, LOOSE))
    placer.close()
    amap.close()

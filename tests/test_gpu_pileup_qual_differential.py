"""The quality-aware pileup against the model of tests/_quality_worker.py on random rows: per seed the 300 rows of
tests/_insertion_worker.py's random_rows (three records, intervals of 0 .. 300 bases, edited by 0 - 25 %, N and lower case,
both strands) with qualities uniform in 0 .. 41, added in three unequal batches at threshold 20 on a map that keeps a ledger
and quality sums; counters, sums, ledger, calls and consensus at two settings are compared.  Every comparison is exact."""
import numpy as np
import pytest

import _insertion_worker as IW
import _pileup_worker as PW
import _quality_worker as QW
import _verify_worker as VW

pytestmark = pytest.mark.gpu

SEEDS = [1721, 1722]  # (tests/test_gpu_insertions_differential.py's: the same rows, now with qualities)
THRESHOLD = 20
BATCHES = ((0, 7), (7, 180), (180, 300))


@pytest.mark.parametrize("seed", SEEDS)
def test_random_rows(dcn, oracle, seed):
    records, reads, rows = IW.random_rows(seed, 300)
    quals = QW.random_quals(np.random.default_rng(seed + 100), reads, 0, 41)
    # the model alone, before the device is looked at: the inputs are not empty, and the threshold cuts through them
    counts, sums, ledger = PW.new_counts(records), QW.new_sums(records), IW.new_ledger(records)
    unmasked = PW.new_counts(records)
    aligned, want = 0, []
    for lo, hi in BATCHES:
        want.append(QW.pile_rows(counts, sums, ledger, reads[lo:hi], quals[lo:hi], records, rows[lo:hi], min_base_qual=THRESHOLD, max_permille=300))
        QW.pile_rows(unmasked, None, None, reads[lo:hi], quals[lo:hi], records, rows[lo:hi], min_base_qual=0, max_permille=300)
        aligned += int((want[-1][0] < VW.OVER).sum())
    base_steps = sum(int(c[:, :4].sum()) for c in unmasked)
    below = base_steps - sum(int(c[:, :4].sum()) for c in counts)
    assert below == sum(int(c[:, PW.N].sum()) for c in counts) - sum(int(c[:, PW.N].sum()) for c in unmasked)
    assert aligned >= 200, aligned
    assert 0.25 * base_steps <= below <= 0.75 * base_steps, (below, base_steps)  # (about 20 / 42 by construction)
    assert sum(int(s.sum()) for s in sums) > 20 * (base_steps - below) and sum(len(x) for x in ledger) >= 100

    amap = VW.build_map(oracle, dcn, records)
    amap.pileup_enable()
    amap.pileup_keep_insertions()
    amap.pileup_keep_qualities()
    placer = dcn.Placer(amap, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    drows = IW.rows_as(dcn.filter.PLACEMENT_DTYPE, rows)
    for (lo, hi), (want_edits, want_added) in zip(BATCHES, want):
        b, o, q = QW.concat(oracle, reads[lo:hi], quals[lo:hi])
        edits, n_added = placer.pileup_batch(b, o, drows[lo:hi], max_permille=300, quals=q, min_base_qual=THRESHOLD)
        assert edits.tolist() == want_edits.tolist() and n_added == want_added
    PW.assert_counts(amap, records, counts)
    QW.assert_sums(amap, records, sums)
    IW.assert_ledger(amap, records, counts, ledger, settings=((3, 500), (1, 200)))
    for R in range(len(records)):
        for min_depth, min_permille in ((3, 500), (1, 200)):
            PW.assert_calls(amap, records, counts, R, min_depth=min_depth, min_permille=min_permille)
    placer.close()
    amap.close()

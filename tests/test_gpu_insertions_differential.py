"""The insertion ledger against the model of tests/_insertion_worker.py on random rows: per seed 300 rows on three records,
intervals of 0 .. 300 bases, edited by 0 - 25 % with insertions favoured, N and lower case in reads and records, both
strands, added in three unequal batches; fetch, call at two settings and the consensus with and without fill are compared.
Every comparison is exact."""
import pytest

import _insertion_worker as IW
import _pileup_worker as PW
import _verify_worker as VW

pytestmark = pytest.mark.gpu

SEEDS = [1721, 1722]  # (picked so that the model meets the two counts asserted below; tests/_insertion_worker.py makes the rows)


@pytest.mark.parametrize("seed", SEEDS)
def test_random_rows(dcn, oracle, seed):
    records, reads, rows = IW.random_rows(seed)
    amap = VW.build_map(oracle, dcn, records)
    amap.pileup_enable()
    amap.pileup_keep_insertions()
    placer = dcn.Placer(amap, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    rows = IW.rows_as(dcn.filter.PLACEMENT_DTYPE, rows)
    counts, ledger = PW.new_counts(records), IW.new_ledger(records)
    aligned = 0
    for lo, hi in ((0, 7), (7, 180), (180, 300)):
        b, o = oracle.concat_reads(reads[lo:hi])
        edits, n_added = placer.pileup_batch(b, o, rows[lo:hi], max_permille=300)
        want_edits, want_added = IW.pile_rows(counts, ledger, reads[lo:hi], records, rows[lo:hi], max_permille=300)
        assert edits.tolist() == want_edits.tolist() and n_added == want_added
        aligned += int((want_edits < VW.OVER).sum())
    total = sum(len(x) for x in ledger)
    assert aligned >= 200 and total >= 100, (aligned, total)  # the inputs are not empty
    PW.assert_counts(amap, records, counts)
    IW.assert_ledger(amap, records, counts, ledger, settings=((3, 500), (1, 200)))
    assert any(e[1] for led in ledger for e in led) and any(b"N" in e[3] for led in ledger for e in led)
    placer.close()
    amap.close()

"""dcn_mark_duplicates_batch against the dict model of tests/_duplicates_worker.py on 20,000 random units per case: seeded
duplication rates of 0, 10 and 90 %, single and paired mode, with and without both_ends; split reads, unplaced rows in front
of placed ones, unplaced reads, reads without rows, clips on both strands and mates swapped.  The units go in as three
uneven calls, so that most duplicates of the later calls are of earlier ones.  Every comparison is exact."""
import numpy as np
import pytest

import _duplicates_worker as DW

pytestmark = pytest.mark.gpu

REC_LENS = [3_000_000, 1_000_000, 2_000_000]


@pytest.fixture(scope="module")
def amap(dcn, oracle):
    m = DW.make_map(oracle, dcn, False)
    m.duplicates_enable()
    yield m
    m.close()


@pytest.mark.parametrize("both_ends", [False, True], ids=["pos5", "both_ends"])
@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
@pytest.mark.parametrize("percent", [0, 10, 90])
def test_twenty_thousand_random_units(dcn, amap, percent, paired, both_ends):
    rng = np.random.default_rng(1000 + percent * 4 + paired * 2 + both_ends)
    per = 2 if paired else 1
    lengths, rows = DW.random_units(rng, 20000, percent / 100.0, REC_LENS, paired=paired)
    amap.duplicates_reset()
    model = DW.Model()
    dtype = DW.dtypes(dcn)[int(rng.integers(0, 3))]
    n_dup = 0
    for part_lengths, part_rows in DW.split(lengths, rows, [7001, 7300], per):
        dup, first = DW.check(dcn, amap, model, dtype, part_lengths, part_rows, paired, both_ends)
        n_dup += sum(dup)
    seen, keyed, keys = amap.duplicates_info()
    assert seen == 20000 and keyed - keys == n_dup
    # the model alone: the rate that was asked for is the rate that is there (a unit without a key is no duplicate)
    assert (n_dup < 60) if percent == 0 else (0.9 * percent / 100 < n_dup / 20000 < 1.1 * percent / 100), n_dup

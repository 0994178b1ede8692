"""dcn_align_batch against the model of tests/_align_worker.py on seeded random rows: 500 rows per seed in four groups of
125, each group one call with its own max_edits and max_permille.  Interval lengths 0 .. 300; substitutions, insertions
and deletions at 0 .. 25 %; both strands; N and lower case in the records; reads that own one to three rows (row_offsets)
or exactly one.  Every run equals the model's, and rule A4's sums hold (the model asserts them for every row it aligns)."""
import numpy as np
import pytest

import _align_worker as AW
import _verify_worker as VW
from conftest import random_reads, revcomp

pytestmark = pytest.mark.gpu

UNPLACED = VW.UNPLACED


@pytest.fixture(scope="module")
def env(dcn, oracle):
    records = random_reads(np.random.default_rng(1441), 3, 2500, 5000, p_n=0.002, p_lower=0.05)
    amap = VW.build_map(oracle, dcn, records, calls=[2, 1])
    placer = dcn.Placer(amap, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    yield records, amap, placer
    placer.close()
    amap.close()


@pytest.mark.parametrize("seed", [0, 1])
def test_random_rows(env, dcn, oracle, seed):
    records, _, placer = env
    rng = np.random.default_rng(1450 + seed)
    seen_d, seen_ops, aligned = set(), set(), 0
    for group in range(4):
        dtype = (dcn.filter.PLACEMENT_DTYPE, dcn.filter.SPLIT_PLACEMENT_DTYPE, dcn.filter.PAIR_PLACEMENT_DTYPE)[(seed + group) % 3]
        max_edits = (1023, 64, 5, 200)[(seed + group) % 4]
        max_permille = (250, 1000, 300, 100)[(3 * seed + group) % 4]
        csr = bool((seed + group) % 2)
        reads, rows, counts = [], [], []
        while len(rows) < 125:
            n_rows = int(rng.integers(1, 4)) if csr else 1
            n_rows = min(n_rows, 125 - len(rows))
            parts, at = [], 0
            for _ in range(n_rows):
                if rng.random() < 0.04:
                    rows.append(VW.make_row(dtype, UNPLACED, 0, 0, 0, 0, 0))
                    continue
                R = int(rng.integers(0, len(records)))
                n = int(rng.integers(0, 301))
                a = int(rng.integers(0, len(records[R]) - n + 1))
                S = VW.mutate_mixed(rng, records[R][a:a + n], float(rng.choice([0, 0.01, 0.05, 0.1, 0.2, 0.25])))[:300]
                if rng.random() < 0.1:
                    S = random_reads(rng, 1, 0, 300)[0]  # unrelated bases, any length against any
                if rng.random() < 0.1:
                    S = S.lower()
                rev = int(rng.integers(0, 2))
                gap = random_reads(rng, 1, 0, 40)[0]
                parts += [gap, revcomp(S) if rev else S]
                at += len(gap)
                rows.append(VW.make_row(dtype, R, rev, at, at + len(S), a, a + n))
                at += len(S)
            reads.append(b"".join(parts) + random_reads(rng, 1, 0, 10)[0])
            counts.append(n_rows)
        rows = np.concatenate(rows)
        ro = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64) if csr else None
        b, o = oracle.concat_reads(reads)
        got = placer.align_batch(b, o, rows, row_offsets=ro, max_edits=max_edits, max_permille=max_permille)
        want = AW.align_rows(reads, records, rows, row_offsets=ro, max_edits=max_edits, max_permille=max_permille)
        AW.assert_same(got, want, rows)
        seen_d |= set(want[0].tolist())
        seen_ops |= {int(x) & 15 for x in want[2]}
        aligned += int((want[0] < VW.OVER).sum())
    assert VW.OVER in seen_d and UNPLACED in seen_d and 0 in seen_d and len(seen_d) > 20 and aligned > 250
    assert seen_ops == {AW.OP_I, AW.OP_D, AW.OP_EQ, AW.OP_X}

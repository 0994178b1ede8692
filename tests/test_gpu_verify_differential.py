"""dcn_verify_batch against the model of tests/_verify_worker.py on seeded random rows: 2,000 rows per seed in four groups of
500, each group one call with its own max_edits and max_permille.  Interval lengths 0 .. 400, edit rates 0 .. 30 %, both
strands, N and lower case now and then, reads that own one to three rows (row_offsets) or exactly one (no row_offsets)."""
import numpy as np
import pytest

import _verify_worker as VW
from conftest import random_reads, revcomp

pytestmark = pytest.mark.gpu

UNPLACED = VW.UNPLACED


@pytest.fixture(scope="module")
def env(dcn, oracle):
    records = random_reads(np.random.default_rng(1331), 3, 2500, 5000, p_n=0.002, p_lower=0.05)
    amap = VW.build_map(oracle, dcn, records, calls=[2, 1])
    placer = dcn.Placer(amap, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    yield records, amap, placer
    placer.close()
    amap.close()


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_random_rows(env, dcn, oracle, seed):
    records, _, placer = env
    rng = np.random.default_rng(1340 + seed)
    dtype = (dcn.filter.PLACEMENT_DTYPE, dcn.filter.SPLIT_PLACEMENT_DTYPE, dcn.filter.PAIR_PLACEMENT_DTYPE)[seed % 3]
    seen = set()
    for group in range(4):
        max_edits = (1023, 3, 64, 0, 200, 20)[(seed + group) % 6]
        max_permille = (200, 1000, 20, 350, 0, 100)[(2 * seed + group) % 6]
        csr = bool((seed + group) % 2)
        reads, rows, counts = [], [], []
        while len(rows) < 500:
            n_rows = int(rng.integers(1, 4)) if csr else 1
            n_rows = min(n_rows, 500 - len(rows))
            parts, at = [], 0
            for _ in range(n_rows):
                if rng.random() < 0.04:
                    rows.append(VW.make_row(dtype, UNPLACED, 0, 0, 0, 0, 0))
                    continue
                R = int(rng.integers(0, len(records)))
                n = int(rng.integers(0, 401))
                a = int(rng.integers(0, len(records[R]) - n + 1))
                S = VW.mutate_mixed(rng, records[R][a:a + n], float(rng.choice([0, 0.01, 0.05, 0.1, 0.2, 0.3])))[:400]
                if rng.random() < 0.1:
                    S = random_reads(rng, 1, 0, 400)[0]  # unrelated bases, any length against any
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
        got = placer.verify_batch(b, o, rows, row_offsets=ro, max_edits=max_edits, max_permille=max_permille)
        want = VW.verify_rows(reads, records, rows, row_offsets=ro, max_edits=max_edits, max_permille=max_permille)
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (seed, group, max_edits, max_permille, [(int(i), int(got[i]), int(want[i]), rows[i]) for i in bad[:5]])
        seen |= set(np.minimum(want, 0xFFFFFFFD).tolist()) | {int(x) for x in want if x >= VW.OVER}
    assert VW.OVER in seen and UNPLACED in seen and 0 in seen and len(seen) > 10

"""dcn_pileup_batch and dcn_anchor_map_pileup_call against the model of tests/_pileup_worker.py on random rows: per seed
300 hand-placed rows on three records, intervals of 0 .. 300 bases, mixed edits at 0 - 25 %, N and lower case in reads and
records, both strands.  All eight columns are exact, and so are the calls and sites at two settings.  At least half of the
rows have an alignment under the default thresholds (asserted against the model's edits): a run that added nothing would
not pass."""
import numpy as np
import pytest

import _pileup_worker as PW
import _verify_worker as VW
from conftest import random_reads, revcomp

pytestmark = pytest.mark.gpu

OVER, UNPLACED = VW.OVER, VW.UNPLACED
LENGTHS = (1500, 777, 2049)


def make_records():
    rng = np.random.default_rng(1531)
    recs = [bytearray(random_reads(rng, 1, n, n)[0]) for n in LENGTHS]
    recs[1][300:304] = b"NNNN"
    recs[1][500:600] = bytes(recs[1][500:600]).lower()
    recs[2][2000:2002] = b"nR"
    return [bytes(r) for r in recs]


def make_rows(dtype, records, seed, n_rows=300):
    rng = np.random.default_rng(seed)
    reads, rows = [], []
    for q in range(n_rows):
        R = int(rng.integers(0, 3))
        ln = int(rng.integers(0, 301)) if q % 10 else (0, 1, 300)[q // 10 % 3]
        a = int(rng.integers(0, len(records[R]) - ln + 1))
        T = records[R][a:a + ln]
        S = VW.mutate_mixed(rng, T, float(rng.choice([0.0, 0.02, 0.05, 0.1, 0.15, 0.25])))
        if q % 7 == 0 and len(S) > 4:
            at = int(rng.integers(0, len(S)))
            S = S[:at] + b"N" + S[at + 1:]
        if q % 5 == 0:
            S = S.lower()
        rev, pre = int(rng.integers(0, 2)), int(rng.integers(0, 40))
        flank = random_reads(rng, 2, pre, pre)[0], random_reads(rng, 1, 0, 9)[0]
        reads.append(flank[0] + (revcomp(S) if rev else S) + flank[1])
        rows.append(VW.make_row(dtype, R, rev, pre, pre + len(S), a, a + ln))
    return reads, np.concatenate(rows)


@pytest.fixture(scope="module")
def env(dcn, oracle):
    records = make_records()
    amap = VW.build_map(oracle, dcn, records)
    amap.pileup_enable()
    placer = dcn.Placer(amap, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    yield dcn, oracle, records, amap, placer
    placer.close()
    amap.close()


@pytest.mark.parametrize("seed", [1532, 1533])
def test_random_rows(env, seed):
    dcn, O, records, amap, placer = env
    reads, rows = make_rows(dcn.filter.PLACEMENT_DTYPE, records, seed)
    counts = PW.new_counts(records)
    want_edits, want_added = PW.pile_rows(counts, reads, records, rows)
    aligned = int((want_edits < OVER).sum())
    assert 2 * aligned >= len(rows) and (want_edits == OVER).sum() >= 10, aligned  # at least half of the rows add
    assert (want_edits[want_edits < OVER] > 20).sum() >= 10                           # ... some of them with many edits
    total = sum(c.sum(axis=0) for c in counts)
    assert all(total[col] > 100 for col in (PW.A, PW.C, PW.G, PW.T, PW.DEL, PW.INS, PW.REV)) and total[PW.N] > 10
    amap.pileup_reset()
    b, o = O.concat_reads(reads)
    edits, n_added = placer.pileup_batch(b, o, rows)
    assert edits.tolist() == want_edits.tolist() and n_added == want_added
    PW.assert_counts(amap, records, counts)
    sites = {}
    for R in range(3):
        for kw in (dict(), dict(min_depth=1, min_permille=250)):
            _, _, info = PW.assert_calls(amap, records, counts, R, **kw)
            for x in info:
                sites[int(x) & 0xFF] = sites.get(int(x) & 0xFF, 0) + 1
    assert sum(sites.values()) > 50 and all(sites.get(f, 0) > 0 for f in (PW.SITE_SUB, PW.SITE_DEL, PW.SITE_INS)), sites

"""dcn_extend_batch against the model of tests/_extend_worker.py on random hand-placed rows: 2 seeds x 500 rows on three
records, flanks of 0 .. 300 bases with 0 - 25 % mixed edits and N, both strands, in groups that have their own penalty,
end_bonus and max_edits.  Every comparison is exact."""
import numpy as np
import pytest

import _extend_worker as XW
import _verify_worker as VW
from conftest import random_reads, revcomp

pytestmark = pytest.mark.gpu

GROUPS = [(6, 4, 1023), (2, 0, 1023), (3, 11, 1023), (9, 0, 5), (6, 4, 0), (4, 65535, 40), (255, 7, 1023), (2, 1, 1)]
N_ROWS = 500


@pytest.fixture(scope="module")
def env(dcn, oracle):
    rng = np.random.default_rng(1631)
    records = [bytearray(r) for r in random_reads(rng, 3, 700, 1100)]
    records[1][300:304] = b"NNNN"
    records[2][100:400] = bytes(records[2][100:400]).lower()
    records = [bytes(r) for r in records]
    amap = VW.build_map(oracle, dcn, records)
    placer = dcn.Placer(amap, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    yield records, amap, placer
    placer.close()
    amap.close()


def random_case(rng, records, dtype):
    reads, rows = [], []
    for _ in range(N_ROWS):
        R = int(rng.integers(0, 3))
        Lr = len(records[R])
        m = int(rng.integers(0, 60))
        fs = int(rng.integers(0, Lr - m + 1))
        if rng.random() < 0.1:
            fs = int(rng.integers(0, min(20, Lr - m + 1)))  # near base 0 of the record
        fe = fs + m
        rate = float(rng.choice([0.0, 0.02, 0.1, 0.25]))
        lo, hi = max(0, fs - int(rng.integers(0, 301))), min(Lr, fe + int(rng.integers(0, 301)))
        left, right = VW.mutate_mixed(rng, records[R][lo:fs], rate), VW.mutate_mixed(rng, records[R][fe:hi], rate)
        if rng.random() < 0.3:
            left = random_reads(rng, 2, 0, 15)[0] + left   # a stretch to clip
        if rng.random() < 0.3:
            right += random_reads(rng, 2, 0, 15)[1]
        if rng.random() < 0.2 and right:
            at = int(rng.integers(0, len(right)))
            right = right[:at] + b"N" + right[at + 1:]
        S = VW.mutate_mixed(rng, records[R][fs:fe], 0.05)
        oriented = left + S + right
        L, a, b = len(oriented), len(left), len(left) + len(S)
        rev = int(rng.integers(0, 2))
        reads.append(revcomp(oriented) if rev else oriented)
        rows.append(VW.make_row(dtype, R, rev, L - b if rev else a, L - a if rev else b, fs, fe))
        if rng.random() < 0.05:
            reads.append(random_reads(rng, 1, 0, 40)[0])
            rows.append(VW.make_row(dtype, XW.UNPLACED, 0, 0, 0, 0, 0))
    return reads, np.concatenate(rows)


@pytest.mark.parametrize("seed", (1, 2))
def test_random_rows_in_groups(env, dcn, oracle, seed):
    records, amap, placer = env
    rng = np.random.default_rng(1640 + seed)
    reads, rows = random_case(rng, records, dcn.filter.SPLIT_PLACEMENT_DTYPE if seed == 1 else dcn.filter.PLACEMENT_DTYPE)
    bounds = np.linspace(0, len(reads), len(GROUPS) + 1).astype(int)
    gained = edits = 0
    for (penalty, end_bonus, max_edits), lo, hi in zip(GROUPS, bounds[:-1], bounds[1:]):
        b, o = oracle.concat_reads(reads[lo:hi])
        kw = dict(penalty=penalty, end_bonus=end_bonus, max_edits=max_edits)
        got_rows, got = placer.extend_batch(b, o, rows[lo:hi], **kw)
        want_rows, want = XW.extend_rows(reads[lo:hi], records, rows[lo:hi], **kw)
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (kw, [(int(t), rows[lo + t], got[t], want[t]) for t in bad[:5]])
        assert got_rows.tobytes() == want_rows.tobytes()
        assert (want["left_edits"] <= max_edits).all() and (want["right_edits"] <= max_edits).all()
        gained += int((want["read_end"] - want["read_start"]).sum()) - int((rows["read_end"][lo:hi] - rows["read_start"][lo:hi]).sum())
        edits += int(want["left_edits"].sum()) + int(want["right_edits"].sum())
    assert gained > 20_000 and edits > 500

"""The counting index build (dcn_index_builder_*, IndexBuilder) against the oracle: an occurrence is a distinct
(sequence, position) pair of the index side's minimizer list, a key's count their number, saturating at 65,535.  The model
(tests/_index_builder_worker.py) takes positions, hashes, the ACGT test and the entropy floor from the oracle alone."""
import os
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

import _index_builder_worker as W
from _index_builder_worker import SAT, assert_counts, occurrences, selected
from conftest import random_reads, revcomp

pytestmark = pytest.mark.gpu

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_index_builder_worker.py")
IUPAC = b"ACGTNRYSWKMBDHVacgtnryswkmbdhv"
KW = [(31, 15), (15, 5)]


def _run_worker(case, **env):
    p = subprocess.run([sys.executable, WORKER, case], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, **env))
    assert p.returncode == 0, (case, env, p.stdout[-2000:], p.stderr[-4000:])
    return p.stdout


def messy_sequences(k, w):
    """IUPAC codes, N runs, lower case, low-complexity stretches, and the lengths around k and l = k + w - 1"""
    rng = np.random.default_rng(700 + k)
    l = k + w - 1
    alpha = np.frombuffer(IUPAC, dtype=np.uint8)
    seqs = []
    for i in range(24):
        ln = int(rng.integers(l, 3000))
        s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, ln)].copy()
        m = rng.random(ln) < 0.01
        s[m] = alpha[rng.integers(0, len(alpha), int(m.sum()))]
        if i % 3 == 0:
            s[rng.random(ln) < 0.5] |= 0x20
        if i % 4 == 0:
            at = int(rng.integers(0, ln - 20))
            s[at:at + 20] = ord("N")
        seqs.append(s.tobytes())
    base = random_reads(rng, 1, 400, 400)[0]
    seqs += [base[:k - 1], base[:k], base[:l - 1], base[:l], base, base, revcomp(base), b"", b"N" * 200,
             b"A" * 100 + base[:150] + b"AT" * 60 + b"ACG" * 40 + b"AAAAAAAAAAT" * 12, b"ACGTNNNNNACGT" * 30]
    return seqs


def test_pure_acgt_model_is_the_filter_side_list(oracle):
    """for pure-ACGT input at entropy 0 the model equals minimizer_hashes_and_positions directly"""
    rng = np.random.default_rng(701)
    seqs = random_reads(rng, 20, 10, 600)
    for k, w in KW:
        direct = Counter()
        for s in seqs:
            h, p = oracle.minimizer_hashes_and_positions(s, k, w)
            if len(p):
                direct.update(h[np.unique(p, return_index=True)[1]].tolist())
        assert direct == occurrences(oracle, seqs, k, w)


@pytest.mark.parametrize("thr", [0.0, 0.5])
@pytest.mark.parametrize("k,w", KW)
def test_parity_with_the_existing_build(oracle, dcn, k, w, thr):
    seqs = messy_sequences(k, w)
    model = occurrences(oracle, seqs, k, w, thr)
    want = sorted(oracle.Index.build(seqs, k=k, w=w, entropy_threshold=thr).keys().tolist())
    assert sorted(model) == want and len(want) > 100 and max(model.values()) >= 3
    if thr:
        assert len(want) < len(occurrences(oracle, seqs, k, w))
    b = dcn.IndexBuilder(k, w, entropy_threshold=thr)
    b.add(seqs)
    idx = b.finish(1, 0)
    assert idx.header() == (k, w, len(want))
    assert sorted(idx.keys().tolist()) == want
    assert sorted(dcn.Index.build(seqs, k, w, entropy_threshold=thr).keys().tolist()) == want
    assert_counts(b, model)
    assert b.info()["n_bases"] == sum(len(s) for s in seqs)


@pytest.fixture(scope="module")
def reads_case(oracle):
    rng = np.random.default_rng(702)
    genome = random_reads(rng, 1, 20_000, 20_000)[0]
    reads = []
    for i in range(2000):
        at = int(rng.integers(0, len(genome) - 150))
        r = genome[at:at + 150]
        reads.append(revcomp(r) if i % 2 else r)
    return reads, {kw: occurrences(oracle, reads, *kw) for kw in KW}


@pytest.mark.parametrize("k,w", KW)
def test_reads_in_three_calls_and_finish_by_count(oracle, dcn, reads_case, k, w):
    reads, models = reads_case
    model = models[(k, w)]
    b = dcn.IndexBuilder(k, w)
    for part in (reads[:700], reads[700:701], reads[701:]):
        b.add(part)
    assert_counts(b, model)
    assert max(model.values()) > 10 and min(model.values()) == 1
    for lo, hi in ((2, 0), (1, 1), (3, 10), (0, 0), (SAT, SAT)):
        want = selected(model, lo, hi)
        assert b.finish(lo, hi, count_only=True) == len(want), (lo, hi)
        idx = b.finish(lo, hi)
        assert idx.header() == (k, w, len(want)) and sorted(idx.keys().tolist()) == want, (lo, hi)
    assert selected(model, SAT, SAT) == []  # the empty selection above: a valid index with 0 keys
    assert 0 < len(selected(model, 3, 10)) < len(selected(model, 2, 0)) < len(model)
    # finish left the builder as it was: the same answer again, and add goes on counting
    assert sorted(b.finish(2, 0).keys().tolist()) == selected(model, 2, 0)
    assert_counts(b, model, bins=(256,))
    b.add(reads[:300])
    more = Counter(model)
    more.update(occurrences(oracle, reads[:300], k, w))
    assert_counts(b, more, bins=(256,))
    assert sorted(b.finish(2, 0).keys().tolist()) == selected(more, 2, 0)
    assert b.info()["n_bases"] == 150 * 2300


def test_split_invariance_and_piece_seams(oracle, dcn):
    W.case_seams(oracle, dcn)  # the default chunk: no sequence is cut
    out = _run_worker("seams", DCN_BUILD_CHUNK_BASES="4096")
    assert "seams chunk=4096" in out


def test_growth_carries_the_counters(oracle, dcn):
    W.case_growth(oracle, dcn)
    out = _run_worker("growth", DCN_TABLE_SLOTS_PER_KEY="2")
    assert "growth slots_per_key=2" in out


def test_saturation(oracle, dcn):
    k, w = 31, 15
    seq = b"A" * 70_000
    model = occurrences(oracle, [seq], k, w)
    (key, n), = model.items()
    assert n == 69_956 > SAT  # the oracle's count
    b = dcn.IndexBuilder(k, w)
    b.add([seq])
    keys, counts = b.counts()
    assert keys.tolist() == [key] and counts.tolist() == [SAT]
    assert b.info()["n_occurrences"] == n and b.info()["n_keys"] == 1
    assert b.finish(1, SAT).keys().tolist() == [key]
    assert b.finish(1, SAT - 1, count_only=True) == 0 and len(b.finish(1, SAT - 1)) == 0
    for nb in (2, 256, 4096):
        hist = b.hist(nb)
        assert hist[nb - 1] == 1 and int(hist.sum()) == 1
    b.add([seq[:1000]])  # a saturated counter stays; the occurrences are still counted
    assert b.counts()[1].tolist() == [SAT] and b.info()["n_occurrences"] == n + 1000 - 45 + 1

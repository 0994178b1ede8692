"""The model of tests/test_gpu_index_builder*.py and the worker of their subprocess cases.

Model, from the oracle alone: for every sequence, the positions canonical_minimizer_positions gives for the canonicalised
bytes, the hash of each from minimizer_hashes_and_positions of the canonicalised sequence, kept when the ORIGINAL k-mer is
all ACGT (either case) and its scaled_entropy meets the floor; the count of a key is the number of distinct
(sequence, position) pairs with its hash, saturating at 65,535.

As a program (python tests/_index_builder_worker.py seams|growth) it runs one case in a process of its own, whose
environment the test has set (DCN_BUILD_CHUNK_BASES, DCN_TABLE_SLOTS_PER_KEY), and exits non-zero with a traceback when a
check fails."""
import os
import sys
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
from conftest import random_reads, revcomp  # noqa: E402

SAT = 65535
ACGT = frozenset(b"ACGTacgt")
_canon = None


def canonicalise(O, seq):
    global _canon
    if _canon is None:
        _canon = bytes(O.canonicalise_nucleotide(c) for c in range(256))
    return bytes(seq).translate(_canon)


def positions_of(O, seq, k, w):
    """distinct index-side minimizer positions of one sequence, before the ACGT test and the entropy floor"""
    if len(seq) < max(k, k + w - 1):
        return np.zeros(0, np.uint32)
    return np.unique(O.canonical_minimizer_positions(canonicalise(O, seq), k, w))


def occurrences(O, seqs, k, w, thr=0.0):
    """Counter: hash -> distinct (sequence, position) pairs with that hash, over every sequence"""
    c = Counter()
    thr = np.float32(thr)
    for s in seqs:
        s = bytes(s)
        pos = positions_of(O, s, k, w)
        if not len(pos):
            continue
        h, p = O.minimizer_hashes_and_positions(canonicalise(O, s), k, w)
        hash_at = dict(zip(p.tolist(), h.tolist()))
        for q in pos.tolist():
            kmer = s[q:q + k]
            if not ACGT.issuperset(kmer):
                continue
            if thr > 0 and np.float32(O.scaled_entropy(kmer, k)) < thr:
                continue
            c[hash_at[q]] += 1
    return c


def assert_counts(b, model, bins=(2, 3, 256, 4096)):
    """counts(), hist() and info() of builder `b` equal the model"""
    want = {key: min(n, SAT) for key, n in model.items()}
    keys, counts = b.counts()
    assert keys.dtype == np.uint64 and counts.dtype == np.uint32 and len(keys) == len(counts)
    order = np.argsort(keys)
    wk = np.array(sorted(want), dtype=np.uint64)
    wc = np.array([want[key] for key in sorted(want)], dtype=np.uint32)
    assert np.array_equal(keys[order], wk), ("keys", len(keys), len(wk))
    assert np.array_equal(counts[order], wc), "counts"
    for nb in bins:
        hist = b.hist(nb)
        assert hist.dtype == np.uint64 and len(hist) == nb
        assert np.array_equal(hist, np.bincount(np.minimum(wc, nb - 1), minlength=nb).astype(np.uint64)), ("hist", nb)
        assert hist[0] == 0 and int(hist.sum()) == len(wk)
    info = b.info()
    assert info["n_keys"] == len(wk) == len(b)
    assert info["n_occurrences"] == sum(model.values())


def selected(model, lo, hi):
    """the keys finish(lo, hi) keeps"""
    lo, hi = max(lo, 1), hi or SAT
    return sorted(key for key, n in model.items() if lo <= min(n, SAT) <= hi)


def pieces_share_a_position(O, seq, k, w, chunk):
    """how many positions two consecutive pieces of `seq`, cut as the library cuts a sequence longer than a chunk (pieces
    of `chunk` bases, each starting l-1 bases before the cut), both report"""
    l, a, shared, last = k + w - 1, 0, 0, set()
    while a + l <= len(seq):
        piece = seq[a:a + chunk]
        cur = set((positions_of(O, piece, k, w) + a).tolist())
        shared += len(cur & last)
        last = cur
        if a + len(piece) >= len(seq):
            break
        a += len(piece) - (l - 1)
    return shared


def seam_sequences():
    rng = np.random.default_rng(711)
    unit, left, right = random_reads(rng, 1, 2000, 2000)[0], random_reads(rng, 1, 700, 700)[0], random_reads(rng, 1, 900, 900)[0]
    return [random_reads(rng, 1, 10_000, 10_000)[0], left + unit * 5 + right]


def case_seams(O, dcn, k=31, w=15):
    """two sequences longer than a chunk of 4,096 bases (when the environment says so): a position inside the l-1 bases two
    pieces share, counted by both, would show as a count too high"""
    seqs = seam_sequences()
    shared = sum(pieces_share_a_position(O, s, k, w, 4096) for s in seqs)
    assert shared >= 1, "no position is reported by two pieces: the case proves nothing"
    whole = occurrences(O, seqs, k, w)
    assert max(whole.values()) >= 5  # the repeated unit
    b = dcn.IndexBuilder(k, w)
    b.add(seqs)
    assert_counts(b, whole, bins=(256,))
    assert b.info()["n_bases"] == sum(len(s) for s in seqs)
    b2 = dcn.IndexBuilder(k, w)  # one sequence per call: the same counts
    for s in seqs:
        b2.add([s])
    assert_counts(b2, whole, bins=(256,))
    print(f"seams chunk={os.environ.get('DCN_BUILD_CHUNK_BASES', 'default')}: {len(whole)} keys, {shared} positions in two pieces")


def case_growth(O, dcn, k=31, w=15):
    """capacity_keys at its minimum and three adds of more than 1,200 new keys each: the table grows and every counter
    arrives at its key's new slot"""
    rng = np.random.default_rng(712)
    b = dcn.IndexBuilder(k, w, capacity_keys=1)
    model, done, bytes_after = Counter(), [], []
    for i in range(3):
        new = random_reads(rng, 1, 12_000, 12_000)[0]
        batch = [new] + done[:1] + [revcomp(new[2000:3000])]  # earlier keys again: their counts move and go on growing
        before = len(model)
        model.update(occurrences(O, batch, k, w))
        assert len(model) - before > 1200
        b.add(batch)
        done.append(new)
        assert_counts(b, model, bins=(16,))
        bytes_after.append(b.info()["device_bytes"])
    assert max(model.values()) >= 3
    # from the first add on the front end's bitmap is counted too: what grows between add 1 and add 3 is table + counters
    assert bytes_after[2] > bytes_after[0]
    idx = b.finish(2, 0)
    assert sorted(idx.keys().tolist()) == selected(model, 2, 0)
    print(f"growth slots_per_key={os.environ.get('DCN_TABLE_SLOTS_PER_KEY', 'default')}: {len(model)} keys, "
          f"{bytes_after[0]} -> {bytes_after[2]} bytes")


if __name__ == "__main__":
    import deacon_server_amd as dcn
    from oracle import oracle as O
    O.lib()
    {"seams": case_seams, "growth": case_growth}[sys.argv[1]](O, dcn)

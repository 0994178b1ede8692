"""The model of tests/test_gpu_depth*.py and the worker of their subprocess cases.

Model: the depth of key K is the number of (read, position) pairs whose minimizer hash is K, positions taken from
oracle.minimizer_hashes_and_positions(read, k, w, prefix_length), each position of a read once, kept when K is in the
set; counters saturate at 65,535.  Members are Python sets of each member's keys.

As a program (python tests/_depth_worker.py seams|saturation) it runs one case in a process of its own, whose environment
the test has set (DCN_TILE_WINDOWS, DCN_TABLE_SLOTS_PER_KEY), and exits non-zero with a traceback when a check fails."""
import os
import sys
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
from conftest import mutate, random_reads, revcomp  # noqa: E402

SAT = 65535
BINS = (2, 3, 256, 4096)


def occurrences(O, reads, k, w, prefix=0):
    """Counter: hash -> (read, distinct position) pairs with that hash, over every read"""
    c = Counter()
    for r in reads:
        h, p = O.minimizer_hashes_and_positions(r, k, w, prefix)
        if len(p):
            _, first = np.unique(p, return_index=True)
            c.update(h[first].tolist())
    return c


def expected(model, mkeys, member=None):
    """{key: depth} of the keys of member `member` (None: of any member) with depth > 0, saturated"""
    keys = set().union(*mkeys) if member is None else mkeys[member]
    return {key: min(d, SAT) for key, d in model.items() if d > 0 and key in keys}


def assert_depths(s, model, mkeys, bins=BINS):
    """depth_keys, depth_stats and depth_hist of set `s` equal the model, for any member and for each"""
    stats = s.depth_stats()
    assert sorted(stats) == ["observed", "saturated", "sum"]
    for name in stats:
        assert stats[name].dtype == np.uint64 and len(stats[name]) == s.n
    for member in [None] + list(range(s.n)):
        want = expected(model, mkeys, member)
        keys, depths = s.depth_keys(member)
        assert keys.dtype == np.uint64 and depths.dtype == np.uint32 and len(keys) == len(depths)
        order = np.argsort(keys)
        wk = np.array(sorted(want), dtype=np.uint64)
        wd = np.array([want[key] for key in sorted(want)], dtype=np.uint32)
        assert np.array_equal(keys[order], wk), ("keys", member, len(keys), len(wk))
        assert np.array_equal(depths[order], wd), ("depths", member)
        n_keys = len(set().union(*mkeys) if member is None else mkeys[member])
        for nb in bins:
            hist = s.depth_hist(member, nb)
            assert hist.dtype == np.uint64 and len(hist) == nb
            wh = np.bincount(np.minimum(wd, nb - 1), minlength=nb).astype(np.uint64)
            wh[0] = n_keys - len(wd)
            assert np.array_equal(hist, wh), ("hist", member, nb)
        if member is not None:
            assert int(stats["observed"][member]) == len(wd), ("observed", member)
            assert int(stats["sum"][member]) == int(wd.astype(np.uint64).sum()), ("sum", member)
            assert int(stats["saturated"][member]) == int((wd == SAT).sum()), ("saturated", member)


def sample(rng, genomes, n, lo, hi, p_n=0.002):
    """n reads of lo..hi bases: three quarters drawn from a genome (1 % substitutions, either strand), the rest random"""
    reads = []
    for _ in range(n):
        ln = int(rng.integers(lo, hi + 1))
        g = genomes[int(rng.integers(0, len(genomes)))]
        if rng.random() < 0.75 and ln < len(g):
            at = int(rng.integers(0, len(g) - ln))
            r = mutate(rng, g[at:at + ln], 0.01)
            if rng.random() < 0.5:
                r = revcomp(r)
        else:
            r = random_reads(rng, 1, ln, ln)[0]
        a = np.frombuffer(r, dtype=np.uint8).copy()
        a[rng.random(ln) < p_n] = ord("N")
        reads.append(a.tobytes())
    return reads


def make_genomes():
    return random_reads(np.random.default_rng(611), 3, 20_000, 20_000)


def member_seqs(genomes):
    g0, g1, g2 = genomes
    return [[g0, g1[:10_000]], [g1], [g2]]  # member 0 overlaps member 1; member 2 is disjoint from both


def mixed_batch(genomes):
    """about 600 reads of 60-250 bp, four of 3-9 kbp (units of more than 64 entries and more than 32 distinct hits: the
    workgroup kernel), and reads shorter than k, with N, in lower case, or empty"""
    rng = np.random.default_rng(612)
    reads = sample(rng, genomes, 600, 60, 250)
    for ln, g in ((3000, 0), (5200, 1), (9000, 2), (7001, 1)):
        at = int(rng.integers(0, len(genomes[g]) - ln))
        reads.append(mutate(rng, genomes[g][at:at + ln], 0.005))
    reads += [b"", b"ACGT", b"A" * 30, b"ACGTN" * 20, b"N" * 200, genomes[0][100:300].lower(),
              genomes[1][5000:5160].lower() + b"N" + genomes[1][5161:5300], genomes[2][40:70]]
    reads += random_reads(rng, 20, 80, 200, p_n=0.01, p_lower=0.3)
    order = rng.permutation(len(reads))
    return [reads[i] for i in order]


def build_members(O, dcn, genomes, k, w):
    """(key sets, device indexes) of the three members"""
    ol = [O.Index.build(seqs, k=k, w=w) for seqs in member_seqs(genomes)]
    return [set(o.keys().tolist()) for o in ol], [dcn.Index.from_keys(o.keys(), k, w) for o in ol]


def classify(O, clf, reads, uid=None):
    b, o = O.concat_reads(reads)
    return clf.classify_batch(b, o, uid)


# ---- subprocess cases ---------------------------------------------------------------------------------------------
def case_seams(O, dcn):
    """the mixed batch with tiles of 16 windows (every read of 31 bases or more is cut into several tiles, each seam a
    carry window), at w = 15 and at w = 1: an entry counted on both sides of a seam would show as a depth too high"""
    assert os.environ.get("DCN_TILE_WINDOWS") == "16"
    genomes = make_genomes()
    reads = mixed_batch(genomes)
    for w in (15, 1):
        mkeys, gl = build_members(O, dcn, genomes, 31, w)
        s = dcn.IndexSet(gl)
        s.enable_depth()
        clf = dcn.Classifier(s, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
        _, hits, total = classify(O, clf, reads)
        assert total.max() > 64 and hits.max() > 32
        model = occurrences(O, reads, 31, w)
        assert max(expected(model, mkeys).values()) > 1
        assert_depths(s, model, mkeys, bins=(256,))
        print(f"seams w={w}: {len(expected(model, mkeys))} keys observed, {int(total.sum())} entries")


def case_saturation(O, dcn):
    """eight hot keys driven to 65,534, to 65,535 and past it beside 950 keys hit once per batch, in a table
    of two slots per key (word neighbours of the hot slots are likely occupied): saturation, and no carry into the
    other half of a word"""
    assert os.environ.get("DCN_TABLE_SLOTS_PER_KEY") == "2"
    rng = np.random.default_rng(613)
    hot = random_reads(rng, 8, 31, 31)
    cold = random_reads(rng, 1, 980, 980)[0]
    ol = [O.Index.build(hot + [cold[:60]], k=31, w=1), O.Index.build([cold], k=31, w=1)]
    mkeys = [set(o.keys().tolist()) for o in ol]
    hot_keys = [int(O.minimizer_hashes_and_positions(r, 31, 1)[0][0]) for r in hot]
    assert len(set(hot_keys)) == 8 and len(mkeys[1]) == 950 and not set(hot_keys) & mkeys[1]
    s = dcn.IndexSet([dcn.Index.from_keys(o.keys(), 31, 1) for o in ol])
    assert s.n_keys == 958 and s.memory == 2048 * 12  # 1024 groups of two slots, nearly half of them occupied
    s.enable_depth()
    clf = dcn.Classifier(s, max_batch_bases=1 << 25, max_batch_reads=1 << 20)
    cold_model = occurrences(O, [cold], 31, 1)
    assert set(cold_model.values()) == {1}

    def send(n_hot, n_cold):
        ascii_ = np.concatenate([np.tile(np.frombuffer(b"".join(hot), np.uint8), n_hot)] +
                                [np.frombuffer(cold, np.uint8)] * n_cold)
        offsets = np.concatenate([np.arange(8 * n_hot, dtype=np.uint64) * 31,
                                  8 * n_hot * 31 + np.arange(n_cold + 1, dtype=np.uint64) * len(cold)])
        _, _, total = clf.classify_batch(ascii_, offsets)
        assert int(total.sum()) == 8 * n_hot + 950 * n_cold

    model = Counter()

    def step(n_hot, n_cold):
        send(n_hot, n_cold)
        for key in hot_keys:
            model[key] += n_hot
        for key in cold_model:
            model[key] += n_cold
        assert_depths(s, model, mkeys, bins=(2, 4096))
        got = dict(zip(*[a.tolist() for a in s.depth_keys()]))
        return [got[key] for key in hot_keys], s.depth_stats()

    depths, stats = step(65534, 1)  # 16 Mbase
    assert depths == [65534] * 8 and stats["saturated"].tolist() == [0, 0]
    depths, stats = step(1, 1)
    assert depths == [SAT] * 8 and stats["saturated"].tolist() == [8, 0]
    sums = stats["sum"].tolist()
    depths, stats = step(100, 0)
    assert depths == [SAT] * 8 and stats["saturated"].tolist() == [8, 0] and stats["sum"].tolist() == sums
    print("saturation: ok", sums)


if __name__ == "__main__":
    import deacon_server_amd as dcn
    from oracle import oracle as O
    O.lib()
    {"seams": case_seams, "saturation": case_saturation}[sys.argv[1]](O, dcn)

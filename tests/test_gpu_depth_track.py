"""Depth tracks (dcn_depth_track_batch, DepthTracker): per bin of every sequence of a batch, the minimizer positions that
start in it, how many are keys of the chosen members, how many of those were observed, and the sum and maximum of their
depth counters.  The model (tests/_depth_track_worker.py) is the statement of include/deacon_hip.h over
oracle.minimizer_hashes_and_positions, a {key: depth} dict and the members' key sets.  Integers only, no tolerance."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _depth_worker as W
from _depth_track_worker import BIN_BASES, Model, assert_track, track, tracked_reads
from _depth_worker import classify, occurrences

pytestmark = pytest.mark.gpu

K, WIN = 31, 15
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_depth_track_worker.py")
MASKS = (1, 2, 4, 7, 5)  # every member, all of them, and two of the three


@pytest.fixture(scope="module")
def genomes():
    return W.make_genomes()


@pytest.fixture(scope="module")
def members(oracle, dcn, genomes):
    return W.build_members(oracle, dcn, genomes, K, WIN)


@pytest.fixture(scope="module")
def batch(genomes):
    return W.mixed_batch(genomes)


@pytest.fixture(scope="module")
def reads(genomes, batch):
    return tracked_reads(genomes, batch)


@pytest.fixture(scope="module")
def classified(oracle, dcn, members, batch):
    """the set after one classify call over the mixed batch, and the depths the model gives it"""
    s = dcn.IndexSet(members[1])
    s.enable_depth()
    clf = dcn.Classifier(s, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    classify(oracle, clf, batch)
    clf.close()
    return s, occurrences(oracle, batch, K, WIN)


@pytest.fixture(scope="module")
def models(oracle, members, reads, classified):
    return {prefix: Model(oracle, reads, K, WIN, members[0], classified[1], prefix) for prefix in (0, 100)}


def _members_of(mask):
    return [j for j in range(3) if mask >> j & 1]


@pytest.mark.parametrize("bin_bases", BIN_BASES)
def test_mixed_batch_against_the_model(oracle, dcn, reads, classified, models, bin_bases):
    s, _ = classified
    assert any(len(r) == 0 for r in reads) and any(0 < len(r) < K for r in reads) and any(r.endswith(b"\n") for r in reads)
    assert any(r and set(r) == {ord("N")} for r in reads) and any(r != r.upper() for r in reads)
    keys = 0
    for mask in MASKS:
        want = models[0].bins(bin_bases, mask)
        got = track(dcn, s, reads, oracle, bin_bases=bin_bases, member=_members_of(mask))
        assert_track(got, want, (bin_bases, mask))
        keys += int(want[1]["n_keys"].sum())
        assert int(want[1]["max_depth"].max()) >= 4 and int(want[1]["n_observed"].sum()) < int(want[1]["n_keys"].sum())
    assert keys > 20_000
    # member=None is every member, an int one member
    assert_track(track(dcn, s, reads, oracle, bin_bases=bin_bases), models[0].bins(bin_bases, 7), (bin_bases, None))
    assert_track(track(dcn, s, reads, oracle, bin_bases=bin_bases, member=1), models[0].bins(bin_bases, 2), (bin_bases, 1))
    for cap in (1, 3):
        for prefix in (0, 100):
            for mask in (7, 2):
                want = models[prefix].bins(bin_bases, mask, cap)
                got = track(dcn, s, reads, oracle, bin_bases=bin_bases, member=_members_of(mask), depth_cap=cap, prefix_length=prefix)
                assert_track(got, want, (bin_bases, mask, cap, prefix))
                assert int(want[1]["max_depth"].max()) <= cap
                if prefix == 0 and mask == 7:
                    assert int(want[1]["max_depth"].max()) == cap
    want = models[100].bins(bin_bases, 7)
    assert_track(track(dcn, s, reads, oracle, bin_bases=bin_bases, prefix_length=100), want, (bin_bases, "prefix"))
    if bin_bases in (31, 32, 33):  # bins past the cut exist and are zero
        bo, w = want
        assert int(bo[1]) == -(-len(reads[0]) // bin_bases) and not w["n_positions"][4:int(bo[1])].any() and w["n_positions"][:3].any()


def test_track_of_sequences(oracle, dcn, genomes, classified, models):
    s, _ = classified
    t = dcn.DepthTracker(s, max_batch_bases=1 << 20, max_batch_reads=1 << 12)  # bin_bases defaults to 1000
    per_seq = t.track(list(genomes) + [b""])
    t.close()
    bo, want = models[0].bins(1000, 7)
    assert [len(x) for x in per_seq] == [20, 20, 20, 0]
    for r in range(3):
        for f in want:
            assert np.array_equal(per_seq[r][f].astype(np.int64), want[f][int(bo[r]):int(bo[r + 1])])


def test_the_counters_are_untouched(oracle, dcn, reads, classified):
    s, _ = classified

    def depth_keys():
        keys, depths = s.depth_keys()
        order = np.argsort(keys)
        return keys[order].tobytes(), depths[order].tobytes()

    before = depth_keys()
    stats = {name: v.tolist() for name, v in s.depth_stats().items()}
    t = dcn.DepthTracker(s, max_batch_bases=1 << 20, max_batch_reads=1 << 12, bin_bases=33)
    b, o = oracle.concat_reads(reads)
    first = t.track_batch(b, o)
    second = t.track_batch(b, o)
    t.set_profiling(True)
    third = t.track_batch(b, o)
    ms, n = t.profile()
    assert n == 1 and ms["distinct"] > 0 and ms["finish"] > 0
    t.close()
    for other in (second, third):
        assert first[0].tobytes() == other[0].tobytes() and first[1].tobytes() == other[1].tobytes()
    assert first[1]["n_observed"].sum() > 0
    assert depth_keys() == before and {name: v.tolist() for name, v in s.depth_stats().items()} == stats


def test_a_position_the_dump_repeats_counts_once(oracle, dcn):
    """the k = 41 search of test_gpu_depth.py: reads in which two windows chose the same k-mer with another between"""
    k, rng = 41, np.random.default_rng(614)
    reads, raw = [], 0
    for _ in range(4000):
        r = W.random_reads(rng, 1, 2000, 2000)[0]
        _, p = oracle.minimizer_hashes_and_positions(r, k, WIN)
        if len(p) != len(np.unique(p)):
            reads.append(r)
            raw += len(p)
            if len(reads) == 3:
                break
    assert len(reads) == 3, "no read with a repeated minimizer position found"
    o = oracle.Index.build(reads, k=k, w=WIN)
    mkeys = [set(o.keys().tolist())]
    s = dcn.IndexSet([dcn.Index.from_keys(o.keys(), k, WIN)])
    s.enable_depth()
    clf = dcn.Classifier(s, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    classify(oracle, clf, reads)
    classify(oracle, clf, reads)
    clf.close()
    depth = occurrences(oracle, reads, k, WIN)
    depth = {key: 2 * d for key, d in depth.items()}
    m = Model(oracle, reads, k, WIN, mkeys, depth)
    for B in (0, 100):
        want = m.bins(B, 1)
        assert_track(track(dcn, s, reads, oracle, bin_bases=B), want, (B,))
        assert int(want[1]["n_positions"].sum()) == int(want[1]["n_keys"].sum()) == len(m.pos) < raw
        assert int(want[1]["sum_depth"].sum()) == 2 * len(m.pos)  # (no k-mer occurs at two positions here)


def test_capacity(oracle, dcn, reads, classified, models):
    N, L = dcn._native, dcn._native.lib()
    s, _ = classified
    b, o = oracle.concat_reads(reads)
    n = len(reads)
    t = dcn.DepthTracker(s, max_batch_bases=1 << 20, max_batch_reads=1 << 12, bin_bases=1000)
    p = t._params()
    wbo, want = models[0].bins(1000, 7)
    need = int(wbo[-1])
    bp, op = b.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p)
    bins = np.zeros(need + 1, dcn.filter.TRACK_BIN_DTYPE)
    bins["n_positions"] = 0xABCD
    binp = bins.ctypes.data_as(C.c_void_p)
    for cap, ptr in ((0, None), (0, binp), (need - 1, binp)):
        bo = np.full(n + 1, 99, np.uint64)
        assert L.dcn_depth_track_batch(t._h, s._h, bp, op, n, C.byref(p), bo.ctypes.data_as(C.c_void_p), ptr, cap) == N.DCN_ERR_CAPACITY
        assert str(need).encode() in L.dcn_last_error()
        assert np.array_equal(bo.astype(np.int64), wbo) and (bins["n_positions"] == 0xABCD).all()
    bo = np.zeros(n + 1, np.uint64)
    assert L.dcn_depth_track_batch(t._h, s._h, bp, op, n, C.byref(p), bo.ctypes.data_as(C.c_void_p), binp, need) == 0
    assert bins["n_positions"][need] == 0xABCD
    assert_track((bo, bins[:need]), (wbo, want))
    t.close()


def test_argument_errors_on_a_real_set(oracle, dcn, members, reads, classified):
    N, L = dcn._native, dcn._native.lib()
    s, _ = classified
    b, o = oracle.concat_reads(reads[:5])
    bp, op = b.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p)
    bo = np.zeros(6, np.uint64)
    bop = bo.ctypes.data_as(C.c_void_p)
    bins = np.zeros(4096, dcn.filter.TRACK_BIN_DTYPE)
    binp = bins.ctypes.data_as(C.c_void_p)
    t = dcn.DepthTracker(s, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    plain = members[1][0]
    no_depth = dcn.IndexSet(members[1])

    def call(index, mask=7, **kw):
        p = N.TrackParams(1000, mask, kw.get("cap", 0), kw.get("reserved", 0), 0)
        return L.dcn_depth_track_batch(t._h, index._h, bp, op, 5, C.byref(p), bop, binp, 4096)

    for rc, word in ((lambda: call(plain), b"not a labelled set"), (lambda: call(no_depth), b"not enabled"),
                     (lambda: call(s, mask=8), b"member count"), (lambda: call(s, mask=0x80000001), b"member count"),
                     (lambda: call(s, mask=0), b"member_mask"), (lambda: call(s, cap=65536), b"depth_cap"),
                     (lambda: call(s, reserved=1), b"reserved")):
        assert rc() == N.DCN_ERR_ARG
        assert word in L.dcn_last_error()
    assert call(s, cap=65535) == 0 and call(s, mask=4) == 0
    with pytest.raises(dcn.DeaconHipError) as e:
        track(dcn, no_depth, reads[:5], oracle)
    assert e.value.code == N.DCN_ERR_ARG
    # a context of another k
    other = dcn.Index.from_keys(np.arange(1, 9, dtype=np.uint64), 21, 11)
    fp = dcn.FilterProcessor(other, max_batch_bases=1 << 16, max_batch_reads=1 << 8)
    p = N.TrackParams(1000, 7, 0, 0, 0)
    assert L.dcn_depth_track_batch(fp._h, s._h, bp, op, 5, C.byref(p), bop, binp, 4096) == N.DCN_ERR_ARG
    assert b"differ" in L.dcn_last_error()
    fp.close()
    t.close()


def test_tile_seams():
    p = subprocess.run([sys.executable, WORKER, "seams"], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, DCN_TILE_WINDOWS="16"))
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "track seams w=15" in p.stdout and "track seams w=1:" in p.stdout

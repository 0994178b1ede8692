"""Depth of a labelled index set (dcn_index_set_depth_*): after enable, every classify call against the set adds, per key
of the set, the (read, position) pairs whose minimizer hash is that key -- each position of a read once, after
prefix_length and the ACGT filter -- into a 16-bit counter that saturates at 65,535.  The model (tests/_depth_worker.py) is
a Python Counter over oracle.minimizer_hashes_and_positions."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _depth_worker as W
from _depth_worker import assert_depths, classify, expected, occurrences

pytestmark = pytest.mark.gpu

K, WIN = 31, 15
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_depth_worker.py")


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
def batch_model(oracle, batch):
    return occurrences(oracle, batch, K, WIN)


def new_set(dcn, members, depth=True):
    s = dcn.IndexSet(members[1])
    if depth:
        s.enable_depth()
    return s


def classifier(dcn, s, **kw):
    return dcn.Classifier(s, max_batch_bases=1 << 20, max_batch_reads=1 << 12, **kw)


def test_mixed_batch_is_exact(oracle, dcn, members, batch, batch_model):
    mkeys = members[0]
    s = new_set(dcn, members)
    assert_depths(s, {}, mkeys)  # nothing counted yet: every key in bin 0
    _, hits, total = classify(oracle, classifier(dcn, s), batch)
    assert (total > 64).sum() >= 4 and (hits.max(axis=1) > 32).any()  # units of the workgroup kernel
    assert ((total > 0) & (total <= 64)).any()                          # and of the lane kernel
    want = expected(batch_model, mkeys)
    assert len(want) > 3000 and max(want.values()) >= 4 and all(len(expected(batch_model, mkeys, j)) for j in range(3))
    assert_depths(s, batch_model, mkeys)


def _run_worker(case, **env):
    p = subprocess.run([sys.executable, WORKER, case], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, **env))
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout


def test_tile_seams_count_once():
    out = _run_worker("seams", DCN_TILE_WINDOWS="16")
    assert "seams w=15" in out and "seams w=1:" in out


def test_a_position_the_dump_repeats_counts_once(oracle, dcn):
    """Two windows of a read can choose the same k-mer with another window's choice between them: the dump (and total[u])
    holds that position twice, an occurrence is the position.  Reads with such a repeat are found by search."""
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
    _, _, total = classify(oracle, classifier(dcn, s), reads)
    model = occurrences(oracle, reads, k, WIN)
    assert int(total.sum()) == raw > sum(model.values())  # the totals count the repeats
    assert_depths(s, model, mkeys, bins=(256,))
    assert int(s.depth_stats()["sum"][0]) == sum(model.values())


def test_paired_units_and_prefix(oracle, dcn, members, batch):
    mkeys = members[0]
    uid = (np.arange(len(batch)) // 2).astype(np.uint32)
    s = new_set(dcn, members)
    _, _, total = classify(oracle, classifier(dcn, s, prefix_length=100), batch, uid)
    model = occurrences(oracle, batch, K, WIN, prefix=100)  # both mates count, each cut to its first 100 bases
    assert 0 < sum(model.values()) < sum(occurrences(oracle, batch, K, WIN).values())
    assert len(total) == (len(batch) + 1) // 2
    assert_depths(s, model, mkeys, bins=(256,))


def test_accumulation_and_lifecycle(oracle, dcn, genomes, members, batch, batch_model):
    mkeys = members[0]
    rng = np.random.default_rng(615)
    other = W.sample(rng, genomes, 300, 60, 250)
    other_model = occurrences(oracle, other, K, WIN)
    s = new_set(dcn, members)
    c1, c2 = classifier(dcn, s), classifier(dcn, s)
    classify(oracle, c1, batch)
    classify(oracle, c2, other)  # another context adds to the same counters
    assert_depths(s, batch_model + other_model, mkeys, bins=(256,))
    s.enable_depth()  # already on: the counts stay
    assert_depths(s, batch_model + other_model, mkeys, bins=(256,))
    classify(oracle, c2, other)
    assert_depths(s, batch_model + other_model + other_model, mkeys, bins=(256,))
    s.reset_depth()
    assert_depths(s, {}, mkeys, bins=(256,))
    classify(oracle, c1, other)
    assert_depths(s, other_model, mkeys, bins=(256,))
    s.enable_depth(False)
    classify(oracle, c1, batch)  # counted nowhere
    with pytest.raises(dcn.DeaconHipError):
        s.depth_stats()
    s.enable_depth()  # off then on: zero
    assert_depths(s, {}, mkeys, bins=(256,))
    classify(oracle, c2, batch)
    assert_depths(s, batch_model, mkeys, bins=(256,))


def test_saturation_and_contention():
    assert "saturation: ok" in _run_worker("saturation", DCN_TABLE_SLOTS_PER_KEY="2")


def test_outputs_unchanged_and_coverage_agrees(oracle, dcn, members, batch, batch_model):
    mkeys = members[0]
    uid = (np.arange(len(batch)) // 2).astype(np.uint32)
    s = new_set(dcn, members, depth=False)
    clf = classifier(dcn, s)
    plain = {}
    for name, u in (("reads", None), ("pairs", uid)):
        plain[name] = classify(oracle, clf, batch, u)
        s.enable_depth()
        on = classify(oracle, clf, batch, u)
        s.enable_depth(False)
        for a, b in zip(plain[name], on):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    s.enable_depth()
    s.enable_coverage()
    both = classify(oracle, clf, batch)
    for a, b in zip(plain["reads"], both):
        assert a.tobytes() == b.tobytes()
    observed, _ = s.coverage()
    assert observed.tolist() == s.depth_stats()["observed"].tolist()
    assert set(s.observed_keys().tolist()) == set(s.depth_keys()[0].tolist()) == set(expected(batch_model, mkeys))
    for j in range(3):
        assert set(s.observed_keys(j).tolist()) == set(s.depth_keys(j)[0].tolist())


def test_key_zero_is_in_bin_zero_only(oracle, dcn, members, batch, batch_model):
    """Key 0 as an unobserved key.  The other side -- a dump entry whose hash is 0 adding to key 0's own word, and the
    host folding that word into observed / sum / saturated / keys -- is covered by reading only: a read whose minimizer
    hashes to 0 means inverting the 64-bit hash, and no test builds one."""
    mkeys, gl = members
    keys0 = np.array(sorted(mkeys[0]) + [0], dtype=np.uint64)
    with_zero = dcn.Index.from_keys(keys0, K, WIN)
    mk = [mkeys[0] | {0}, mkeys[1], mkeys[2]]
    s = dcn.IndexSet([with_zero, gl[1], gl[2]])
    s.enable_depth()
    classify(oracle, classifier(dcn, s), batch)
    assert 0 not in batch_model  # no read yields hash 0: key 0 stays unobserved
    assert_depths(s, batch_model, mk)  # (hist[0] of member 0 and of "any" includes key 0: the model's key counts do)
    bare = new_set(dcn, members)
    classify(oracle, classifier(dcn, bare), batch)
    for member in (None, 0):
        assert int(s.depth_hist(member, 256)[0]) == int(bare.depth_hist(member, 256)[0]) + 1
    assert int(s.depth_hist(1, 256)[0]) == int(bare.depth_hist(1, 256)[0])
    assert s.depth_stats()["observed"].tolist() == bare.depth_stats()["observed"].tolist()
    assert 0 not in s.depth_keys()[0].tolist() and 0 not in s.depth_keys(0)[0].tolist()


def test_refused_device_batch_counts_nothing(oracle, dcn, members, batch, batch_model):
    torch = pytest.importorskip("torch")
    mkeys = members[0]
    b, o = oracle.concat_reads(batch)
    n = len(batch)
    s = new_set(dcn, members)
    clf = classifier(dcn, s)
    dev = torch.device("cuda:0")
    d_b = torch.from_numpy(b).to(dev)
    d_bad = torch.from_numpy(np.ascontiguousarray(o.view(np.int64)[::-1])).to(dev)
    d_m = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    clf.classify_batch_device(d_b.data_ptr(), d_bad.data_ptr(), n, len(b), d_m.data_ptr())
    with pytest.raises(dcn.DeaconHipError) as e:
        clf.synchronize()
    assert e.value.code == dcn._native.DCN_ERR_ARG
    assert_depths(s, {}, mkeys, bins=(256,))
    d_o = torch.from_numpy(o.view(np.int64)).to(dev)
    torch.cuda.synchronize()
    clf.classify_batch_device(d_b.data_ptr(), d_o.data_ptr(), n, len(b), d_m.data_ptr())  # the device form counts too
    clf.synchronize()
    assert_depths(s, batch_model, mkeys, bins=(256,))


def test_argument_errors_on_a_real_set(dcn, members):
    N, L = dcn._native, dcn._native.lib()
    s = new_set(dcn, members, depth=False)
    buf = (C.c_uint64 * 4096)()
    d32 = (C.c_uint32 * 16)()
    n = C.c_uint64(7)
    for call in (s.reset_depth, s.depth_stats, s.depth_hist, s.depth_keys):
        with pytest.raises(dcn.DeaconHipError) as e:
            call()
        assert e.value.code == N.DCN_ERR_ARG and "not enabled" in e.value.message
    s.enable_depth()
    for call, word in ((lambda: L.dcn_index_set_depth_stats(s._h, None, buf, buf), b"NULL"),
                       (lambda: L.dcn_index_set_depth_stats(s._h, buf, buf, None), b"NULL"),
                       (lambda: L.dcn_index_set_depth_hist(s._h, 0, 256, None), b"NULL"),
                       (lambda: L.dcn_index_set_depth_hist(s._h, 3, 256, buf), b"out of range"),
                       (lambda: L.dcn_index_set_depth_hist(s._h, 0, 1, buf), b"n_bins"),
                       (lambda: L.dcn_index_set_depth_hist(s._h, 0, 4097, buf), b"n_bins"),
                       (lambda: L.dcn_index_set_depth_keys(s._h, 0, buf, d32, 16, None), b"NULL"),
                       (lambda: L.dcn_index_set_depth_keys(s._h, 3, buf, d32, 16, C.byref(n)), b"out of range"),
                       (lambda: L.dcn_index_set_depth_keys(s._h, 0, None, d32, 16, C.byref(n)), b"NULL"),
                       (lambda: L.dcn_index_set_depth_keys(s._h, 0, buf, None, 16, C.byref(n)), b"NULL")):
        assert call() == N.DCN_ERR_ARG  # called one at a time: dcn_last_error holds the latest only
        assert word in L.dcn_last_error()
    plain = members[1][0]
    for call in (lambda: L.dcn_index_set_depth_enable(plain._h, 1), lambda: L.dcn_index_set_depth_reset(plain._h),
                 lambda: L.dcn_index_set_depth_stats(plain._h, buf, buf, buf),
                 lambda: L.dcn_index_set_depth_hist(plain._h, 0, 256, buf),
                 lambda: L.dcn_index_set_depth_keys(plain._h, 0, None, None, 0, C.byref(n))):
        assert call() == N.DCN_ERR_ARG
        assert b"not a labelled set" in L.dcn_last_error()
    # the counters are the set's alone: not in its reported memory, not in a clone
    table_bytes = C.c_uint64()
    N.check(L.dcn_index_set_info(s._h, None, None, None, None, C.byref(table_bytes)))
    assert table_bytes.value == s.memory
    h = C.c_void_p()
    N.check(L.dcn_index_clone(s._h, 0, C.byref(h)))
    try:
        assert L.dcn_index_set_depth_stats(h, buf, buf, buf) == N.DCN_ERR_ARG
    finally:
        L.dcn_index_destroy(h)


def test_capacity_is_reported_with_the_count(oracle, dcn, members, batch, batch_model):
    N, L = dcn._native, dcn._native.lib()
    s = new_set(dcn, members)
    classify(oracle, classifier(dcn, s), batch)
    want = len(expected(batch_model, members[0], 2))
    n = C.c_uint64()
    keys, depths = (C.c_uint64 * 8)(), (C.c_uint32 * 8)()
    assert L.dcn_index_set_depth_keys(s._h, 2, keys, depths, 8, C.byref(n)) == N.DCN_ERR_CAPACITY
    assert n.value == want > 8 and not any(keys) and not any(depths)

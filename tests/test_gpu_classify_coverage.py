"""Coverage of a labelled index set (dcn_index_set_coverage*): after enable, every classify call against the set marks
the set's keys among the minimizers its units counted.  The expected observed keys of member j are the oracle's minimizer
hashes (after prefix_length and the ACGT filter) of every read of every batch, intersected with member j's keys."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import mutate, random_reads
from test_gpu_classify import CLI, _fastq, _member_seqs, edge_reads, sample

pytestmark = pytest.mark.gpu

W = 15


@pytest.fixture(scope="module")
def genomes():
    rng = np.random.default_rng(171)
    return random_reads(rng, 3, 40_000, 40_000)


def _pairs(oracle, dcn, genomes, k, with_zero=True):
    """(oracle index, device index) per member: overlapping and disjoint genomes, plus (with_zero) a copy of member 0
    that also holds key 0"""
    out = []
    for seqs in _member_seqs(genomes):
        o = oracle.Index.build(seqs, k=k, w=W)
        out.append((o, dcn.Index.from_keys(o.keys(), k, W)))
    if with_zero:
        keys = np.concatenate([out[0][0].keys(), np.array([0], np.uint64)])
        out.append((oracle.Index(keys, k, W), dcn.Index.from_keys(keys, k, W)))
    return out


@pytest.fixture(scope="module")
def members31(oracle, dcn, genomes):
    return _pairs(oracle, dcn, genomes, 31)


@pytest.fixture(scope="module")
def members41(oracle, dcn, genomes):
    return _pairs(oracle, dcn, genomes, 41)


def observed_hashes(oracle, reads, k, prefix=0):
    out = set()
    for r in reads:
        h, _ = oracle.minimizer_hashes_and_positions(r, k, W, prefix)
        out.update(h.tolist())
    return out


def member_keys(ol):
    return [set(o.keys().tolist()) for o in ol]


def assert_observed(s, seen, mkeys):
    """every member's observed keys, the union's, and coverage() equal the expected sets"""
    observed, keys = s.coverage()
    assert observed.dtype == np.uint64 and keys.dtype == np.uint64 and len(observed) == s.n
    assert keys.tolist() == [len(m) for m in mkeys]
    want_any = set()
    for j, m in enumerate(mkeys):
        want = seen & m
        want.discard(0)  # no read yields hash 0 here; the check below pins that the key-0 mark stays clear
        got = s.observed_keys(j)
        assert got.dtype == np.uint64
        assert sorted(got.tolist()) == sorted(want), j
        assert int(observed[j]) == len(want), j
        want_any |= want
    got = s.observed_keys()
    assert sorted(got.tolist()) == sorted(want_any)
    assert 0 not in got.tolist()


def classify(oracle, clf, reads, uid=None):
    b, o = oracle.concat_reads(reads)
    return clf.classify_batch(b, o, uid)


def test_enable_reports_member_keys_and_errors(oracle, dcn, members31):
    N = dcn._native
    ol = [o for o, _ in members31]
    s = dcn.IndexSet([g for _, g in members31])
    for call in (s.coverage, s.reset_coverage, s.observed_keys):
        with pytest.raises(dcn.DeaconHipError) as e:
            call()
        assert e.value.code == N.DCN_ERR_ARG and "not enabled" in e.value.message
    s.enable_coverage()
    observed, keys = s.coverage()
    assert keys.tolist() == [len(o) for o in ol]  # member 3 holds key 0: counted among its keys
    assert keys[3] == keys[0] + 1
    assert not observed.any()
    assert len(s.observed_keys()) == 0
    L = N.lib()
    table_bytes, mem = C.c_uint64(), C.c_uint64()
    N.check(L.dcn_index_set_info(s._h, None, None, None, None, C.byref(table_bytes)))
    N.check(L.dcn_index_memory(s._h, C.byref(mem)))
    assert table_bytes.value == s.memory and mem.value < s.memory  # the bitmap is counted by neither
    with pytest.raises(dcn.DeaconHipError) as e:
        s.observed_keys(4)
    assert e.value.code == N.DCN_ERR_ARG and "out of range" in e.value.message
    n = C.c_uint64()
    obs = np.zeros(4, np.uint64)
    assert L.dcn_index_set_coverage(s._h, None, obs.ctypes.data_as(C.c_void_p)) == N.DCN_ERR_ARG
    assert L.dcn_index_set_coverage(s._h, obs.ctypes.data_as(C.c_void_p), None) == N.DCN_ERR_ARG
    assert b"NULL" in L.dcn_last_error()
    assert L.dcn_index_set_coverage_keys(s._h, 0, None, 0, None) == N.DCN_ERR_ARG
    assert L.dcn_index_set_coverage_keys(s._h, 0, None, 5, C.byref(n)) == N.DCN_ERR_ARG
    assert b"NULL" in L.dcn_last_error()
    # a plain index is not a set; a clone of the set is a plain index without coverage
    plain = members31[0][1]
    for rc in (L.dcn_index_set_coverage_enable(plain._h, 1), L.dcn_index_set_coverage_reset(plain._h),
               L.dcn_index_set_coverage(plain._h, obs.ctypes.data_as(C.c_void_p), obs.ctypes.data_as(C.c_void_p)),
               L.dcn_index_set_coverage_keys(plain._h, 0, None, 0, C.byref(n))):
        assert rc == N.DCN_ERR_ARG
        assert b"not a labelled set" in L.dcn_last_error()
    h = C.c_void_p()
    N.check(L.dcn_index_clone(s._h, 0, C.byref(h)))
    try:
        assert L.dcn_index_set_coverage(h, obs.ctypes.data_as(C.c_void_p), obs.ctypes.data_as(C.c_void_p)) == N.DCN_ERR_ARG
    finally:
        L.dcn_index_destroy(h)
    s.enable_coverage(False)
    with pytest.raises(dcn.DeaconHipError):
        s.coverage()


@pytest.mark.parametrize("k", [31, 41])
@pytest.mark.parametrize("paired,prefix", [(False, 0), (True, 0), (False, 60), (True, 60)])
def test_observed_keys_are_exact(oracle, dcn, genomes, members31, members41, k, paired, prefix):
    members = members31 if k == 31 else members41
    ol = [o for o, _ in members]
    rng = np.random.default_rng(k * 10 + prefix + paired)
    reads = sample(rng, genomes, 1500, 60, 200) + edge_reads() + [b"ACGT"]
    uid = (np.arange(len(reads)) // 2).astype(np.uint32) if paired else None
    s = dcn.IndexSet([g for _, g in members])
    s.enable_coverage()
    clf = dcn.Classifier(s, prefix_length=prefix, max_batch_bases=1 << 21, max_batch_reads=1 << 13)
    _, _, total = classify(oracle, clf, reads, uid)
    seen = observed_hashes(oracle, reads, k, prefix)
    b, o = oracle.concat_reads(reads)
    assert total.tolist() == oracle.filter_batch(ol[0], b, o, uid, prefix_length=prefix, threads=4)[2].tolist()
    assert_observed(s, seen, member_keys(ol))
    assert all(len(seen & m) for m in member_keys(ol)[:3])


def test_long_units_and_the_workgroup_path(oracle, dcn, genomes, members31, monkeypatch):
    ol = [o for o, _ in members31]
    rng = np.random.default_rng(8)
    # units of more than 64 entries and more than 32 distinct hits (the workgroup kernel, and the lane kernel's hand-off
    # of a unit whose hits overflow its list), a whole genome (several hash partitions), short ones around them
    long_reads = sample(rng, genomes, 40, 500, 4000, p_n=0.0005)
    mid_reads = sample(rng, genomes, 200, 300, 480, p_n=0.0)  # up to 64 entries, often more than 32 distinct hits
    reads = sample(rng, genomes, 300, 80, 160) + mid_reads + long_reads + [mutate(rng, genomes[1], 0.002)]
    rng.shuffle(reads)
    seen = observed_hashes(oracle, reads, 31)
    for tw in ("16", "100"):
        monkeypatch.setenv("DCN_TILE_WINDOWS", tw)
        s = dcn.IndexSet([g for _, g in members31])
        s.enable_coverage()
        clf = dcn.Classifier(s, max_batch_bases=1 << 22, max_batch_reads=1 << 12)
        _, hits, total = classify(oracle, clf, reads)
        assert total.max() > 5000 and (hits.max(axis=1) > 32).any()
        assert ((total <= 64) & (hits.max(axis=1) > 32)).any()  # a unit the lane kernel hands off
        assert_observed(s, seen, member_keys(ol))
        s.reset_coverage()
        classify(oracle, clf, reads, (np.arange(len(reads)) // 2).astype(np.uint32))
        assert_observed(s, seen, member_keys(ol))


def test_outputs_unchanged_by_coverage(oracle, dcn, genomes, members31, monkeypatch):
    monkeypatch.setenv("DCN_TILE_WINDOWS", "100")
    rng = np.random.default_rng(12)
    reads = sample(rng, genomes, 1500, 60, 200) + sample(rng, genomes, 20, 1000, 5000) + edge_reads()
    uid = (np.arange(len(reads)) // 2).astype(np.uint32)
    s = dcn.IndexSet([g for _, g in members31])
    clf = dcn.Classifier(s, max_batch_bases=1 << 22, max_batch_reads=1 << 13)
    for u in (None, uid):
        off = classify(oracle, clf, reads, u)
        s.enable_coverage()
        on = classify(oracle, clf, reads, u)
        s.enable_coverage(False)
        for a, b in zip(off, on):
            assert a.tolist() == b.tolist()


def test_thirty_two_members_mark_member_31(oracle, dcn, genomes, members31):
    rng = np.random.default_rng(7)
    reads = sample(rng, genomes, 800, 80, 300)
    s = dcn.IndexSet([members31[j % 3][1] for j in range(32)])
    s.enable_coverage()
    clf = dcn.Classifier(s, max_batch_bases=1 << 21, max_batch_reads=1 << 13)
    classify(oracle, clf, reads)
    seen = observed_hashes(oracle, reads, 31)
    mkeys = member_keys([members31[j % 3][0] for j in range(32)])
    observed, keys = s.coverage()
    want31 = seen & mkeys[31]  # member 31 is members31[1]
    assert want31 and int(observed[31]) == len(want31) and int(keys[31]) == len(mkeys[31])
    assert sorted(s.observed_keys(31).tolist()) == sorted(want31)
    assert observed.tolist() == [len(seen & m) for m in mkeys]


def test_marks_accumulate_reset_and_reenable(oracle, dcn, genomes, members31):
    ol = [o for o, _ in members31]
    mkeys = member_keys(ol)
    rng = np.random.default_rng(13)
    b1, b2, b3 = (sample(rng, genomes, 600, 80, 200) for _ in range(3))
    s = dcn.IndexSet([g for _, g in members31])
    s.enable_coverage()
    c1 = dcn.Classifier(s, max_batch_bases=1 << 21, max_batch_reads=1 << 13)
    c2 = dcn.Classifier(s, max_batch_bases=1 << 21, max_batch_reads=1 << 13)
    classify(oracle, c1, b1)
    assert_observed(s, observed_hashes(oracle, b1, 31), mkeys)
    classify(oracle, c1, b2)
    classify(oracle, c2, b3)
    assert_observed(s, observed_hashes(oracle, b1 + b2 + b3, 31), mkeys)
    s.enable_coverage()  # already on: the marks stay
    assert_observed(s, observed_hashes(oracle, b1 + b2 + b3, 31), mkeys)
    s.reset_coverage()
    assert not s.coverage()[0].any() and len(s.observed_keys()) == 0
    classify(oracle, c2, b2)
    assert_observed(s, observed_hashes(oracle, b2, 31), mkeys)
    s.enable_coverage(False)
    classify(oracle, c1, b3)  # not marked anywhere
    s.enable_coverage()
    assert not s.coverage()[0].any()
    classify(oracle, c1, b1)
    assert_observed(s, observed_hashes(oracle, b1, 31), mkeys)


def test_device_form(oracle, dcn, genomes, members31):
    torch = pytest.importorskip("torch")
    ol = [o for o, _ in members31]
    rng = np.random.default_rng(11)
    reads = sample(rng, genomes, 2000, 100, 151) + sample(rng, genomes, 10, 2000, 5000)
    b, o = oracle.concat_reads(reads)
    uid = (np.arange(len(reads)) // 2).astype(np.uint32)
    n_units = int(uid[-1]) + 1
    s = dcn.IndexSet([g for _, g in members31])
    s.enable_coverage()
    clf = dcn.Classifier(s, prefix_length=100, max_batch_bases=1 << 22, max_batch_reads=1 << 13)
    dev = torch.device("cuda:0")
    d_b = torch.from_numpy(b).to(dev)
    d_o = torch.from_numpy(o.view(np.int64)).to(dev)
    d_u = torch.from_numpy(uid.view(np.int32)).to(dev)
    d_m = torch.zeros(n_units, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    clf.classify_batch_device(d_b.data_ptr(), d_o.data_ptr(), len(reads), len(b), d_m.data_ptr(),
                              d_unit_id=d_u.data_ptr(), n_units=n_units)
    clf.synchronize()
    assert_observed(s, observed_hashes(oracle, reads, 31, 100), member_keys(ol))


def test_refused_device_batch_marks_nothing(oracle, dcn, genomes, members31):
    torch = pytest.importorskip("torch")
    ol = [o for o, _ in members31]
    rng = np.random.default_rng(24)
    reads = sample(rng, genomes, 1500, 100, 200)
    b, o = oracle.concat_reads(reads)
    n = len(reads)
    s = dcn.IndexSet([g for _, g in members31])
    s.enable_coverage()
    clf = dcn.Classifier(s, max_batch_bases=1 << 20, max_batch_reads=4096)
    dev = torch.device("cuda:0")
    d_b = torch.from_numpy(b).to(dev)
    d_bad = torch.from_numpy(np.ascontiguousarray(o.view(np.int64)[::-1])).to(dev)
    d_m = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    clf.classify_batch_device(d_b.data_ptr(), d_bad.data_ptr(), n, len(b), d_m.data_ptr())
    with pytest.raises(dcn.DeaconHipError) as e:
        clf.synchronize()
    assert e.value.code == dcn._native.DCN_ERR_ARG
    assert not s.coverage()[0].any() and len(s.observed_keys()) == 0
    classify(oracle, clf, reads)
    assert_observed(s, observed_hashes(oracle, reads, 31), member_keys(ol))


def test_cli_classify_coverage(oracle, genomes, tmp_path):
    paths = []
    for j, seqs in enumerate(_member_seqs(genomes)):
        fa, out = tmp_path / f"m{j}.fa", tmp_path / f"m{j}.idx"
        fa.write_text("".join(f">s{i}\n{s.decode()}\n" for i, s in enumerate(seqs)))
        subprocess.run([CLI, "index", "build", str(fa), "-o", str(out), "-q"], check=True, capture_output=True, timeout=300)
        paths.append(str(out))
    rng = np.random.default_rng(31)
    reads = sample(rng, genomes, 2000, 80, 300) + sample(rng, genomes, 4, 20_000, 30_000)
    fq = tmp_path / "r.fq"
    _fastq(fq, [f"r{i}" for i in range(len(reads))], reads)
    x = [a for p in paths for a in ("-x", p)]
    mkeys = [set(oracle.Index.read(p).keys().tolist()) for p in paths]
    seen = observed_hashes(oracle, reads, 31)
    env = dict(os.environ, DCN_CLI_CLASSIFY_BATCH_BASES="10000")  # many batches, and contexts recreated for long records
    summ = tmp_path / "cov.json"
    p = subprocess.run([CLI, "classify", *x, str(fq), "-s", str(summ), "--coverage"], capture_output=True, text=True,
                       timeout=300, env=env, check=True)
    js = json.load(open(summ))
    for j, entry in enumerate(js["indexes"]):
        want = len(seen & mkeys[j])
        assert entry["keys"] == len(mkeys[j])
        assert entry["keys_observed"] == want, j
        assert entry["keys_observed_proportion"] == pytest.approx(want / len(mkeys[j]))
        assert f"m{j}: {want}/{len(mkeys[j])} (" in p.stderr and "index minimizers observed" in p.stderr
    plain = tmp_path / "plain.json"
    p = subprocess.run([CLI, "classify", *x, str(fq), "-s", str(plain)], capture_output=True, text=True, timeout=300,
                       env=env, check=True)
    for entry in json.load(open(plain))["indexes"]:
        assert "keys_observed" not in entry and "keys_observed_proportion" not in entry
    assert "observed" not in p.stderr
    q = subprocess.run([CLI, "classify", *x, str(fq), "--coverage", "-q"], capture_output=True, text=True, timeout=300,
                       env=env, check=True)
    assert "observed" not in q.stderr

"""Labelled index sets and per-member classification (dcn_index_set_create / dcn_classify_batch*) against the CPU oracle:
for every member j, hits[:, j], total and match bit j are what a counting filter run against member j alone gives."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, mutate, random_reads, revcomp

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "deacon-server_amd", "bin", "deacon-hip")


@pytest.fixture(scope="module")
def genomes():
    rng = np.random.default_rng(71)
    return random_reads(rng, 3, 60_000, 60_000)


def _member_seqs(genomes):
    g0, g1, g2 = genomes
    # A overlaps B (half of g1), C is disjoint from both: keys held by one, two and no member occur
    return [[g0, g1[:30_000]], [g1], [g2]]


@pytest.fixture(scope="module")
def members(oracle, dcn, genomes):
    out = []
    for seqs in _member_seqs(genomes):
        o = oracle.Index.build(seqs, k=31, w=15)
        out.append((o, dcn.Index.from_keys(o.keys(), 31, 15)))
    return out


def sample(rng, genomes, n, lo, hi, p_n=0.002):
    reads = []
    for _ in range(n):
        ln = int(rng.integers(lo, hi + 1))
        g = genomes[int(rng.integers(0, len(genomes)))]
        if rng.random() < 0.75 and ln < len(g):
            s = int(rng.integers(0, len(g) - ln))
            r = mutate(rng, g[s:s + ln], 0.01)
            if rng.random() < 0.5:
                r = revcomp(r)
        else:
            r = random_reads(rng, 1, ln, ln)[0]
        a = np.frombuffer(r, dtype=np.uint8).copy()
        if ln:
            a[rng.random(ln) < p_n] = ord("N")
            if rng.random() < 0.1:  # an N run
                s = int(rng.integers(0, ln))
                a[s:s + 40] = ord("N")
        reads.append(a.tobytes())
    return reads


def edge_reads():
    return [b"", b"ACGT", b"A" * 30, b"ACGTN" * 20, b"N" * 200]


def check(oracle, clf, oidx_list, reads, unit_id=None):
    b, o = oracle.concat_reads(reads)
    match, hits, total = clf.classify_batch(b, o, unit_id)
    assert hits.shape == (len(match), len(oidx_list))
    for j, oidx in enumerate(oidx_list):
        keep, h, t = oracle.filter_batch(oidx, b, o, unit_id, abs_threshold=clf.abs_threshold,
                                         rel_threshold=clf.rel_threshold, prefix_length=clf.prefix_length,
                                         deplete=False, threads=4)
        assert total.tolist() == t.tolist(), ("total", j)
        assert hits[:, j].tolist() == h.tolist(), ("hits", j)
        assert ((match >> j) & 1).astype(bool).tolist() == keep.tolist(), ("match", j)
    return match, hits, total


@pytest.mark.parametrize("abs_t,rel_t,prefix", [(2, 0.01, 0), (1, 0.0, 0), (3, 0.2, 0), (2, 0.01, 60)])
def test_three_members_short_reads(oracle, dcn, genomes, members, abs_t, rel_t, prefix):
    rng = np.random.default_rng(abs_t * 10 + prefix)
    reads = sample(rng, genomes, 3000, 80, 160) + edge_reads()
    s = dcn.IndexSet([g for _, g in members])
    assert (s.n, s.k, s.w) == (3, 31, 15)
    union = set()
    for o, _ in members:
        union |= set(o.keys().tolist())
    assert s.n_keys == len(union)
    assert s.memory > 0
    clf = dcn.Classifier(s, abs_threshold=abs_t, rel_threshold=rel_t, prefix_length=prefix,
                         max_batch_bases=1 << 21, max_batch_reads=1 << 13)
    match, hits, _ = check(oracle, clf, [o for o, _ in members], reads)
    assert (hits[:, 0] > 0).any() and (hits[:, 1] > 0).any() and (hits[:, 2] > 0).any()
    assert ((match & 3) == 3).any(), "no read matched both overlapping members"


def test_paired_units(oracle, dcn, genomes, members):
    rng = np.random.default_rng(5)
    reads = sample(rng, genomes, 2000, 100, 151) + [b"", b"ACGT"]
    uid = (np.arange(len(reads)) // 2).astype(np.uint32)
    clf = dcn.Classifier(dcn.IndexSet([g for _, g in members]), max_batch_bases=1 << 21, max_batch_reads=1 << 13)
    check(oracle, clf, [o for o, _ in members], reads, uid)
    clf.prefix_length = 50
    check(oracle, clf, [o for o, _ in members], reads, uid)


def test_one_member_equals_filter_counting_mode(oracle, dcn, genomes, members):
    rng = np.random.default_rng(6)
    reads = sample(rng, genomes, 2000, 50, 300) + edge_reads()
    b, o = oracle.concat_reads(reads)
    gidx = members[1][1]
    clf = dcn.Classifier(dcn.IndexSet([gidx]), max_batch_bases=1 << 21, max_batch_reads=1 << 13)
    proc = dcn.FilterProcessor(gidx, deplete=False, max_batch_bases=1 << 21, max_batch_reads=1 << 13)
    for uid in (None, (np.arange(len(reads)) // 2).astype(np.uint32)):
        match, hits, total = clf.classify_batch(b, o, uid)
        keep, h, t = proc.filter_batch(b, o, uid)
        assert match.astype(bool).tolist() == keep.tolist()
        assert match.max() <= 1
        assert hits[:, 0].tolist() == h.tolist()
        assert total.tolist() == t.tolist()


def test_thirty_two_members_with_repeats(oracle, dcn, genomes, members):
    rng = np.random.default_rng(7)
    reads = sample(rng, genomes, 1500, 80, 400)
    gl = [members[j % 3][1] for j in range(32)]
    s = dcn.IndexSet(gl)
    assert s.n == 32
    clf = dcn.Classifier(s, max_batch_bases=1 << 21, max_batch_reads=1 << 13)
    b, o = oracle.concat_reads(reads)
    match, hits, total = clf.classify_batch(b, o)
    for j in range(32):
        assert hits[:, j].tolist() == hits[:, j % 3].tolist()
        assert ((match >> j) & 1).tolist() == ((match >> (j % 3)) & 1).tolist()
    keep, h, t = oracle.filter_batch(members[2][0], b, o, None, deplete=False, threads=4)
    assert hits[:, 29].tolist() == h.tolist()  # member 29 is members[2]
    assert total.tolist() == t.tolist()
    assert ((match >> 29) & 1).astype(bool).tolist() == keep.tolist()


def test_long_reads_across_tiles_and_the_workgroup_path(oracle, dcn, genomes, members, monkeypatch):
    rng = np.random.default_rng(8)
    # reads of several tiles, reads with more entries / hits than a lane takes, and one whole genome (tens of thousands
    # of entries: several hash partitions of the workgroup kernel's LDS set), among short ones
    long_reads = sample(rng, genomes, 60, 500, 6000, p_n=0.0005)
    whole = mutate(rng, genomes[1], 0.002)
    reads = sample(rng, genomes, 300, 80, 160) + long_reads + [whole, genomes[0] + genomes[2]]
    rng.shuffle(reads)
    ol = [o for o, _ in members]
    for tw in (None, "16", "100"):
        if tw:
            monkeypatch.setenv("DCN_TILE_WINDOWS", tw)
        clf = dcn.Classifier(dcn.IndexSet([g for _, g in members]), max_batch_bases=1 << 22, max_batch_reads=1 << 12)
        _, _, total = check(oracle, clf, ol, reads)
        assert total.max() > 10_000
        uid = (np.arange(len(reads)) // 2).astype(np.uint32)
        check(oracle, clf, ol, reads, uid)


def test_k_above_32(oracle, dcn, genomes):
    seqs = _member_seqs(genomes)
    pairs = []
    for s in seqs:
        o = oracle.Index.build(s, k=41, w=15)
        pairs.append((o, dcn.Index.from_keys(o.keys(), 41, 15)))
    rng = np.random.default_rng(9)
    reads = sample(rng, genomes, 1500, 60, 200) + edge_reads()
    s = dcn.IndexSet([g for _, g in pairs])
    assert s.k == 41
    clf = dcn.Classifier(s, max_batch_bases=1 << 21, max_batch_reads=1 << 13)
    check(oracle, clf, [o for o, _ in pairs], reads)


def test_member_holding_hash_zero(oracle, dcn, genomes, members):
    o0, _ = members[0]
    keys = np.concatenate([o0.keys(), np.array([0], np.uint64)])
    oz = oracle.Index(keys, 31, 15)
    gz = dcn.Index.from_keys(keys, 31, 15)
    s = dcn.IndexSet([gz, members[2][1]])
    assert s.n_keys == len(oz) + len(members[2][0])
    rng = np.random.default_rng(10)
    reads = sample(rng, genomes, 1000, 80, 200)
    clf = dcn.Classifier(s, max_batch_bases=1 << 21, max_batch_reads=1 << 13)
    check(oracle, clf, [oz, members[2][0]], reads)


def test_device_form_equals_host_form(oracle, dcn, genomes, members):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(11)
    reads = sample(rng, genomes, 3000, 100, 151) + sample(rng, genomes, 20, 2000, 5000)
    b, o = oracle.concat_reads(reads)
    uid = (np.arange(len(reads)) // 2).astype(np.uint32)
    clf = dcn.Classifier(dcn.IndexSet([g for _, g in members]), max_batch_bases=1 << 22, max_batch_reads=1 << 13)
    dev = torch.device("cuda:0")
    d_b = torch.from_numpy(b).to(dev)
    d_o = torch.from_numpy(o.view(np.int64)).to(dev)
    d_u = torch.from_numpy(uid.view(np.int32)).to(dev)
    for unit, n_units in ((None, len(reads)), (d_u, int(uid[-1]) + 1)):
        d_m = torch.zeros(n_units, dtype=torch.int32, device=dev)
        d_h = torch.zeros(n_units * 3, dtype=torch.int32, device=dev)
        d_t = torch.zeros(n_units, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        clf.classify_batch_device(d_b.data_ptr(), d_o.data_ptr(), len(reads), len(b), d_m.data_ptr(), d_h.data_ptr(),
                                  d_t.data_ptr(), d_unit_id=unit.data_ptr() if unit is not None else None,
                                  n_units=n_units)
        clf.synchronize()
        match, hits, total = clf.classify_batch(b, o, None if unit is None else uid)
        assert d_m.cpu().numpy().view(np.uint32).tolist() == match.tolist()
        assert d_h.cpu().numpy().view(np.uint32).reshape(n_units, 3).tolist() == hits.tolist()
        assert d_t.cpu().numpy().view(np.uint32).tolist() == total.tolist()


def test_refusals(dcn, genomes, members):
    N = dcn._native
    g31 = members[0][1]
    g41 = dcn.Index.from_keys(np.arange(1, 100, dtype=np.uint64), 41, 15)
    g33 = dcn.Index.from_keys(np.arange(1, 100, dtype=np.uint64), 31, 13)
    for bad, text in (([g31, g41], "Incompatible headers"), ([g31, g33], "Incompatible headers"), ([], "1 to 32"),
                      ([g31] * 33, "1 to 32")):
        with pytest.raises(dcn.DeaconHipError) as e:
            dcn.IndexSet(bad)
        assert e.value.code == N.DCN_ERR_ARG and text in e.value.message
    # another minimizer rule
    dcn.set_minimizer_variant(7, 16, "add")
    try:
        gv = dcn.Index.from_keys(np.arange(1, 100, dtype=np.uint64), 31, 15)
    finally:
        dcn.set_minimizer_variant()
    with pytest.raises(dcn.DeaconHipError) as e:
        dcn.IndexSet([g31, gv])
    assert e.value.code == N.DCN_ERR_ARG and "minimizer rules" in e.value.message
    # another device, where there is one
    n = C.c_int()
    N.check(N.lib().dcn_device_count(C.byref(n)))
    if n.value > 1:
        g1 = g31.clone(1)
        with pytest.raises(dcn.DeaconHipError) as e:
            dcn.IndexSet([g31, g1])
        assert e.value.code == N.DCN_ERR_ARG and "different devices" in e.value.message
    # a context whose index does not agree with the set; a plain index where a set is expected
    s = dcn.IndexSet([g31])
    p41 = dcn.FilterProcessor(g41, max_batch_bases=1 << 16, max_batch_reads=256)
    b = np.frombuffer(b"ACGT" * 40, np.uint8).copy()
    o = np.array([0, len(b)], np.uint64)
    m, h, t = np.zeros(1, np.uint32), np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    prm = N.Params(2, 0.01, 0, 0, 0)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert N.lib().dcn_classify_batch(p41._h, s._h, ptr(b), ptr(o), None, 1, C.byref(prm), ptr(m), ptr(h), ptr(t)) == N.DCN_ERR_ARG
    assert b"differ" in N.lib().dcn_last_error()
    p31 = dcn.FilterProcessor(g31, max_batch_bases=1 << 16, max_batch_reads=256)
    assert N.lib().dcn_classify_batch(p31._h, g31._h, ptr(b), ptr(o), None, 1, C.byref(prm), ptr(m), ptr(h), ptr(t)) == N.DCN_ERR_ARG
    assert b"not a labelled set" in N.lib().dcn_last_error()
    assert N.lib().dcn_classify_batch(p31._h, s._h, ptr(b), ptr(o), None, 1, C.byref(prm), ptr(m), ptr(h), ptr(t)) == 0


def test_counters_unchanged_and_members_may_go(oracle, dcn, genomes):
    seqs = _member_seqs(genomes)
    ol = [oracle.Index.build(s, k=31, w=15) for s in seqs]
    gl = [dcn.Index.from_keys(o.keys(), 31, 15) for o in ol]
    s = dcn.IndexSet(gl)
    rng = np.random.default_rng(12)
    reads = sample(rng, genomes, 2000, 80, 200)
    b, o = oracle.concat_reads(reads)
    clf = dcn.Classifier(s, max_batch_bases=1 << 21, max_batch_reads=1 << 13)
    before = clf.classify_batch(b, o)
    for g in gl:  # the set owns its table
        g.close()
    del gl
    after = check(oracle, clf, ol, reads)
    for x, y in zip(before, after):
        assert x.tolist() == y.tolist()
    assert all(v == 0 for v in clf.stats().values())
    # on a context that has filtered: classification adds nothing to its six counters
    gidx = dcn.Index.from_keys(ol[0].keys(), 31, 15)
    proc = dcn.FilterProcessor(gidx, max_batch_bases=1 << 21, max_batch_reads=1 << 13)
    proc.filter_batch(b, o)
    s0 = proc.stats()
    assert s0["total_seqs"] == len(reads)
    N = dcn._native
    n_units = len(reads)
    m, h, t = np.zeros(n_units, np.uint32), np.zeros(n_units * 3, np.uint32), np.zeros(n_units, np.uint32)
    prm = N.Params(2, 0.01, 0, 1, 0)  # (deplete is ignored by classification)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    N.check(N.lib().dcn_classify_batch(proc._h, s._h, ptr(b), ptr(o), None, len(reads), C.byref(prm), ptr(m), ptr(h), ptr(t)))
    assert proc.stats() == s0
    assert m.tolist() == after[0].tolist() and h.reshape(-1, 3).tolist() == after[1].tolist()


# ---- the command line ---------------------------------------------------------------------------------------------------
def _fastq(path, names, reads):
    with open(path, "w") as f:
        for nm, r in zip(names, reads):
            f.write(f"@{nm} extra\n{r.decode()}\n+\n{'I' * len(r)}\n")


def _kept_ids(path):
    lines = open(path).read().splitlines()
    return [lines[i][1:].split()[0] for i in range(0, len(lines), 4)]


def test_cli_classify_equals_separate_filter_runs(oracle, genomes, tmp_path):
    rng = np.random.default_rng(13)
    idx = []
    for j, seqs in enumerate(_member_seqs(genomes)):
        fa = tmp_path / f"g{j}.fa"
        fa.write_text("".join(f">s{i}\n{s.decode()}\n" for i, s in enumerate(seqs)))
        out = tmp_path / f"ref{j}.idx"
        subprocess.run([CLI, "index", "build", str(fa), "-o", str(out), "-q"], check=True, capture_output=True, timeout=300)
        idx.append(str(out))
    reads = sample(rng, genomes, 1199, 60, 250) + [b"ACGT"]
    names = [f"r{i}" for i in range(len(reads))]
    fq = tmp_path / "reads.fq"
    _fastq(fq, names, reads)
    m1, m2 = tmp_path / "m1.fq", tmp_path / "m2.fq"
    _fastq(m1, names[0::2], reads[0::2])
    _fastq(m2, [n + "b" for n in names[1::2]], reads[1::2])
    flags = ["-a", "2", "-r", "0.05", "-p", "120"]
    for inputs in ([str(fq)], [str(m1), str(m2)]):
        tsv, summ = tmp_path / "per_read.tsv", tmp_path / "summary.json"
        x = sum((["-x", p] for p in idx), [])
        subprocess.run([CLI, "classify", *x, *inputs, *flags, "--per-read", str(tsv), "-s", str(summ), "-q"], check=True,
                       capture_output=True, timeout=300)
        rows = [ln.split("\t") for ln in open(tsv).read().splitlines()]
        assert rows[0] == ["id", "length", "minimizers", "hits:ref0", "hits:ref1", "hits:ref2", "matched"]
        rows = rows[1:]
        js = json.load(open(summ))
        seqs_in = sum(1 if len(inputs) == 1 else 2 for _ in rows)
        assert js["seqs_in"] == seqs_in
        assert js["bp_in"] == sum(int(r[1]) for r in rows)
        for j, p in enumerate(idx):
            out1, s1 = tmp_path / f"keep{j}.fq", tmp_path / f"keep{j}.json"
            cmd = [CLI, "filter", p, *inputs, *flags, "-o", str(out1), "-s", str(s1), "-q"]
            if len(inputs) == 2:
                cmd += ["-O", str(tmp_path / f"keep{j}_2.fq")]
            subprocess.run(cmd, check=True, capture_output=True, timeout=300)
            kept = set(_kept_ids(out1))
            matched = {r[0] for r in rows if f"ref{j}" in r[-1].split(",")}
            assert matched == kept, j
            fj = json.load(open(s1))
            ij = js["indexes"][j]
            assert (ij["path"], ij["k"], ij["w"]) == (p, 31, 15)
            assert ij["seqs_matched"] == fj["seqs_out"] and ij["bp_matched"] == fj["bp_out"]
            assert ij["seqs_matched_proportion"] == fj["seqs_out_proportion"]
        assert all(r[-1] == "-" or r[-1] for r in rows)

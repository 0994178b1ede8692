"""The seams of classification (classify.hip, classify_api.hip's entry points, `deacon-hip classify`) that random reads
do not reach: the lane kernel's entry and hit limits at their exact edges, the workgroup kernel's fill-limit retry, member
labels in displaced slots of a crowded set, every minimizer rule, one context through many different calls, a set used as
a plain index, and the command line over many batches.  Every comparison is exact.

The constructed units are made of single-window reads: with w = 15 a read of k + 14 bases has exactly one window, so it
is exactly one dump entry (invalid when its one window's k-mers all hold the read's middle base, an N).  A unit of such
reads (through unit_id) has exactly the entries, valid entries, duplicates and hits it is built with, and is checked
against a plain statement of the counts as well as against the oracle."""
import ctypes as C
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, random_reads
from oracle.oracle import VARIANTS
from test_classify_replicas import group_of, key_in_group, mix_hi32, partition
from test_gpu_classify import CLI, _fastq, _kept_ids, _member_seqs, check, edge_reads, sample

pytestmark = pytest.mark.gpu

W = 15
LANE_ENTRIES = 64                 # DCN_CLS_LANE_ENTRIES (dcn_classify.h)
HALF, FULL = 2048, 3072           # classify_big_kernel: entries per partition aimed at, fill limit of its LDS set


def group_slots():
    text = open(os.path.join(ROOT, "deacon-server_amd", "csrc", "dcn_internal.h")).read()
    return int(re.search(r"#define DCN_GROUP_SLOTS (\d+)", text).group(1))


@pytest.fixture(scope="module")
def genomes():
    rng = np.random.default_rng(171)
    return random_reads(rng, 3, 30_000, 30_000)


class Pool:
    """distinct single-window reads (k + w - 1 random bases) with their one minimizer hash, handed out once each"""

    def __init__(self, oracle, k, n, seed):
        self.oracle, self.k, self.l = oracle, k, k + W - 1
        self.rng = np.random.default_rng(seed)
        codes = np.frombuffer(b"ACGT", np.uint8)[self.rng.integers(0, 4, (n, self.l))]
        reads, hashes, seen = [], [], set()
        for row in codes:
            r = row.tobytes()
            h, _ = oracle.minimizer_hashes_and_positions(r, k, W)
            assert len(h) == 1
            if int(h[0]) in seen:
                continue
            seen.add(int(h[0]))
            reads.append(r)
            hashes.append(int(h[0]))
        self.reads, self.hashes = reads, np.array(hashes, np.uint64)
        self.used = np.zeros(len(reads), bool)

    def take(self, count, where=None):
        """count unused (read, hash) pairs, whose hashes satisfy `where` (a predicate on a u64 array)"""
        ok = ~self.used if where is None else ~self.used & where(self.hashes)
        idx = np.flatnonzero(ok)[:count]
        assert len(idx) == count, "pool too small"
        self.used[idx] = True
        return [(self.reads[i], int(self.hashes[i])) for i in idx]

    def invalid(self):
        """a single-window read whose every k-mer holds its middle base, an N: one dump entry, not valid"""
        r = bytearray(np.frombuffer(b"ACGT", np.uint8)[self.rng.integers(0, 4, self.l)].tobytes())
        r[self.l // 2] = ord("N")
        r = bytes(r)
        assert len(self.oracle.minimizer_hashes_and_positions(r, self.k, W)[0]) == 0
        return (r, None)


def required(abs_t, rel_t, total):
    """dcn_required_hits: max(abs, total == 0 ? 0 : max(1, round_half_away(rel * total)))"""
    if total == 0:
        return abs_t
    r = rel_t * total
    f = math.floor(r)
    return max(abs_t, max(1, int(f + 1 if r - f >= 0.5 else f)))


class Units:
    """a batch of units built entry by entry, with the member sets that go with it"""

    def __init__(self, n_members):
        self.units = []  # lists of (read, hash | None)
        self.members = [set() for _ in range(n_members)]

    def add(self, entries, held=()):
        self.units.append(list(entries))
        for j, hs in held:
            self.members[j].update(int(h) for h in hs)

    def batch(self):
        reads, uid = [], []
        for u, es in enumerate(self.units):
            if not es:
                es = [(b"", None)]  # a unit without entries: one empty read
            for r, _ in es:
                reads.append(r)
                uid.append(u)
        return reads, np.array(uid, np.uint32)

    def expected(self, abs_t, rel_t):
        """the plain statement: total = valid entries, hits[j] = |distinct valid hashes & member j|, match bit j =
        hits[j] >= required(total)"""
        n = len(self.members)
        match = np.zeros(len(self.units), np.uint32)
        hits = np.zeros((len(self.units), n), np.uint32)
        total = np.zeros(len(self.units), np.uint32)
        for u, es in enumerate(self.units):
            valid = [h for _, h in es if h is not None]
            total[u] = len(valid)
            d = set(valid)
            req = required(abs_t, rel_t, len(valid))
            for j, m in enumerate(self.members):
                hits[u, j] = len(d & m)
                if hits[u, j] >= req:
                    match[u] |= np.uint32(1 << j)
        return match, hits, total

    def index_pairs(self, oracle, dcn, k, rng):
        out = []
        for m in self.members:
            keys = np.array(sorted(m) + [int(rng.integers(1, 2**63))], np.uint64)  # (never empty)
            out.append((oracle.Index(keys, k, W), dcn.Index.from_keys(keys, k, W)))
        return out


def _hits_of(entries):
    return [h for _, h in entries if h is not None]


def _constructed_units(oracle, k):
    """Members: 0 holds every hit of a unit, 1 every other one, 2 none, 3 the same as 0 (threshold-tie units hand out
    their own holdings)."""
    pool = Pool(oracle, k, 44_000, 1000 + k)
    rng = np.random.default_rng(k)
    U = Units(4)

    def std(entries, hits):
        hits = list(hits)
        U.add(entries, [(0, hits), (1, hits[::2]), (3, hits)])

    # -- the workgroup kernel's retry (taken first: they need hashes from chosen ranges) --------------------------------
    # ~3 500 distinct hits with mix_hi32 < 2^30: one partition at P = 2 and at P = 4, split at P = 8
    a = pool.take(3500, lambda h: mix_hi32(h) < np.uint64(1 << 30))
    assert set(partition(np.array([h for _, h in a], np.uint64), 4).tolist()) == {0}
    a_other = pool.take(300, lambda h: mix_hi32(h) >= np.uint64(1 << 31)) + [pool.invalid() for _ in range(40)]
    es = a + a_other
    rng.shuffle(es)
    assert (len(es) - 40 + HALF - 1) // HALF == 2
    std(es, _hits_of(a))
    # ~3 200 distinct hits in partition 2 of 5, duplicated to ~8 200 entries: first P = 5, split at P = 10
    b = pool.take(3200, lambda h: partition(h, 5) == np.uint64(2))
    es = b + [b[i % len(b)] for i in range(5000)]
    rng.shuffle(es)
    assert (len(es) + HALF - 1) // HALF == 5
    std(es, _hits_of(b))
    # exactly FULL distinct hits, all in partition 0 of 2 (no retry unless a lost CAS counted twice: either is right)
    c = pool.take(FULL, lambda h: mix_hi32(h) < np.uint64(1 << 31))
    assert (FULL + HALF - 1) // HALF == 2
    std(c, _hits_of(c))

    # -- the lane kernel's entry limit ---------------------------------------------------------------------------------
    for n in (0, 1, 63, 64, 65):
        es = pool.take(n)
        std(es, [h for _, h in es[::3]])
    for n, bad in ((64, 4), (65, 1), (65, 10), (64, 64), (65, 65)):  # total <= 64 while the entry count crosses it
        es = pool.take(n - bad) + [pool.invalid() for _ in range(bad)]
        rng.shuffle(es)
        std(es, [h for _, h in es[::2] if h is not None])

    # -- the lane kernel's hit limit -----------------------------------------------------------------------------------
    for d, n in ((31, 40), (32, 40), (33, 40), (33, 64), (32, 64), (33, 34)):
        hits = pool.take(d)
        rest = pool.take(n - d)
        es = hits[:-1] + rest
        rng.shuffle(es)
        es.append(hits[-1])  # the last distinct hit is the unit's last entry: `over` fires after 32 were counted
        std(es, _hits_of(hits))
    for n in (64, 65):  # all hits: over fires early
        es = pool.take(n)
        std(es, _hits_of(es))
    # duplicates: the distinct hits stay, the entries grow
    hits = pool.take(32)
    es = hits + [hits[i % 32] for i in range(20)] + pool.take(12)
    rng.shuffle(es)
    std(es, _hits_of(hits))
    hits = pool.take(33)
    es = hits[:-1] + [hits[i % 32] for i in range(20)]
    rng.shuffle(es)
    es.append(hits[-1])
    std(es, _hits_of(hits))
    # 11 distinct hits among 21 entries: required 11 at rel 0.5; one duplicate keeps it (22 -> 11), two break it (23 -> 12)
    hits, other = pool.take(11), pool.take(10)
    for dup in (0, 1, 2, 3):
        es = hits + other + hits[:dup]
        rng.shuffle(es)
        std(es, _hits_of(hits))

    # -- threshold ties per member: rel 0.5, odd totals (x.5 exactly), hits = required - 1, required, required + 1 -----
    for t in (1, 3, 5, 21, 33, 63, 65, 129):
        es = pool.take(t)
        hs = _hits_of(es)
        req = required(1, 0.5, t)
        held = [(j, hs[:max(0, min(t, req - 1 + j))]) for j in range(3)] + [(3, hs[-1:])]
        U.add(es, held)
        # the same with duplicates of a hit: an even total, the distinct hits unchanged
        es2 = pool.take(t)
        hs2 = _hits_of(es2)
        U.add(es2 + es2[:1], [(j, hs2[:max(0, min(t, req - 1 + j))]) for j in range(3)])
    return U


@pytest.mark.parametrize("k", [31, 41])
def test_constructed_units_at_the_kernels_limits(oracle, dcn, k):
    U = _constructed_units(oracle, k)
    reads, uid = U.batch()
    pairs = U.index_pairs(oracle, dcn, k, np.random.default_rng(k + 1))
    ol = [o for o, _ in pairs]
    s = dcn.IndexSet([g for _, g in pairs])
    assert s.n_keys == len(set().union(*U.members)) + 4
    for abs_t, rel_t in ((1, 0.5), (0, 0.5), (2, 0.01), (0, 0.0)):
        clf = dcn.Classifier(s, abs_threshold=abs_t, rel_threshold=rel_t, max_batch_bases=1 << 21,
                             max_batch_reads=1 << 15)
        match, hits, total = check(oracle, clf, ol, reads, uid)
        want = U.expected(abs_t, rel_t)
        assert total.tolist() == want[2].tolist(), (abs_t, rel_t)
        for j in range(len(ol)):
            assert hits[:, j].tolist() == want[1][:, j].tolist(), (abs_t, rel_t, j)
        assert match.tolist() == want[0].tolist(), (abs_t, rel_t)
        # a unit without valid entries matches every member when abs_threshold is 0 (required 0), none otherwise
        assert (total == 0).sum() == 3
        assert match[total == 0].tolist() == [0xF if abs_t == 0 else 0] * 3
        clf.close()
    # the cases reach what they aim at
    assert total[0] == 3800 and total[1] == 8200 and hits[2, 0] == FULL
    assert hits[:, 2].max() > 0 and hits[:, 3].max() > 0  # (the tie units' members)


# ---- member labels under displacement --------------------------------------------------------------------------------
def displaced_members(oracle):
    """The construction of test_member_labels_in_displaced_slots, for a table built under DCN_TABLE_SLOTS_PER_KEY=2:
    (k, the table's groups, the three members' key arrays, the target home groups, the single-window reads)."""
    k = 31
    S = group_slots()
    G = 2048 // S                      # a 2 048-slot table: the member key counts sum to 509..1020
    pool = Pool(oracle, k, 24_000, 7)
    rng = np.random.default_rng(8)
    home = group_of(pool.hashes, G)
    counts = np.bincount(home.astype(np.int64), minlength=G)
    targets = [G - 1, G - 5]
    for g in range(3, G - 8, 24):
        if counts[g] >= 5:
            targets.append(g)
    targets = targets[:44]
    m0, m1, m2 = set(), set(), set()
    reads = []
    for g in targets:
        rs = pool.take(5, lambda h, g=g: group_of(h, G) == np.uint64(g))
        (ra, ha), (rb, hb), (rc, hc), (rd, hd), (re_, he) = rs
        m1.update([ha, hc])
        m2.update([hb, hc])
        m0.add(he)
        fill = [key_in_group(rng, g, G, S), key_in_group(rng, (g + 1) % G, G, S)]
        for f in fill:
            m0.update(int(x) for x in f)
        m2.add(int(fill[0][0]))
        reads += [ra, rb, rc, rd, re_]
    while len(m0) + len(m1) + len(m2) < 980:  # the rest of the half-full table: keys anywhere
        m0.add(int(rng.integers(1, 2**63)))
    n_sum = len(m0) + len(m1) + len(m2)
    rule = 64
    while rule * S < n_sum * 2 + 8:
        rule <<= 1
    assert rule == G
    rng.shuffle(reads)
    return k, G, [np.array(sorted(m), np.uint64) for m in (m0, m1, m2)], targets, reads


def test_member_labels_in_displaced_slots(oracle, dcn, monkeypatch):
    """At 2 slots per key the set is about half full.  Member 0 fills the home group of every target hash and the group
    after it, so the targets (held by members 1 and 2) sit two or more groups away; some home groups are the last one,
    whose chains wrap to group 0.  Some fillers are in member 2 too (their labels are ORed into slots member 0 placed),
    and some read hashes in the same groups are in no member: their lookups walk the same chains and find nothing."""
    monkeypatch.setenv("DCN_TABLE_SLOTS_PER_KEY", "2")
    S = group_slots()
    k, G, members, targets, reads = displaced_members(oracle)
    m0, m1, m2 = (set(m.tolist()) for m in members)
    ol = [oracle.Index(m, k, W) for m in members]
    s = dcn.IndexSet([dcn.Index.from_keys(m, k, W) for m in members])
    assert s.memory % 12 == 0 and s.memory // 12 == G * S  # 8 bytes of key and 4 of label per slot
    assert s.n_keys == len(m0 | m1 | m2)
    assert len(m0 | m1 | m2) * 2 > G * S * 0.85  # about half full
    clf = dcn.Classifier(s, abs_threshold=1, rel_threshold=0.0, max_batch_bases=1 << 20, max_batch_reads=1 << 13)
    _, hits, _ = check(oracle, clf, ol, reads)  # one read per unit: the lane path
    assert [int((hits[:, j] > 0).sum()) for j in range(3)] == [len(targets), 2 * len(targets), 2 * len(targets)]
    short = (np.arange(len(reads)) // 3).astype(np.uint32)
    check(oracle, clf, ol, reads, short)
    big = (np.arange(len(reads)) // 70).astype(np.uint32)  # 70 entries per unit: the workgroup path
    _, hits, total = check(oracle, clf, ol, reads, big)
    assert total.max() > LANE_ENTRIES


# ---- minimizer rules ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_every_minimizer_rule(oracle, dcn, genomes, variant):
    rng = np.random.default_rng(VARIANTS.index(variant))
    reads = sample(rng, genomes, 600, 60, 200) + sample(rng, genomes, 6, 3000, 9000) + edge_reads()
    uid = (np.arange(len(reads)) // 2).astype(np.uint32)
    dcn.set_minimizer_variant(*variant)
    oracle.set_variant(*variant)
    try:
        ol = [oracle.Index.build(s, k=31, w=15) for s in _member_seqs(genomes)]
        s = dcn.IndexSet([dcn.Index.from_keys(o.keys(), 31, 15) for o in ol])
        clf = dcn.Classifier(s, max_batch_bases=1 << 21, max_batch_reads=1 << 12)
        _, hits, total = check(oracle, clf, ol, reads)
        assert total.max() > LANE_ENTRIES and (hits > 0).any()
        check(oracle, clf, ol, reads, uid)
    finally:
        dcn.set_minimizer_variant()
        oracle.set_variant()


# ---- one context, many calls --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three(oracle, dcn, genomes):
    ol = [oracle.Index.build(s, k=31, w=15) for s in _member_seqs(genomes)]
    return ol, [dcn.Index.from_keys(o.keys(), 31, 15) for o in ol]


def _union(oracle, ol):
    return oracle.Index(np.unique(np.concatenate([o.keys() for o in ol])), 31, 15)


class _ClassifierOn:
    """classify_batch* of dcn.Classifier on a context someone else owns (a FilterProcessor's)"""

    def __init__(self, dcn, ctx_h, index_set):
        self._c = dcn.Classifier.__new__(dcn.Classifier)
        self._c.__dict__.update(index_set=index_set, abs_threshold=2, rel_threshold=0.01, prefix_length=0, _h=ctx_h)

    def __getattr__(self, name):
        return getattr(self._c, name)

    def release(self):
        self._c._h = None


def test_one_context_switches_sets(oracle, dcn, genomes, three):
    ol, gl = three
    rng = np.random.default_rng(21)
    reads = sample(rng, genomes, 800, 60, 300) + sample(rng, genomes, 4, 2000, 6000) + edge_reads()
    s3 = dcn.IndexSet(gl)
    clf = dcn.Classifier(s3, max_batch_bases=1 << 21, max_batch_reads=1 << 12)
    for n in (3, 32, 1, 3):
        clf.index_set = s3 if n == 3 else dcn.IndexSet([gl[(j + 1) % 3] for j in range(n)])
        _, hits, _ = check(oracle, clf, [ol[(j + (n != 3)) % 3] for j in range(n)], reads)
        assert hits.shape[1] == n


def test_filter_and_classify_interleaved_on_one_context(oracle, dcn, genomes, three):
    torch = pytest.importorskip("torch")
    ol, gl = three
    union = _union(oracle, ol)
    rng = np.random.default_rng(22)
    s = dcn.IndexSet(gl)
    proc = dcn.FilterProcessor(s, max_batch_bases=1 << 21, max_batch_reads=1 << 12)  # a context over the set's union
    alone = dcn.FilterProcessor(s, max_batch_bases=1 << 21, max_batch_reads=1 << 12)  # the same filter calls only
    clf = _ClassifierOn(dcn, proc._h, s)
    dev = torch.device("cuda:0")
    try:
        for step in range(3):
            reads = sample(rng, genomes, 700, 60, 250) + sample(rng, genomes, 3, 1500, 5000)
            b, o = oracle.concat_reads(reads)
            n = len(reads)
            want_f = oracle.filter_batch(union, b, o, None, threads=4)
            got = proc.filter_batch(b, o)
            alone.filter_batch(b, o)
            for g, w in zip(got, want_f):
                assert g.tolist() == w.tolist(), step
            match, hits, total = check(oracle, clf, ol, reads)
            d_b = torch.from_numpy(b).to(dev)
            d_o = torch.from_numpy(o.view(np.int64)).to(dev)
            d_k = torch.zeros(n, dtype=torch.uint8, device=dev)
            d_h = torch.zeros(n, dtype=torch.int32, device=dev)
            d_t = torch.zeros(n, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            proc.filter_batch_device(d_b.data_ptr(), d_o.data_ptr(), n, len(b), d_k.data_ptr(), d_h.data_ptr(),
                                     d_t.data_ptr())
            proc.synchronize()
            assert d_k.cpu().numpy().astype(bool).tolist() == want_f[0].tolist()
            assert d_h.cpu().numpy().view(np.uint32).tolist() == want_f[1].tolist()
            assert d_t.cpu().numpy().view(np.uint32).tolist() == want_f[2].tolist()
            alone.filter_batch_device(d_b.data_ptr(), d_o.data_ptr(), n, len(b), d_k.data_ptr(), d_h.data_ptr(),
                                      d_t.data_ptr())
            alone.synchronize()
            d_m = torch.zeros(n, dtype=torch.int32, device=dev)
            d_h3 = torch.zeros(n * 3, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            clf.classify_batch_device(d_b.data_ptr(), d_o.data_ptr(), n, len(b), d_m.data_ptr(), d_h3.data_ptr(),
                                      d_t.data_ptr())
            clf.synchronize()
            assert d_m.cpu().numpy().view(np.uint32).tolist() == match.tolist()
            assert d_h3.cpu().numpy().view(np.uint32).reshape(n, 3).tolist() == hits.tolist()
            assert d_t.cpu().numpy().view(np.uint32).tolist() == total.tolist()
        st = proc.stats()
        assert st == alone.stats() and st["total_seqs"] > 0
    finally:
        clf.release()


def test_device_classify_without_hits_and_totals(oracle, dcn, genomes, three):
    torch = pytest.importorskip("torch")
    ol, gl = three
    rng = np.random.default_rng(23)
    reads = sample(rng, genomes, 1500, 60, 250) + sample(rng, genomes, 5, 2000, 6000)
    b, o = oracle.concat_reads(reads)
    uid = (np.arange(len(reads)) // 2).astype(np.uint32)
    clf = dcn.Classifier(dcn.IndexSet(gl), max_batch_bases=1 << 21, max_batch_reads=1 << 12)
    dev = torch.device("cuda:0")
    d_b = torch.from_numpy(b).to(dev)
    d_o = torch.from_numpy(o.view(np.int64)).to(dev)
    d_u = torch.from_numpy(uid.view(np.int32)).to(dev)
    for unit, n_units in ((None, len(reads)), (d_u, int(uid[-1]) + 1)):
        want = check(oracle, clf, ol, reads, None if unit is None else uid)[0]
        d_m = torch.full((n_units,), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        clf.classify_batch_device(d_b.data_ptr(), d_o.data_ptr(), len(reads), len(b), d_m.data_ptr(), None, None,
                                  d_unit_id=None if unit is None else unit.data_ptr(), n_units=n_units)
        clf.synchronize()
        assert d_m.cpu().numpy().view(np.uint32).tolist() == want.tolist()


def test_device_classify_with_refused_offsets(oracle, dcn, genomes, three):
    torch = pytest.importorskip("torch")
    ol, gl = three
    rng = np.random.default_rng(24)
    g = genomes[1]
    reads = [g[x:x + 150] for x in rng.integers(0, len(g) - 150, 3000).tolist()] + [g[:20_000]]
    b, o = oracle.concat_reads(reads)
    n = len(reads)
    clf = dcn.Classifier(dcn.IndexSet(gl), max_batch_bases=1 << 20, max_batch_reads=4096)
    want = check(oracle, clf, ol, reads)
    dev = torch.device("cuda:0")
    d_b = torch.from_numpy(b).to(dev)
    d_good = torch.from_numpy(o.view(np.int64)).to(dev)
    d_m = torch.zeros(n, dtype=torch.int32, device=dev)
    d_h = torch.zeros(n * 3, dtype=torch.int32, device=dev)
    d_t = torch.zeros(n, dtype=torch.int32, device=dev)
    bad_arrays = {
        "leftovers": rng.integers(0, 2**63 - 1, n + 1, dtype=np.int64),
        "decreasing": o.view(np.int64)[::-1].copy(),
        "beyond the batch": o.view(np.int64) + np.int64(len(b)),
        "one bad read": np.concatenate([o.view(np.int64)[:1500], [np.int64(7)], o.view(np.int64)[1501:]]),
        "all ones": np.full(n + 1, -1, dtype=np.int64),
    }
    for name, arr in bad_arrays.items():
        d_bad = torch.from_numpy(np.ascontiguousarray(arr)).to(dev)
        for t in (d_m, d_h, d_t):
            t.fill_(0x5A5A)
        torch.cuda.synchronize()
        clf.classify_batch_device(d_b.data_ptr(), d_bad.data_ptr(), n, len(b), d_m.data_ptr(), d_h.data_ptr(),
                                  d_t.data_ptr())
        with pytest.raises(dcn.DeaconHipError) as e:
            clf.synchronize()
        assert e.value.code == dcn._native.DCN_ERR_ARG, name
        clf.synchronize()  # (reported once)
        for t in (d_m, d_h, d_t):
            assert not t.cpu().numpy().any(), name
        clf.classify_batch_device(d_b.data_ptr(), d_good.data_ptr(), n, len(b), d_m.data_ptr(), d_h.data_ptr(),
                                  d_t.data_ptr())
        clf.synchronize()
        assert d_m.cpu().numpy().view(np.uint32).tolist() == want[0].tolist(), name
        assert d_h.cpu().numpy().view(np.uint32).reshape(n, 3).tolist() == want[1].tolist(), name
        assert d_t.cpu().numpy().view(np.uint32).tolist() == want[2].tolist(), name


# ---- a set as a plain index ---------------------------------------------------------------------------------------------
class _Borrowed:
    """dcn.Index's methods on a handle someone else owns (an IndexSet's)"""

    def __init__(self, dcn, h, device):
        self._i = dcn.Index.__new__(dcn.Index)
        dcn.Index.__init__(self._i, h, device)

    def __getattr__(self, name):
        return getattr(self._i, name)

    def release(self):
        self._i._h = None


def test_set_serves_as_its_union(oracle, dcn, genomes, three, tmp_path):
    ol, gl = three
    union = _union(oracle, ol)
    want_keys = sorted(union.keys().tolist())
    s = dcn.IndexSet(gl)
    v = _Borrowed(dcn, s._h, s.device)
    try:
        assert (v.kmer_length, v.window_size, v.n_keys) == (31, 15, len(union))
        assert sorted(v.keys().tolist()) == want_keys
        path = str(tmp_path / "set.idx")
        v.write(path)
        back = oracle.Index.read(path)
        assert (back.k, back.w) == (31, 15) and sorted(back.keys().tolist()) == want_keys
        rng = np.random.default_rng(25)
        reads = sample(rng, genomes, 1500, 60, 250) + sample(rng, genomes, 4, 2000, 6000) + edge_reads()
        b, o = oracle.concat_reads(reads)
        want = oracle.filter_batch(union, b, o, None, threads=4)
        proc = dcn.FilterProcessor(v, max_batch_bases=1 << 21, max_batch_reads=1 << 12)
        got = proc.filter_batch(b, o)
        for x, y in zip(got, want):
            assert x.tolist() == y.tolist()
        assert proc.filter_batch(b, o, counts=False).tolist() == want[0].tolist()
        h = C.c_void_p()
        dcn._native.check(dcn._native.lib().dcn_index_clone(s._h, 0, C.byref(h)))
        plain = dcn.Index(h, 0)
        assert sorted(plain.keys().tolist()) == want_keys
        p2 = dcn.FilterProcessor(plain, max_batch_bases=1 << 21, max_batch_reads=1 << 12)
        for x, y in zip(p2.filter_batch(b, o), want):
            assert x.tolist() == y.tolist()
        m = np.zeros(len(reads), np.uint32)
        prm = dcn._native.Params(2, 0.01, 0, 0, 0)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = dcn._native.lib().dcn_classify_batch(p2._h, plain._h, ptr(b), ptr(o), None, len(reads), C.byref(prm),
                                                  ptr(m), None, None)
        assert rc == dcn._native.DCN_ERR_ARG and b"not a labelled set" in dcn._native.lib().dcn_last_error()
        proc.close()
        p2.close()
    finally:
        v.release()


def test_set_as_a_member_of_a_set(oracle, dcn, genomes, three):
    ol, gl = three
    inner = dcn.IndexSet(gl[:2])
    outer = dcn.IndexSet([inner, gl[2]])
    assert outer.n == 2 and outer.n_keys == len(_union(oracle, ol))
    rng = np.random.default_rng(26)
    reads = sample(rng, genomes, 1500, 60, 250) + sample(rng, genomes, 4, 2000, 6000) + edge_reads()
    clf = dcn.Classifier(outer, max_batch_bases=1 << 21, max_batch_reads=1 << 12)
    _, hits, _ = check(oracle, clf, [_union(oracle, ol[:2]), ol[2]], reads)
    assert (hits[:, 0] > 0).any() and (hits[:, 1] > 0).any()


# ---- the command line over many batches -------------------------------------------------------------------------------
def test_cli_classify_over_many_batches(oracle, genomes, tmp_path):
    rng = np.random.default_rng(27)
    idx = []
    for j, seqs in enumerate(_member_seqs(genomes)):
        fa = tmp_path / f"g{j}.fa"
        fa.write_text("".join(f">s{i}\n{s.decode()}\n" for i, s in enumerate(seqs)))
        out = tmp_path / f"ref{j}.idx"
        subprocess.run([CLI, "index", "build", str(fa), "-o", str(out), "-q"], check=True, capture_output=True, timeout=300)
        idx.append(str(out))
    hook = 3000  # bases per batch; the first context takes twice that
    reads = sample(rng, genomes, 600, 60, 250)
    reads[300] = genomes[1][1000:1000 + 3 * hook]  # longer than the context: it is made again, larger
    reads[301] = genomes[0][:2 * hook + 7]
    names = [f"r{i}" for i in range(len(reads))]
    fq = tmp_path / "reads.fq"
    _fastq(fq, names, reads)
    m1, m2 = tmp_path / "m1.fq", tmp_path / "m2.fq"
    _fastq(m1, names[0::2], reads[0::2])
    _fastq(m2, [n + "b" for n in names[1::2]], reads[1::2])
    flags = ["-a", "2", "-r", "0.05"]
    x = sum((["-x", p] for p in idx), [])
    for inputs in ([str(fq)], [str(m1), str(m2)]):
        runs = {}
        for hooked in (False, True):
            env = dict(os.environ)
            env.pop("DCN_CLI_CLASSIFY_BATCH_BASES", None)
            if hooked:
                env["DCN_CLI_CLASSIFY_BATCH_BASES"] = str(hook)
            tsv, summ = tmp_path / f"per_read{hooked}.tsv", tmp_path / f"summary{hooked}.json"
            subprocess.run([CLI, "classify", *x, *inputs, *flags, "--per-read", str(tsv), "-s", str(summ), "-q"],
                           check=True, capture_output=True, timeout=300, env=env)
            runs[hooked] = (open(tsv).read().splitlines(), json.load(open(summ)))
        assert len(runs[True][0]) == len(reads) // (len(inputs)) + 1
        assert runs[True][0] == runs[False][0]
        rows = [ln.split("\t") for ln in runs[True][0][1:]]
        js = runs[True][1]
        assert js["seqs_in"] == len(reads) and js["bp_in"] == sum(len(r) for r in reads)
        for j, p in enumerate(idx):
            out1, s1 = tmp_path / f"keep{j}.fq", tmp_path / f"keep{j}.json"
            cmd = [CLI, "filter", p, *inputs, *flags, "-o", str(out1), "-s", str(s1), "-q"]
            if len(inputs) == 2:
                cmd += ["-O", str(tmp_path / f"keep{j}_2.fq")]
            subprocess.run(cmd, check=True, capture_output=True, timeout=300)
            matched = {r[0] for r in rows if f"ref{j}" in r[-1].split(",")}
            assert matched == set(_kept_ids(out1)), j
            fj, ij = json.load(open(s1)), js["indexes"][j]
            assert ij["seqs_matched"] == fj["seqs_out"] and ij["bp_matched"] == fj["bp_out"]

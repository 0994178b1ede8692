"""The seams of the depth track kernels (track.hip) with every key and every depth placed base by base, in the
construction of tests/test_gpu_locate_seams.py: at w = 1 every position 0 .. len - k of an A/C/G/T read is a minimizer
position, a read is a slice of its own of a random genome, the set holds the hashes at chosen positions, and a chosen
depth d is placed exactly by classifying d copies of the k-mer as reads of k bases (each adds 1).  Reads shorter than k
in front of a read put its first base at a chosen residue mod 32 of the batch-absolute position bitmap.  Expectations are
the model of tests/_depth_track_worker.py over the oracle's hashes.  Integers only, no tolerance."""
import numpy as np
import pytest

import _depth_worker as DW
from _depth_track_worker import SAT, Model, assert_track
from test_gpu_locate_seams import MODS, Genome
from test_gpu_classify_seams import W as WIN15, displaced_members

pytestmark = pytest.mark.gpu

K = 31
LANE_BASES = 1024   # DCN_TRK_LANE_BASES: a read whose widest bin is wider goes to the wave kernel
PIECE_BASES = 8192  # DCN_TRK_PIECE_BASES: a wide bin is cut into pieces of this many bases, a wave each
CTX_BASES = 1 << 20


class Plan:
    """reads with planned keys {position: (label, depth)}, each read a slice of its own of the genome"""

    def __init__(self, oracle, genome, n_members):
        self.oracle, self.g, self.k, self.n_members = oracle, genome, genome.k, n_members
        self.reads, self.start = [], []
        self.cursor = 0  # of the genome
        self.o = 0       # of the batch: the first base of the next read
        self.label, self.depth, self.at = {}, {}, {}  # hash -> label, depth, a genome position of the k-mer
        self.set = None

    def pad(self, mod):
        n = (mod - self.o) % 32
        while n:
            take = min(n, self.k - 1)
            self._push((b"ACGT" * 8)[:take])
            n -= take

    def _push(self, read):
        self.reads.append(read)
        self.start.append(self.o)
        self.o += len(read)
        return len(self.reads) - 1

    def add(self, length, keys):
        a = self.cursor
        self.cursor += length
        assert self.cursor <= len(self.g.seq) and self.set is None
        for p, (lab, d) in keys.items():
            assert 0 <= p <= length - self.k and 0 < lab < (1 << self.n_members) and 0 <= d <= SAT
            h = int(self.g.hashes[a + p])
            self.label[h] = self.label.get(h, 0) | lab
            self.depth[h] = self.depth.get(h, 0) + d  # (a k-mer that repeats in the genome: its depths add up, as they will)
            self.at[h] = a + p
        return self._push(self.g.seq[a:a + length])

    def mkeys(self):
        return [np.array(sorted(h for h, lab in self.label.items() if lab >> j & 1), np.uint64) for j in range(self.n_members)]

    def build(self, dcn):
        """the set, with every planned depth placed by k-mer reads"""
        self.set = dcn.IndexSet([dcn.Index.from_keys(m, self.k, 1) for m in self.mkeys()])
        self.set.enable_depth()
        hs = [h for h, d in self.depth.items() if d]
        starts = np.repeat(np.array([self.at[h] for h in hs], np.int64), [self.depth[h] for h in hs])
        seq = np.frombuffer(self.g.seq, np.uint8)
        per = CTX_BASES // self.k
        clf = dcn.Classifier(self.set, max_batch_bases=CTX_BASES, max_batch_reads=per + 1)
        for i in range(0, len(starts), per):
            st = starts[i:i + per]
            bases = seq[st[:, None] + np.arange(self.k)[None, :]].ravel()
            _, _, total = clf.classify_batch(bases, np.arange(len(st) + 1, dtype=np.uint64) * self.k)
            assert (total == 1).all()
        clf.close()
        got = dict(zip(*[a.tolist() for a in self.set.depth_keys()]))
        assert got == {h: min(d, SAT) for h, d in self.depth.items() if d}  # the construction holds
        return self.set

    def model(self):
        return Model(self.oracle, self.reads, self.k, 1, self.mkeys(), self.depth)

    def tracker(self, dcn, **kw):
        return dcn.DepthTracker(self.set, max_batch_bases=CTX_BASES, max_batch_reads=len(self.reads) + 1, **kw)


def check(dcn, oracle, s, model, reads, bin_bases, mask=None, n_members=3, cap=0, what=()):
    b, o = oracle.concat_reads(reads)
    mask = (1 << n_members) - 1 if mask is None else mask
    t = dcn.DepthTracker(s, max_batch_bases=CTX_BASES, max_batch_reads=len(reads) + 1, bin_bases=bin_bases,
                         member=[j for j in range(n_members) if mask >> j & 1], depth_cap=cap)
    try:
        got = t.track_batch(b, o)
    finally:
        t.close()
    want = model.bins(bin_bases, mask, cap)
    assert_track(got, want, (bin_bases, mask, cap) + tuple(what))
    return want


def dense(length, k):
    """a key at almost every position, with depths that differ between neighbours: every fifth position is no key, every
    eleventh key unobserved, labels in turn; the first and the last position are observed keys"""
    keys = {}
    for p in range(length - k + 1):
        if p % 5 == 3:
            continue
        keys[p] = (1 + p % 3 if p % 3 else 7, 0 if p % 11 == 0 else 1 + p % 7)
    keys[0] = (1, 5)
    keys[length - k] = (2, 6)
    return keys


def sparse(length, k, edges):
    """keys on both sides of every edge and at the read's first and last position, and a thin cover between"""
    keys = {p: (1 + p % 3, 1 + p % 5) for p in range(0, length - k + 1, 97)}
    for e in edges:
        for p in (e - 1, e, e + 1):
            if 0 <= p <= length - k:
                keys[p] = (1 + p % 3, 2 + p % 7)
    keys[0] = (1, 5)
    keys[length - k] = (2, 6)
    return keys


@pytest.fixture(scope="module")
def g31(oracle):
    g = Genome(oracle, K, 120_000, 31)
    assert g.distinct  # the construction's condition
    return g


@pytest.fixture(scope="module")
def edges_plan(oracle, dcn, g31):
    """per residue of the first base: dense reads of 2,100 bases (bins of 1 .. 1,025 bases and one bin), dense reads on
    either side of the lane path's limit, a read of exactly k bases, and a 20,000-base read with keys around every piece
    edge of bin_bases 0 and 17,000"""
    p = Plan(oracle, g31, 3)
    for mod in MODS:
        p.pad(mod)
        p.add(2100, dense(2100, K))
        for length in (LANE_BASES - 1, LANE_BASES, LANE_BASES + 1):
            p.pad(mod)
            p.add(length, dense(length, K))
        p.pad(mod)
        p.add(K, {0: (4, 3)})
        p.pad(mod)
        pieces = [j * PIECE_BASES for j in range(1, 3)] + [17_000, 17_000 + PIECE_BASES] + [j * 1025 for j in range(1, 19)]
        p.add(20_000, sparse(20_000, K, pieces))
    p.build(dcn)
    return p, p.model()


@pytest.mark.parametrize("bin_bases", [1, 31, 32, 33, 1000, LANE_BASES - 1, LANE_BASES, LANE_BASES + 1, 0, 17_000, 2 * PIECE_BASES,
                                       2 * PIECE_BASES + 1])
def test_bin_edges_and_the_path_switch(oracle, dcn, edges_plan, bin_bases):
    """bins that end mid-word, at a word edge, as the short last bin of a read and at its last position, with keys of
    distinct depths on both sides; bins of the lane path's limit, one less and one more; wide bins of one, two and three
    pieces with keys in the first and last base of each piece; one bin over a read of 625 bitmap words"""
    p, model = edges_plan
    assert sorted(s & 31 for s, r in zip(p.start, p.reads) if len(r) >= K) == sorted(MODS * 6)
    want = check(dcn, oracle, p.set, model, p.reads, bin_bases)
    bo, w = want
    assert w["max_depth"].max() == 8 and (w["n_keys"] > w["n_observed"]).any() and (w["n_positions"] > w["n_keys"]).any()
    for mask in (1, 2, 4, 6):
        check(dcn, oracle, p.set, model, p.reads, bin_bases, mask)
    check(dcn, oracle, p.set, model, p.reads, bin_bases, cap=3)
    if bin_bases and bin_bases <= 33:  # both sides of an edge differ, so a position in the wrong bin shows
        r = next(i for i, x in enumerate(p.reads) if len(x) == 2100)
        sums = w["sum_depth"][int(bo[r]):int(bo[r + 1])]
        assert len(sums) == -(-2100 // bin_bases) and len(set(sums[:8].tolist())) > 1


def test_reads_sharing_a_word(oracle, dcn):
    """k = 15: reads of 15 .. 40 bases, two or three to a bitmap word, every position a key; bins of 1, 4, 7 and 16 bases
    put three and more bins into one word, and a read of exactly k bases has one position"""
    k = 15
    g = Genome(oracle, k, 30_000, 15)
    rng = np.random.default_rng(815)
    p = Plan(oracle, g, 2)
    for i in range(600):
        length = k if i % 7 == 0 else int(rng.integers(k, 41))
        p.add(length, {q: (1 + (q + i) % 3 if (q + i) % 3 else 3, (q + i) % 6) for q in range(length - k + 1)})
        if i % 50 == 0:
            p._push(b"")
    p.build(dcn)
    model = p.model()
    words = {}
    for s, r in zip(p.start, p.reads):
        if len(r) >= k:
            words.setdefault(s >> 5, []).append(s)
    assert sum(1 for v in words.values() if len(v) >= 2) > 100
    for B in (1, 4, 7, 16, 0):
        for mask in (3, 1, 2):
            check(dcn, oracle, p.set, model, p.reads, B, mask, n_members=2)


def test_extreme_values(oracle, dcn):
    """sum_depth past 2^32 in one bin: a sequence of period 5 has five k-mers, each driven past 65,535 by 340 reads of 1,000
    bases of it; a 70,000-base stretch then holds 69,970 positions of saturated keys (69,970 * 65,535 > 2^32), every full
    piece of it sums to 8,192 * 65,535.  One more key is driven to 65,534 and then to 65,535 by the k-mer recipe of
    tests/_depth_worker.py: max_depth and depth_cap at those two values."""
    unit = b"ACGGT"
    rep = unit * 14_000
    hot = DW.random_reads(np.random.default_rng(816), 1, 200, 200)[0]
    hot_kmer = hot[50:50 + K]
    o = oracle.Index.build([rep[:1000], hot_kmer], k=K, w=1)
    mkeys = [set(o.keys().tolist())]
    hot_key = int(oracle.minimizer_hashes_and_positions(hot_kmer, K, 1)[0][0])
    assert 2 <= len(mkeys[0]) <= 6 and hot_key in mkeys[0]
    s = dcn.IndexSet([dcn.Index.from_keys(o.keys(), K, 1)])
    s.enable_depth()
    clf = dcn.Classifier(s, max_batch_bases=1 << 22, max_batch_reads=1 << 17)
    soak = [rep[:1000]] * 340
    DW.classify(oracle, clf, soak)
    depth = DW.occurrences(oracle, soak, K, 1)
    assert min(depth.values()) > SAT

    def send_hot(n):
        bases = np.tile(np.frombuffer(hot_kmer, np.uint8), n)
        clf.classify_batch(bases, np.arange(n + 1, dtype=np.uint64) * K)
        depth[hot_key] += n

    send_hot(SAT - 1)
    reads = [rep[:70_000], hot, rep[:LANE_BASES], rep[:2 * PIECE_BASES + K - 1]]
    for step in range(2):
        model = Model(oracle, reads, K, 1, mkeys, depth)
        for B in (0, LANE_BASES, 40_000):
            bo, w = check(dcn, oracle, s, model, reads, B, n_members=1)
            if B == 0:
                assert w["n_keys"][0] == 69_970 and w["sum_depth"][0] == 69_970 * SAT > 1 << 32
                assert w["max_depth"].tolist() == [SAT, SAT - 1 + step, SAT, SAT]
                assert w["sum_depth"][3] == 2 * PIECE_BASES * SAT  # two full pieces
            for cap in (SAT - 1, SAT):
                bo, c = check(dcn, oracle, s, model, reads, B, n_members=1, cap=cap)
                if B == 0:
                    assert c["max_depth"].tolist() == [cap, SAT - 1 + (step if cap == SAT else 0), cap, cap]
                    assert c["sum_depth"][0] == 69_970 * cap > 1 << 32
        send_hot(1)
    clf.close()


def test_displaced_slots(oracle, dcn, monkeypatch):
    """the half-full table of test_member_labels_in_displaced_slots as a set with depth: the targets sit in the second slot
    of a group, in a displaced group, in group 0 after the last; the home slots hold member 0's fillers, whose depth is 0,
    so a depth read from the home slot shows"""
    monkeypatch.setenv("DCN_TABLE_SLOTS_PER_KEY", "2")
    k, G, members, targets, reads = displaced_members(oracle)
    s = dcn.IndexSet([dcn.Index.from_keys(m, k, WIN15) for m in members])
    s.enable_depth()
    soak = [r for i, r in enumerate(reads) for _ in range(1 + i % 5)]
    clf = dcn.Classifier(s, max_batch_bases=CTX_BASES, max_batch_reads=1 << 12)
    DW.classify(oracle, clf, soak)
    clf.close()
    depth = DW.occurrences(oracle, soak, k, WIN15)
    model = Model(oracle, reads, k, WIN15, members, depth)

    def run(B, mask):
        b, o = oracle.concat_reads(reads)
        t = dcn.DepthTracker(s, max_batch_bases=CTX_BASES, max_batch_reads=len(reads) + 1, bin_bases=B,
                             member=[j for j in range(3) if mask >> j & 1])
        got = t.track_batch(b, o)
        t.close()
        want = model.bins(B, mask)
        assert_track(got, want, (B, mask))
        return want[1]

    w = run(0, 7)
    assert (w["n_positions"] == 1).all() and int(w["n_keys"].sum()) == 4 * len(targets)
    assert int(w["n_observed"].sum()) == 4 * len(targets) and sorted(set(w["max_depth"].tolist())) == [0, 1, 2, 3, 4, 5]
    for mask in (1, 2, 4, 6):
        run(0, mask)
    run(16, 7)


@pytest.mark.parametrize("n_reads", [2047, 2048, 2049, 4097])
def test_many_reads_and_bins(oracle, dcn, edges_plan, n_reads):
    """one bin per read over 2,047 .. 4,097 reads, empty ones among them (no bin at all when bin_bases is not 0), and one
    batch of more than 65,537 bins; the reads are cut from the stretch of the genome that holds the plan's keys"""
    p, _ = edges_plan
    rng = np.random.default_rng(n_reads)
    reads = []
    for i in range(n_reads):
        if i % 97 == 5:
            reads.append(b"")
            continue
        a = int(rng.integers(0, p.cursor - 64))
        reads.append(p.g.seq[a:a + int(rng.integers(K - 2, 60))])
    model = Model(oracle, reads, K, 1, p.mkeys(), p.depth)
    w = check(dcn, oracle, p.set, model, reads, 0)
    assert len(w[1]["n_keys"]) == n_reads and w[1]["n_keys"].sum() > n_reads and w[1]["n_observed"].sum() > n_reads // 2
    check(dcn, oracle, p.set, model, reads, 16, mask=5)
    if n_reads == 4097:
        w = check(dcn, oracle, p.set, model, reads, 1)
        assert len(w[1]["n_keys"]) >= 65_537
        check(dcn, oracle, p.set, model, reads, 2, mask=2)

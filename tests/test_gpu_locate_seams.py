"""The seams of locate (locate.hip, locate_api.hip) with every hit placed base by base: gap equality on the lane and the
wave path, the segment carried from one 64-word iteration of the wave kernel to the next, min_hits at its edges, 64
segments in an iteration and none, reads that share a bitmap word, saturation of k + max_gap, labels across lanes and
iterations, the scan over reads and the growth of the segment buffer, and locate's own table probe under displacement.
Integers only, no tolerance.

The construction: at w = 1 every k-mer is its own window, so every position 0 .. len - k of an A/C/G/T read is a
minimizer position.  A read is a slice of a random genome G whose k-mer hashes are all distinct (asserted), the index
holds the hashes at the planned positions, so the read's hit bitmap is exactly the plan; every read has a slice of its
own.  The expected segments are the statement of include/deacon_hip.h (segments_of) applied to the hits that the
oracle's hashes of the read and the key set give; for k >= 31 these hits are asserted to be the plan first.

The hit bitmap is batch-absolute: bit o0 + p for position p of a read that starts at base o0 of the batch.  Reads
shorter than k (no window) in front of a read put o0 at a chosen residue mod 32, and Batch.pos(word, bit) is the read
position whose bit is `bit` of bitmap word (o0 >> 5) + word: word 0 is lane 0 of the wave kernel's first iteration, word
63 its lane 63, word 64 lane 0 of the second iteration."""
import numpy as np
import pytest

from conftest import random_reads
from test_classify_replicas import group_of
from test_gpu_classify_seams import W, displaced_members, group_slots

pytestmark = pytest.mark.gpu

K = 31
LANE_BASES = 1024          # DCN_LOC_LANE_BASES: longer reads go to the wave kernel when k + max_gap >= 31
ITER_WORDS = 64            # bitmap words per iteration of the wave kernel (2,048 bases)
SCAN_BLOCK = 2048          # DCN_SCAN_BLOCK: reads per block of the scan over reads
SCAN_THREADS = 256         # DCN_LOC_THREADS: locate_scan_blocks_kernel takes ceil(blocks / 256) blocks per thread
SEG_BUFFER = 1 << 16       # a context's first device segment buffer (grow_segments)
MODS = (0, 1, 31)          # o0 mod 32 of the reads under test
ALL = 0xFFFFFFFF


class Genome:
    """a random sequence with the hash of its every k-mer (w = 1)"""

    def __init__(self, oracle, k, n, seed):
        self.k = k
        self.seq = random_reads(np.random.default_rng(seed), 1, n, n)[0]
        self.hashes, pos = oracle.minimizer_hashes_and_positions(self.seq, k, 1)
        assert np.array_equal(pos, np.arange(n - k + 1))
        self.distinct = len(np.unique(self.hashes)) == len(self.hashes) and bool((self.hashes != 0).all())


@pytest.fixture(scope="module")
def g31(oracle):
    g = Genome(oracle, K, 800_000, 31)
    assert g.distinct  # the construction's condition
    return g


@pytest.fixture(scope="module")
def g15(oracle):
    return Genome(oracle, 15, 60_000, 15)  # (some 15-mers repeat: expectations come from the oracle's hashes alone)


def segments_of(hits, k, max_gap, min_hits):
    """include/deacon_hip.h over {position: label}: ascending, a hit joins when p - last <= k + max_gap, end = last + k,
    segments below min_hits dropped"""
    segs = []
    for p in sorted(hits):
        if segs and p - segs[-1][1] <= k + max_gap:
            s = segs[-1]
            segs[-1] = (s[0], p, s[2] + 1, s[3] | hits[p])
        else:
            segs.append((p, p, 1, hits[p]))
    return [(s, l + k, n, m) for (s, l, n, m) in segs if n >= min_hits]


class Batch:
    """reads with planned hits, each a slice of its own of the genome; n_members = 0: a plain index (labels are 1)"""

    def __init__(self, oracle, genome, n_members=0):
        self.oracle, self.g, self.k, self.n_members = oracle, genome, genome.k, n_members
        self.reads, self.plan, self.start = [], [], []
        self.cursor = 0  # of the genome
        self.o = 0       # of the batch: o0 of the next read
        self.label = {}  # hash -> label
        self._index = self._hits = None

    def pad(self, mod):
        """reads without a window in front, so that the next read's o0 mod 32 is mod"""
        n = (mod - self.o) % 32
        while n:
            take = min(n, self.k - 1)
            self._push((b"ACGT" * 8)[:take], None)
            n -= take

    def pos(self, word, bit):
        return word * 32 + bit - (self.o & 31)

    def word_of(self, r, p):
        """the bitmap word of position p of read r, counted from the read's first word"""
        return ((self.start[r] + p) >> 5) - (self.start[r] >> 5)

    def _push(self, read, plan):
        self.reads.append(read)
        self.plan.append(plan)
        self.start.append(self.o)
        self.o += len(read)
        return len(self.reads) - 1

    def add(self, length, hits):
        """a read of `length` bases that hits at `hits`: positions (label 1) or {position: label}"""
        hits = dict(hits) if isinstance(hits, dict) else {int(p): 1 for p in hits}
        a = self.cursor
        self.cursor += length
        assert self.cursor <= len(self.g.seq) and self._index is None
        for p, lab in hits.items():
            assert 0 <= p <= length - self.k and 0 < lab < (1 << max(self.n_members, 1)), (p, length, lab)
            h = int(self.g.hashes[a + p])
            self.label[h] = self.label.get(h, 0) | lab
        return self._push(self.g.seq[a:a + length], hits)

    def index(self, dcn):
        if self._index is None:
            keys = lambda j: np.array(sorted(h for h, lab in self.label.items() if lab >> j & 1), np.uint64)
            if self.n_members:
                self._index = dcn.IndexSet([dcn.Index.from_keys(keys(j), self.k, 1) for j in range(self.n_members)])
            else:
                self._index = dcn.Index.from_keys(keys(0), self.k, 1)
        return self._index

    def hits(self):
        """per read {position: label}, from the oracle's hashes of the read and the key set"""
        if self._hits is None:
            keys = np.array(sorted(self.label), np.uint64)
            self._hits = []
            for read, plan in zip(self.reads, self.plan):
                h, p = self.oracle.minimizer_hashes_and_positions(read, self.k, 1)
                assert len(p) == max(len(read) - self.k + 1, 0)
                m = np.isin(h, keys)
                got = {int(q): self.label[int(x)] for x, q in zip(h[m], p[m])}
                if self.g.distinct:
                    assert got == (plan or {})  # the construction did not degenerate
                self._hits.append(got)
        return self._hits

    def expect(self, max_gap, min_hits=1, member_mask=ALL):
        out = []
        for hits in self.hits():
            masked = {p: lab & member_mask for p, lab in hits.items() if lab & member_mask}
            out.append(segments_of(masked, self.k, max_gap, min_hits))
        return out

    def locate(self, dcn, max_gap, min_hits=1, member_mask=ALL):
        bases, offsets = self.oracle.concat_reads(self.reads)
        assert offsets[:-1].tolist() == self.start
        loc = dcn.Locator(self.index(dcn), max_gap=max_gap, min_hits=min_hits, member_mask=member_mask,
                          max_batch_bases=len(bases) + 64, max_batch_reads=len(self.reads) + 1)
        so, segs = loc.locate_batch(bases, offsets)
        loc.close()
        assert len(so) == len(self.reads) + 1 and so[0] == 0 and int(so[-1]) == len(segs)
        rows = segs.tolist()
        return [[tuple(s) for s in rows[int(so[r]):int(so[r + 1])]] for r in range(len(self.reads))]

    def check(self, dcn, max_gap, min_hits=1, member_mask=ALL):
        want = self.expect(max_gap, min_hits, member_mask)
        got = self.locate(dcn, max_gap, min_hits, member_mask)
        assert len(got) == len(want)
        for r, (g, w) in enumerate(zip(got, want)):
            assert g == w, (max_gap, min_hits, member_mask, r, self.start[r] & 31, len(self.reads[r]), g[:4], w[:4])
        return got


# ---- 1. gap equality on both paths ---------------------------------------------------------------------------------------
# (word, bit) of the first hit of a pair; the second one is k + max_gap (one segment) or one more (two) after it
ANCHORS = ((0, 31), (1, 0), (1, 3), (1, 5), (2, 31), (30, 9), (62, 17), (63, 0), (63, 31))


@pytest.mark.parametrize("max_gap", [0, 1, 29, 2017, 5000, 9000])
def test_gap_equality(oracle, dcn, g31, max_gap):
    """max_gap 0: pairs inside one word (bits 0 and 31), in adjacent words, across word 63 -> 64; 2,017: join = 2,048, the
    same lane of the next iteration; 5,000 and 9,000: one and three (or more) wholly empty iterations between the two"""
    join = K + max_gap
    b = Batch(oracle, g31)
    cases = {}
    for mod in MODS:
        for length in (1000, 1023, 1024, 1025, 9000, 12000):
            if length == 12000 and join < 8000:
                continue
            for a, (word, bit) in enumerate(ANCHORS):
                for delta in (0, 1):
                    b.pad(mod)
                    p = b.pos(word, bit)
                    q = p + join + delta
                    if q <= length - K:
                        cases[mod, length, a, delta] = (b.add(length, [p, q]), p, q)
    want = b.expect(max_gap)
    same_word = seam = empty_between = lane = wave = 0
    for (mod, length, a, delta), (r, p, q) in cases.items():
        assert want[r] == ([(p, q + K, 2, 1)] if delta == 0 else [(p, p + K, 1, 1), (q, q + K, 1, 1)])
        wp, wq = b.word_of(r, p), b.word_of(r, q)
        assert wp == ANCHORS[a][0]
        same_word += wp == wq
        seam += wp == ITER_WORDS - 1 and wq == ITER_WORDS
        empty_between = max(empty_between, wq // ITER_WORDS - wp // ITER_WORDS - 1)
        lane += length <= LANE_BASES
        wave += length > LANE_BASES
    assert wave >= 12
    if max_gap == 0:
        assert same_word >= 6 and seam >= 6
    if join <= 60:
        assert lane >= 30 and seam >= 3
    if max_gap == 2017:
        assert all(b.word_of(r, q) - b.word_of(r, p) in (ITER_WORDS, ITER_WORDS + 1) for r, p, q in cases.values())
    if max_gap == 5000:
        assert empty_between >= 1
    if max_gap == 9000:
        assert empty_between >= 3
    got = b.check(dcn, max_gap)
    for (mod, length, a, delta), (r, p, q) in cases.items():  # the same pattern on either side of the threshold
        if length == 1024 and (mod, 1023, a, delta) in cases:
            assert got[r] == got[cases[mod, 1023, a, delta][0]] == got[cases[mod, 1025, a, delta][0]]


@pytest.mark.parametrize("max_gap", [15, 16])
def test_gap_equality_small_k(oracle, dcn, g15, max_gap):
    """k = 15: join 30 sends every read to the bit walk (a word may hold hits of two segments), join 31 sends the
    3,000-base read to the wave kernel; pairs 30, 31 and 32 apart inside a word and across two"""
    k = 15
    join = k + max_gap
    b = Batch(oracle, g15)
    pairs = [(bit, d) for bit in (0, 1, 10, 31) for d in (30, 31, 32)]
    cases = []
    for mod in MODS:
        for length in (3000, 1000):
            b.pad(mod)
            hits = []
            for i, (bit, d) in enumerate(pairs):
                p = b.pos(2 + 4 * i, bit)  # (pairs 128 bases apart: never joined to one another)
                if p + d <= length - k:
                    hits += [p, p + d]
            cases.append((b.add(length, hits), len(hits) // 2, sum(1 for x, y in zip(hits[::2], hits[1::2]) if y - x > join)))
    want = b.expect(max_gap)
    for r, n_pairs, n_split in cases:
        assert len(want[r]) == n_pairs + n_split and n_pairs >= 7
        assert sum(n for (_, _, n, _) in want[r]) == 2 * n_pairs
    assert cases[0][1] == len(pairs) and cases[0][2] == (8 if max_gap == 15 else 4)
    b.check(dcn, max_gap)
    b.check(dcn, max_gap, min_hits=2)


# ---- 2. the carried segment ----------------------------------------------------------------------------------------------
def _carried_patterns(b, length):
    last = length - K
    return {
        # hits in every one of the first four iterations, and on both sides of every seam between them
        "every iteration": [b.pos(w, 7) for w in (10, 40, 63, 64, 100, 127, 128, 190, 191, 192, 255)],
        # a segment closed inside iteration 0; one left open there (words 60, 61), iteration 1 empty, closed by a head in
        # lane 5 of iteration 2, which three more segments follow; iteration 3 empty; one more in iteration 4 (words
        # 256 .. 281 of a 9,000-base read: its fifth and last iteration)
        "closed by a later head": [b.pos(w, 11) for w in (3, 4, 60, 61, 133, 134, 140, 150, 151, 170, 260)],
        "lane 63 only": [b.pos(w, 31) for w in (63, 127, 191)] + [b.pos(63, 0)],
        "lane 0 only": [b.pos(w, 0) for w in (64, 128, 192)] + [b.pos(192, 31)],
        "across the seam": [b.pos(63, 31), b.pos(64, 0), b.pos(127, 0), b.pos(128, 31)],
        "first and last position": [0, last],
        "first and last two": [0, 1, last - 1, last],
        "open at the end": [b.pos(10, 3), b.pos(250, 3), last - 40, last - 3, last],
    }


def test_carried_segment(oracle, dcn, g31):
    b = Batch(oracle, g31)
    rows = {}
    for mod in MODS:
        for length in (9000, 9024 - mod):  # (the second one ends at a word's end: its last word is whole)
            b.pad(mod)
            for name, hits in _carried_patterns(b, length).items():
                b.pad(mod)
                rows[mod, length, name] = b.add(length, hits)
    assert any((b.start[r] + len(b.reads[r])) % 32 == 0 for r in rows.values())
    assert any((b.start[r] + len(b.reads[r])) % 32 != 0 for r in rows.values())
    # what the cases aim at, on the model
    w29, w5000 = b.expect(29), b.expect(5000)
    for (mod, length, name), r in rows.items():
        if name == "every iteration":
            assert len(w5000[r]) == 1 and w5000[r][0][2] == 11
            assert [n for (_, _, n, _) in w29[r]] == [1, 1, 2, 1, 2, 3, 1]
        if name == "closed by a later head":
            assert [n for (_, _, n, _) in w29[r]] == [2, 2, 2, 1, 2, 1, 1]
        if name == "first and last position":
            assert w29[r] == [(0, K, 1, 1), (length - K, length, 1, 1)]
        if name == "open at the end":
            assert w29[r][-1] == (length - K - 40, length, 3, 1)
    for max_gap in (0, 29, 2017, 5000):
        for min_hits in (1, 2):
            b.check(dcn, max_gap, min_hits)


# ---- 3. min_hits at its edges ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [2, 3, 5])
def test_min_hits_edges(oracle, dcn, g31, m):
    """segments of m - 1 and of m hits (hits 32 apart, max_gap 29) in every place where the kernels decide on min_hits"""
    b = Batch(oracle, g31)
    run = lambda w0, n, bit=7: [b.pos(w0 + i, bit) for i in range(n)]
    pairs = []
    for mod in MODS:
        for n in (m - 1, m):
            rs = []
            b.pad(mod)  # (pos() below is of a read at this residue; every read of the loop is put there)
            for length, hits in (
                # wholly inside an iteration, between two segments that stay
                (9000, run(2, m) + run(20, n) + run(40, m)),
                # carried with m - 1 hits and completed (n = m) or not (n = m - 1) by lane 0 of the next iteration;
                # closed by a head there, and the segments after it land in consecutive slots
                (9000, run(2, m) + run(64 - (m - 1), n) + run(70, m) + run(90, m) + run(110, m - 1) + run(120, m)),
                # the same without a segment before it, closed two iterations later by a head in lane 9
                (9000, run(64 - (m - 1), n) + run(137, m) + run(150, m)),
                # the last segment of the read
                (9000, run(2, m) + [9000 - K - 32 * i for i in range(n)]),
                (9000, run(100, m) + run(272, n, 0)),
                # the lane path
                (1000, run(2, n) + run(12, m) + [1000 - K - 32 * i for i in range(n)]),
            ):
                b.pad(mod)
                rs.append(b.add(length, hits))
            pairs.append(rs)
    want = b.expect(29, m)
    for short, full in zip(pairs[0::2], pairs[1::2]):  # n = m - 1 beside n = m
        for case, (r0, r1) in enumerate(zip(short, full)):
            assert len(want[r1]) - len(want[r0]) == (2 if case == 5 else 1)
            assert all(n >= m for (_, _, n, _) in want[r0] + want[r1])
    b.check(dcn, 29, m)
    b.check(dcn, 29, 1)
    b.check(dcn, 29, m - 1)
    b.check(dcn, 29, m + 1)


# ---- 4. many segments per iteration, and none ------------------------------------------------------------------------------
def test_many_segments_and_none(oracle, dcn, g31):
    b = Batch(oracle, g31)
    rows = {}
    for mod in MODS:
        b.pad(mod)
        for name, length, hits in (
            ("every 32", 9000, range(32 - mod, 9000 - K + 1, 32)),  # one hit in every word but the first
            ("every 33", 9000, range(5, 9000 - K + 1, 33)),
            ("every position", 9000, range(9000 - K + 1)),
            ("every 33", 1000, range(5, 1000 - K + 1, 33)),
            ("every position", 1000, range(1000 - K + 1)),
            ("before none", 9000, [b.pos(3, 3), 9000 - K]),
            ("none", 9000, []),
            ("after none", 9000, [0, 8960]),
        ):
            if name != "none" and name != "after none":
                b.pad(mod)
            rows[mod, name, length] = b.add(length, hits)
    w0, w1, w2 = b.expect(0), b.expect(1), b.expect(2)
    for (mod, name, length), r in rows.items():
        n = len(b.plan[r])
        if name == "every 32":
            assert len(w0[r]) == n >= 280 and len(w1[r]) == 1
            in_iteration = [s for (s, _, _, _) in w0[r] if b.word_of(r, s) // ITER_WORDS == 1]
            assert len(in_iteration) == 64  # every lane starts a segment
        if name == "every 33":
            assert len(w0[r]) == len(w1[r]) == n and w2[r] == [(5, 5 + 33 * (n - 1) + K, n, 1)]
        if name == "every position":
            assert w0[r] == [(0, length, length - K + 1, 1)]
        if name == "none":
            assert w0[r] == [] and w0[r - 1] and w0[r + 1]
    for max_gap in (0, 1, 2):
        b.check(dcn, max_gap)
    b.check(dcn, 0, 2)
    b.check(dcn, 2, 2)


# ---- 5. neighbours in one bitmap word --------------------------------------------------------------------------------------
def test_neighbours_share_bitmap_words(oracle, dcn, g31):
    """every read hits in its last window and at its position 0, with no read without a window between them: the lengths
    (31 .. 62 and 1,025 .. 1,056) put the boundaries at chosen bits of a word, bit 31 among them, where the last hit of a
    read and the first of the next lie in one word"""
    b = Batch(oracle, g31)
    residues = (31, 0, 1, 31, 16, 31, 7, 0, 30, 31)
    for i in range(150):
        base = 1025 if i % 3 == 2 else K
        length = base + (residues[i % len(residues)] - (b.o + base)) % 32
        assert K <= length <= 70 or 1025 <= length <= 1090
        b.add(length, [0, length - K])
    shared = [r for r in range(1, len(b.reads)) if b.start[r] & 31 == 31]
    assert sum(len(b.reads[r]) > LANE_BASES for r in shared) >= 5 and sum(len(b.reads[r]) <= LANE_BASES for r in shared) >= 10
    assert {b.start[r] & 31 for r in range(len(b.reads))} >= {0, 1, 7, 16, 30, 31}
    want = b.expect(0)
    for r, w in enumerate(want):
        n = len(b.reads[r])
        assert w == ([(0, K, 1, 1)] if n == K else [(0, n, 2, 1)] if n <= 2 * K else [(0, K, 1, 1), (n - K, n, 1, 1)])
    assert all(w == [(0, len(rd), 1 + (len(rd) > K), 1)] for w, rd in zip(b.expect(ALL), b.reads))
    b.check(dcn, 0)
    b.check(dcn, ALL)


# ---- 6. saturation of k + max_gap ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_gap", [0xFFFFFFFF, 0xFFFFFFF0])
def test_join_saturates(oracle, dcn, g31, max_gap):
    b = Batch(oracle, g31)
    rows = []
    for mod in MODS:
        for length in (1000, 1025, 9000):
            b.pad(mod)
            hits = [b.pos(w, 3 + w % 5) for w in (1, 5, 9, 20, 29, 63, 64, 130, 270) if b.pos(w, 7) <= length - K]
            rows.append(b.add(length, hits))
        b.add(2000, [])
    for r, w in enumerate(b.expect(max_gap)):
        plan = b.plan[r]
        if plan:
            assert min(y - x for x, y in zip(sorted(plan), sorted(plan)[1:])) > K  # (apart at any join that wrapped)
            assert w == [(min(plan), max(plan) + K, len(plan), 1)]
        else:
            assert w == []
    b.check(dcn, max_gap)
    b.check(dcn, max_gap, min_hits=5)


# ---- 7. labels across lanes and iterations -----------------------------------------------------------------------------------
def test_labels_across_lanes_and_iterations(oracle, dcn, g31):
    b = Batch(oracle, g31, n_members=3)
    rows = {}
    for mod in MODS:
        for length, scale in ((9000, 1), (1000, 0)):
            b.pad(mod)
            w = (lambda big, small: big if scale else small)
            # labels 1, 2, 4 and a key of members 0 and 1, each in an iteration of its own (in the short read: a word)
            rows[mod, length, "spread"] = b.add(length, {b.pos(w(10, 2), 7): 1, b.pos(w(70, 9), 7): 2,
                                                          b.pos(w(140, 17), 7): 4, b.pos(w(200, 25), 7): 3})
            b.pad(mod)
            # members 0 and 1 in turn, 40 apart: masking one of them leaves hits 80 apart
            rows[mod, length, "in turn"] = b.add(length, {p: 1 + (i & 1) for i, p in enumerate(range(100, length - 100, 40))})
            b.pad(mod)
            # several labels inside one word, in adjacent lanes, and on both sides of a seam between iterations
            rows[mod, length, "close"] = b.add(length, {b.pos(w(66, 6), 1): 1, b.pos(w(66, 6), 9): 4, b.pos(w(67, 7), 0): 2,
                                                         b.pos(w(127, 20), 31): 4, b.pos(w(128, 21), 0): 1,
                                                         b.pos(w(191, 25), 30): 2, b.pos(w(192, 26), 1): 5})
    wide = b.expect(3000)
    for (mod, length, name), r in rows.items():
        if name == "spread":
            first, last = min(b.plan[r]), max(b.plan[r])
            assert wide[r] == [(first, last + K, 4, 7)]
            # mask 1 leaves the first hit and the last (label 3): too far apart in the long read, which splits
            only0 = b.expect(3000, 1, 1)[r]
            assert only0 == ([(first, first + K, 1, 1), (last, last + K, 1, 1)] if length == 9000 else [(first, last + K, 2, 1)])
            third = sorted(b.plan[r])[2]
            assert b.expect(3000, 1, 4)[r] == [(third, third + K, 1, 4)]
        if name == "in turn":
            n = len(b.plan[r])
            assert len(b.expect(20)[r]) == 1 and b.expect(20)[r][0][2:] == (n, 3)
            assert len(b.expect(20, 1, 1)[r]) == (n + 1) // 2 and len(b.expect(20, 1, 2)[r]) == n // 2
            assert b.expect(20, 1, 4)[r] == []
        if name == "close":
            assert [m for (_, _, _, m) in b.expect(20)[r]] == [7, 5, 7]
    for max_gap in (20, 3000):
        for mask in (ALL, 1, 2, 4, 5):
            b.check(dcn, max_gap, 1, mask)
        b.check(dcn, max_gap, 2, 5)
        b.check(dcn, max_gap, 2, ALL)


# ---- 8. the scan over reads and the segment buffer -----------------------------------------------------------------------------
def _one_window_reads(g, n):
    """reads G[i : i + k], i < n, as a batch: read i has one window, whose hash is g.hashes[i]"""
    codes = np.frombuffer(g.seq, np.uint8)
    bases = np.lib.stride_tricks.sliding_window_view(codes, g.k)[:n].reshape(-1).copy()
    return bases, np.arange(n + 1, dtype=np.uint64) * np.uint64(g.k)


def _check_one_window_batch(dcn, g, loc, n, hit):
    bases, offsets = _one_window_reads(g, n)
    so, segs = loc.locate_batch(bases, offsets)
    want = np.concatenate([[0], np.cumsum(hit)]).astype(np.uint64)
    assert np.array_equal(so, want)
    assert len(segs) == int(want[-1])
    for name, value in (("start", 0), ("end", g.k), ("n_hits", 1), ("members", 1)):
        assert (segs[name] == value).all(), name


def _locator_for(dcn, g, n, hit, n_max=None):
    idx = dcn.Index.from_keys(g.hashes[:n][hit], g.k, 1)
    n_max = n_max or n
    return dcn.Locator(idx, max_gap=0, max_batch_bases=n_max * g.k + 64, max_batch_reads=n_max + 1)


@pytest.mark.parametrize("n", [2047, 2048, 2049, 4097])
def test_scan_over_reads_at_block_seams(dcn, g31, n):
    """reads with a hit clustered so that whole blocks of the scan are full or empty; a read's segment count is 0 or 1"""
    idx = np.arange(n)
    for hit in (idx < SCAN_BLOCK - 1,                        # all but the last read of the first block
                idx >= SCAN_BLOCK - 1,                       # that one and every block after it
                (idx < 100) | (idx >= n - 1),                # the last read alone at the far end
                (idx // 8) % 2 == 1,                         # every other thread of the scan
                np.ones(n, bool)):
        loc = _locator_for(dcn, g31, n, hit)
        _check_one_window_batch(dcn, g31, loc, n, hit)
        loc.close()


def test_scan_over_more_than_256_blocks_and_buffer_growth(dcn, g31):
    """530,000 reads are 259 blocks of the scan: locate_scan_blocks_kernel takes two blocks per thread.  About 300,000 of
    them hit, on a fresh context: more than its first segment buffer holds, so the buffer grows and the write pass runs
    again.  A smaller call on the same context follows."""
    n = 530_000
    assert (n + SCAN_BLOCK - 1) // SCAN_BLOCK > SCAN_THREADS
    block = np.arange(n) // SCAN_BLOCK
    rng = np.random.default_rng(8)
    # whole blocks full, whole blocks empty, the rest at random; the blocks past the 256th differ from one another
    kind = rng.integers(0, 4, block[-1] + 1)
    kind[[255, 256, 257, 258]] = (1, 3, 0, 1)
    hit = np.where(kind[block] == 0, False, np.where(kind[block] == 1, True, rng.random(n) < 0.6))
    assert 250_000 < hit.sum() < 350_000 and hit.sum() > SEG_BUFFER
    loc = _locator_for(dcn, g31, n, hit)
    _check_one_window_batch(dcn, g31, loc, n, hit)
    _check_one_window_batch(dcn, g31, loc, 5000, hit[:5000])
    _check_one_window_batch(dcn, g31, loc, n, hit)
    loc.close()


@pytest.mark.parametrize("total", [SEG_BUFFER, SEG_BUFFER + 1])
def test_segment_buffer_edge(dcn, g31, total):
    """exactly what a fresh context's segment buffer holds, and one segment more"""
    n = 70_000
    hit = np.zeros(n, bool)
    hit[:3000] = True
    hit[n - (total - 3000):] = True
    assert hit.sum() == total
    loc = _locator_for(dcn, g31, n, hit)
    _check_one_window_batch(dcn, g31, loc, n, hit)
    loc.close()


# ---- 9. locate's own probe under displacement ---------------------------------------------------------------------------------
def test_probe_in_displaced_slots(oracle, dcn, monkeypatch):
    """the half-full table of test_member_labels_in_displaced_slots through a Locator: as a set (the label is read from
    the slot that matched: the second of a group, a displaced group, group 0 after the last) and as a plain index"""
    monkeypatch.setenv("DCN_TABLE_SLOTS_PER_KEY", "2")
    S = group_slots()
    k, G, members, targets, reads = displaced_members(oracle)
    label = {}
    for j, m in enumerate(members):
        for h in m.tolist():
            label[h] = label.get(h, 0) | (1 << j)
    union = np.array(sorted(label), np.uint64)
    homed = np.bincount(group_of(union, G).astype(np.int64), minlength=G)
    assert all(homed[g] >= S + 4 and homed[(g + 1) % G] >= S for g in targets) and G - 1 in targets

    def want(label_of):
        out = []
        for r in reads:
            (h,), (p,) = oracle.minimizer_hashes_and_positions(r, k, W)
            L = label_of(int(h))
            out.append([(int(p), int(p) + k, 1, L)] if L else [])
        return out

    def got(index, **kw):
        bases, offsets = oracle.concat_reads(reads)
        loc = dcn.Locator(index, max_gap=0, max_batch_bases=len(bases) + 64, max_batch_reads=len(reads) + 1, **kw)
        so, segs = loc.locate_batch(bases, offsets)
        loc.close()
        rows = segs.tolist()
        return [[tuple(s) for s in rows[int(so[r]):int(so[r + 1])]] for r in range(len(reads))]

    s = dcn.IndexSet([dcn.Index.from_keys(m, k, W) for m in members])
    assert s.memory // 12 == G * S and s.n_keys == len(union)
    w = want(lambda h: label.get(h, 0))
    assert sorted(m for sg in w for (_, _, _, m) in sg) == sorted([1] * len(targets) + [2, 4, 6] * len(targets))
    assert sum(1 for sg in w if not sg) == len(targets)
    assert got(s) == w
    for mask in (1, 2, 4, 6):
        assert got(s, member_mask=mask) == want(lambda h: label.get(h, 0) & mask)
    plain = dcn.Index.from_keys(union, k, W)
    assert plain.table_bytes == G * S * 8 and plain.n_keys == len(union)
    assert got(plain) == want(lambda h: 1 if h in label else 0)

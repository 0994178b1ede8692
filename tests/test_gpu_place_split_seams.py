"""The seams of the split placement kernels, with hits placed base by base: w = 1, so every position of a read is a
minimizer and a cut of n bases from a record has n - k + 1 anchor hits on one diagonal.  A read is built from cuts with an
N between them (no k-mer spans an N, so a group's hits and its interval [first q, last q + k) are exactly the cut's);
build() places every cut on a chosen diagonal.  Everything is compared with the model of tests/_place_split_worker.py
exactly; where the construction fixes the outcome it is asserted as well.

Cases 9 to 12 (the path switch, partitions of the LDS count, small tiles, displaced slots) run in the worker, in
processes whose environment sets the hooks."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _place_split_worker as SW
import _place_worker as PW
from conftest import random_reads, revcomp

pytestmark = pytest.mark.gpu

K = 31
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_place_split_worker.py")


@pytest.fixture(scope="module")
def ref(oracle, dcn):
    """two random records of 6,000 and 3,000 bases at w = 1: (records, model, map)"""
    rng = np.random.default_rng(981)
    records = random_reads(rng, 1, 6000, 6000) + random_reads(rng, 1, 3000, 3000)
    model, amap = PW.build_map(oracle, dcn, records, K, 1)
    assert model.info()["repeats"] == 0
    yield records, model, amap
    amap.close()


def hits(n):
    """the length of a cut with n hits"""
    return n + K - 1


def build(records, parts, D0=None, W=1, first=2000):
    """A read of the cuts `parts` = [(record, length, delta, reverse)] with an N between them.  A forward cut's hits have
    the diagonal D0 + delta (D = P - q + len), and D0 is a multiple of W; a reverse-complemented cut is taken where its
    diagonal P + q is D0 + delta as well.  -> (read, [(q0, q1) of each cut's interval])"""
    ln = sum(p[1] for p in parts) + len(parts) - 1
    if D0 is None:
        D0 = (first + ln + W - 1) // W * W
    read, spans, q = [], [], 0
    for rec, n, delta, rev in parts:
        if not rev:
            s = D0 + delta - ln + q  # P - q' = s - q for every hit of the cut
            cut = records[rec][s:s + n]
        else:  # read base q + i is the complement of record base s + n - 1 - i: P + q' = s + n - K + q
            s = D0 + delta - q - n + K
            cut = revcomp(records[rec][s:s + n])
        assert s >= 0 and len(cut) == n, (s, n)
        read.append(cut)
        spans.append((q, q + n))
        q += n + 1
    return b"N".join(read), spans


def run(oracle, dcn, ref, reads, n=4, **kw):
    records, model, amap = ref
    po, rows, counts = SW.check_split(dcn, oracle, model, amap, reads, max_placements=n, **kw)
    return [rows[int(po[r]):int(po[r + 1])] for r in range(len(reads))]


@pytest.mark.parametrize("W", (2, 31, 256))
def test_two_groups_share_a_cell_or_not(oracle, dcn, ref, W):
    """1. diagonals W - 1 and W apart: one placement of both groups; 2W apart: two"""
    records = ref[0]
    reads = [build(records, [(0, hits(30), 0, 0), (0, hits(20), gap, 0)], W=W, first=a)[0]
             for a in (1000, 1000 + W // 2, 1000 + W - 1) for gap in (W - 1, W, 2 * W)]
    got = run(oracle, dcn, ref, reads, band_bases=W, min_votes=1)
    for i, g in enumerate(got):
        if i % 3 < 2 and i < 3:  # (D0 a multiple of W: x and x + W share the cell that starts at x)
            assert g["votes"].tolist() == [50] and g["mapq"].tolist() == [60]
        if i % 3 == 2:
            assert g["votes"].tolist() == [30, 20] and g["rank"].tolist() == [0, 1] and g["n_placed"].tolist() == [2, 2]
            assert g["rival_votes"].tolist() == [0, 0] and (g["n_anchors"] == 50).all()


def test_three_adjacent_bands(oracle, dcn, ref):
    """2. groups at D / W = j - 1, j, j + 1: cells j and j + 1 both hold two of them.  Equal groups: the cells tie and the
    smaller takes j - 1 and j, the third group is round 1.  A larger third group: cell j + 1 wins and the FIRST group is
    round 1.  The middle group leaves with the winner either way: it is nobody's second vote"""
    records, W = ref[0], 64
    eq, sp = build(records, [(0, hits(30), 0, 0), (0, hits(30), W, 0), (0, hits(30), 2 * W, 0)], W=W)
    up, _ = build(records, [(0, hits(30), 0, 0), (0, hits(30), W, 0), (0, hits(35), 2 * W, 0)], W=W)
    mid, _ = build(records, [(0, hits(20), 0, 0), (0, hits(30), W, 0), (0, hits(20), 2 * W, 0)], W=W)
    got = run(oracle, dcn, ref, [eq, up, mid], band_bases=W, min_votes=1)
    assert got[0]["votes"].tolist() == [60, 30] and (got[0]["read_start"][1], got[0]["read_end"][1]) == sp[2]
    assert (got[0]["read_start"][0], got[0]["read_end"][0]) == (sp[0][0], sp[1][1])
    assert got[1]["votes"].tolist() == [65, 30] and (got[1]["read_start"][1], got[1]["read_end"][1]) == sp[0]
    assert got[2]["votes"].tolist() == [50, 20] and got[2]["read_start"].tolist() == [0, hits(20) + 1 + hits(30) + 1]


def test_equal_votes_rank_by_record_strand_and_band(oracle, dcn, ref):
    """3. two rounds of equal votes: the smaller (R, o, j) is rank 0, wherever it lies on the read"""
    records = ref[0]
    n = hits(25)
    reads = [build(records, [(1, n, 0, 0), (0, n, 0, 0)])[0],        # record 0 before record 1
             build(records, [(0, n, 0, 1), (0, n, 700, 0)])[0],      # '+' before '-'
             build(records, [(0, n, 900, 0), (0, n, 0, 0)], W=64)[0],  # the smaller band
             build(records, [(1, n, 0, 1), (1, n, 300, 1), (0, n, 0, 1)], W=64)[0]]
    got = run(oracle, dcn, ref, reads, band_bases=64)
    assert [(g["record"].tolist(), g["reverse"].tolist(), g["read_start"].tolist()) for g in got] == \
        [([0, 1], [0, 0], [n + 1, 0]), ([0, 0], [0, 1], [n + 1, 0]), ([0, 0], [0, 0], [n + 1, 0]),
         ([0, 1, 1], [1, 1, 1], [2 * n + 2, 0, n + 1])]
    assert all((g["votes"] == 25).all() and (g["mapq"] == 60).all() for g in got)


def sandwich(records, outer, inner, inner_rec=1):
    """two cuts of `outer` hits each on ONE diagonal of record 0 with a cut of `inner` hits of another place between them:
    the outer cell's interval spans the inner one's"""
    return build(records, [(0, hits(outer), 0, 0), (inner_rec, hits(inner), 0 if inner_rec else 1500, 0), (0, hits(outer), 0, 0)])[0]


def test_min_votes_and_unreported_rivals(oracle, dcn, ref):
    """4. a second group of exactly min_votes is reported, one of min_votes - 1 is not: but it was computed, and it is the
    rival of the placement whose interval it lies in"""
    records = ref[0]
    reads = [sandwich(records, 40, 5), sandwich(records, 40, 4), sandwich(records, 40, 4, 0)]
    got = run(oracle, dcn, ref, reads, min_votes=5)
    assert got[0]["votes"].tolist() == [80, 5] and got[0]["rival_votes"].tolist() == [5, 80]
    for g in got[1:]:
        assert g["votes"].tolist() == [80] and g["rival_votes"].tolist() == [4] and g["n_placed"].tolist() == [1]
        assert g["mapq"].tolist() == [60 * 76 // 80] and g["n_anchors"].tolist() == [84]


def test_touching_and_overlapping_intervals(oracle, dcn, ref):
    """5. two cuts of 60 bases with nothing between them.  Where the bases on both sides of the junction differ from the
    other record's continuation, the intervals are [0, 60) and [60, 120): they touch, no rival.  Where the second cut's
    first base equals the first record's next base, the first group has one more hit and its interval is [0, 61): one
    base of overlap, each is the other's rival"""
    r0, r1 = ref[0]
    a = 1500
    touch = next(b for b in range(100, 2000) if r1[b] != r0[a + 60] and r1[b - 1] != r0[a + 59])
    over = next(b for b in range(100, 2000) if r1[b] == r0[a + 60] and r1[b + 1] != r0[a + 61] and r1[b - 1] != r0[a + 59])
    reads = [r0[a:a + 60] + r1[touch:touch + 60], r0[a:a + 60] + r1[over:over + 60]]
    got = run(oracle, dcn, ref, reads)
    assert got[0]["votes"].tolist() == [30, 30] and got[0]["read_end"][0] == got[0]["read_start"][1] == 60
    assert got[0]["rival_votes"].tolist() == [0, 0] and got[0]["mapq"].tolist() == [60, 60]
    assert got[1]["votes"].tolist() == [31, 30] and (got[1]["read_end"][0], got[1]["read_start"][1]) == (61, 60)
    assert got[1]["rival_votes"].tolist() == [30, 31] and got[1]["mapq"].tolist() == [60 * 1 // 31, 0]


def test_mapq_values(oracle, dcn, ref):
    """6. 60 (no rival), 0 (a rival as strong or stronger) and a division that floors: 60 * 130 / 140 = 55.7"""
    records = ref[0]
    reads = [sandwich(records, 70, 10), build(records, [(0, hits(40), 0, 0), (1, hits(10), 0, 0)])[0],
             build(records, [(0, hits(12), 0, 0), (1, hits(12), 0, 0), (0, hits(12), 0, 0)])[0]]
    got = run(oracle, dcn, ref, reads)
    assert got[0]["votes"].tolist() == [140, 10] and got[0]["mapq"].tolist() == [55, 0]
    assert got[1]["votes"].tolist() == [40, 10] and got[1]["mapq"].tolist() == [60, 60]
    assert got[2]["votes"].tolist() == [24, 12] and got[2]["mapq"].tolist() == [30, 0]


def test_the_round_after_the_last_is_nobodys_rival(oracle, dcn, ref):
    """7. four groups of 40 (in two halves, around the fourth), 20, 15 and 6 hits.  max_placements = 2 computes three
    rounds: the group of 6 is never computed, and the first placement, whose interval it lies in, has no rival
    (max_placements + 2 groups).  max_placements = 3 computes it as the unreported last round (max_placements + 1
    groups): the first placement's rival has 6 votes"""
    records = ref[0]
    read = build(records, [(0, hits(20), 0, 0), (1, hits(6), 0, 0), (0, hits(20), 0, 0), (1, hits(20), 600, 0),
                           (0, hits(15), 2500, 1)])[0]
    two = run(oracle, dcn, ref, [read], n=2)[0]
    assert two["votes"].tolist() == [40, 20] and two["rival_votes"].tolist() == [0, 0] and two["n_anchors"].tolist() == [81, 81]
    three = run(oracle, dcn, ref, [read], n=3)[0]
    assert three["votes"].tolist() == [40, 20, 15] and three["rival_votes"].tolist() == [6, 0, 0]
    assert three["mapq"].tolist() == [60 * 34 // 40, 60, 60]
    four = run(oracle, dcn, ref, [read], n=4)[0]
    assert four["votes"].tolist() == [40, 20, 15, 6] and four["mapq"].tolist() == [51, 60, 60, 0]
    one = run(oracle, dcn, ref, [read], n=1)[0]  # round 1 is the last computed one: disjoint, no rival
    assert one["votes"].tolist() == [40] and one["rival_votes"].tolist() == [0]


def test_bitmap_words_shared_with_neighbours(oracle, dcn, ref):
    """8. reads of two or three small groups whose starts cover every offset mod 32 of the batch stream, so that every
    read's first and last word of the anchor bitmap's copy also holds hits of its neighbours, which are cleared while the
    read's own rounds run.  The model places a read by itself: equality in both orders of the batch says that no read's
    rounds saw or cleared a neighbour's bits"""
    records = ref[0]
    rng = np.random.default_rng(982)
    reads = []
    for i in range(320):
        parts = [(int(rng.integers(0, 2)), hits(int(rng.integers(1, 5))), int(rng.integers(0, 1500)), int(rng.integers(0, 2)))
                 for _ in range(2 + i % 2)]
        reads.append(build(records, parts, first=int(rng.integers(600, 1200)))[0])
        if i % 9 == 0:
            reads.append(random_reads(rng, 1, 33, 33)[0])
    starts = np.cumsum([0] + [len(r) for r in reads[:-1]])
    assert set((starts % 32).tolist()) == set(range(32))
    for batch in (reads, reads[::-1]):
        got = run(oracle, dcn, ref, batch, n=2, band_bases=31, min_votes=1)
        assert sum(len(g) == 2 for g in got) > 250


SCAN_BLOCK = 2048  # DCN_SCAN_BLOCK: reads per block of the scan of the per-read counts into place_offsets


@pytest.fixture(scope="module")
def scan_kinds(ref):
    """four short reads with 0, 1, 2 and 2 placements, each with the model's (rows, read_counts), computed once"""
    records, model, _ = ref
    kinds = [random_reads(np.random.default_rng(983), 1, 70, 70)[0],
             build(records, [(0, hits(30), 0, 0)])[0],
             build(records, [(0, hits(20), 0, 0), (1, hits(15), 0, 0)])[0],
             build(records, [(1, hits(25), 0, 1), (0, hits(12), 900, 0)])[0]]
    want = [SW.place_split(model, r) for r in kinds]
    assert [len(rows) for rows, _ in want] == [0, 1, 2, 2]
    return kinds, want


@pytest.mark.parametrize("before", (True, False))
@pytest.mark.parametrize("n_reads", (SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1, 2 * SCAN_BLOCK + 1))
def test_offsets_across_the_scan_blocks(oracle, dcn, ref, scan_kinds, n_reads, before):
    """13. place_offsets where the scan over reads changes block (2,048 reads each) and at its last, partial block: the
    placements either all lie before read 2,047, so that every offset from the first block's last read on is the total,
    or they begin at read 2,047, so that the first block's sum is 0 but for its last read and the later blocks carry
    the prefix.  Offsets, rows and read_counts are the model's, expanded from one run per distinct read"""
    kinds, want = scan_kinds
    edge = SCAN_BLOCK - 1
    which = [(1 + i % 3 if (i < edge) == before else 0) for i in range(n_reads)]
    w_off, w_rows, w_counts = [0], [], []
    for kind in which:
        w_rows += want[kind][0]
        w_counts.append(want[kind][1])
        w_off.append(len(w_rows))
    assert (w_off[edge] == w_off[-1] and w_off[-1] > 0) if before else (w_off[edge] == 0 and (n_reads == edge or w_off[-1] > 0))
    b, o = oracle.concat_reads([kinds[kind] for kind in which])
    p = dcn.Placer(ref[2], max_batch_bases=1 << 20, max_batch_reads=1 << 13)
    try:
        got = p.place_split_batch(b, o, max_placements=4)
    finally:
        p.close()
    SW.assert_split(got, (w_off, w_rows, w_counts), (n_reads, before))


def run_worker(case, **env):
    p = subprocess.run([sys.executable, WORKER, case], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout


def test_path_switch():
    """9."""
    assert "place split switch ok" in run_worker("switch", DCN_PLACE_LANE_BASES="100")


def test_partitions():
    """10."""
    assert "place split partitions ok" in run_worker("partitions", DCN_PLACE_LDS_CELLS="16", DCN_PLACE_LANE_BASES="0")


def test_tile_seams():
    """11."""
    assert "place split seams ok" in run_worker("seams", DCN_TILE_WINDOWS="16")


def test_displaced_slots():
    """12."""
    assert "place split displaced ok" in run_worker("displaced", DCN_TABLE_SLOTS_PER_KEY="2")

"""The seams of paired placement (place_pair.hip and dcn_place_pair_batch) with hits placed base by base: a map at k = 31,
w = 1 over the k-mers at chosen positions only (tests/_place_pair_worker.py: Seams), so that every vote count, extent and
read interval below is set by where a cut begins and ends.  Each case first asserts ON THE MODEL that its seam is really
hit (the two sums are equal, the rival is round N, ...), then compares the GPU's rows with the model's, all 80 bytes.
Blocks of 1000 bases keep the cases apart: block i of a record begins at base 1000 * i."""
import numpy as np
import pytest

import _place_pair_worker as PPW
import _place_worker as PW
from _place_pair_worker import F, MATE_PLACED, PROPER, RESCUED, UNPLACED
from conftest import revcomp

pytestmark = pytest.mark.gpu

K = 31
W = 32  # band_bases of every case: parts a few hundred bases apart never share a cell


def block(i):
    return 1000 * i


def overlap_base(records):
    """a position c of record 1's block 11 whose first base equals record 0's base at block 11 + 70: the k-mer there can
    begin on the last base of a cut of record 0 that ends at + 71"""
    B = block(11)
    for c in range(B + 500, B + 600):
        if records[1][c] == records[0][B + 70]:
            return c
    raise AssertionError("no such base")


def positions(records):
    p0, p1 = [], []
    at = lambda i, ds: [block(i) + d for d in ds]  # noqa: E731
    p0 += at(1, (0, 40, 80, 600, 640))            # insert: T = 671
    p0 += at(2, (700, 730, 770))                  # F begins one base before V ends
    p0 += at(3, (700, 731, 770))                  # F begins where V ends
    p0 += at(4, (0, 40, 80))                      # equal ref_start
    p0 += at(5, (0, 40, 600, 640))                # ties (0,0) / (1,1)
    p1 += at(5, (0, 40, 600, 640))
    p0 += at(6, (0, 40, 80, 600, 640))            # ties (0,1) / (1,0)
    p1 += at(6, (0, 40, 600, 640, 680))
    p0 += at(7, (0, 40, 300, 340, 600, 640))      # ties (0,0) / (0,1)
    p1 += at(8, (0, 40, 80))                      # the concordant round at t = N
    p0 += at(8, (0, 40, 600, 640))
    p0 += at(9, (0, 40, 600))                     # min_votes
    p0 += at(10, (0, 40, 120, 600, 640))          # the rival from round N
    p1 += at(10, (71, 600, 640))
    p0 += at(11, (0, 40, 600, 640))               # intervals that touch / overlap by one base
    p1 += at(11, (300,)) + [overlap_base(records)]
    p0 += at(12, (0, 40, 80, 600, 640))           # offsets mod 32
    return {0: p0, 1: p1}


@pytest.fixture(scope="module")
def seams(oracle, dcn):
    records = PW.make_records(PW.make_genomes())
    S = PPW.Seams(oracle, records, positions(records)).attach(dcn)
    yield S
    S.close()


def cut(S, R, i, a, b):
    return S.records[R][block(i) + a:block(i) + b]


def rc(S, R, i, a, b):
    return revcomp(cut(S, R, i, a, b))


def model_pair(S, m1, m2, **kw):
    return PPW.place_pair(S.model, m1, m2, W=W, **kw)


def check(S, oracle, dcn, reads, what, **kw):
    return PPW.check_pairs(dcn, oracle, S.model, S.amap, reads, (what,), band_bases=W, **kw)


def test_insert_at_the_limit_and_one_past(seams, oracle, dcn):
    S = seams
    m1, m2 = cut(S, 0, 1, 0, 111), rc(S, 0, 1, 600, 671)
    a, b, T = model_pair(S, m1, m2, max_insert=671)
    assert T == 671 and a[F["votes"]] == 3 and b[F["votes"]] == 2 and a[F["tlen"]] == 671 and b[F["tlen"]] == -671
    assert a[F["ref_start"]] == block(1) and b[F["ref_end"]] == block(1) + 671
    a, b, T = model_pair(S, m1, m2, max_insert=670)
    assert T is None and a[F["flags"]] == b[F["flags"]] == MATE_PLACED
    for I in (671, 670):
        check(S, oracle, dcn, [m1, m2, m2, m1], "insert", max_insert=I)


def test_forward_mate_must_begin_before_the_reverse_mate_ends(seams, oracle, dcn):
    S = seams
    before = (cut(S, 0, 2, 730, 801), rc(S, 0, 2, 690, 731))  # F.ref_start == V.ref_end - 1
    at_end = (cut(S, 0, 3, 731, 801), rc(S, 0, 3, 690, 731))  # F.ref_start == V.ref_end
    a, b, T = model_pair(S, *before)
    assert T == 101 and a[F["ref_start"]] == b[F["ref_end"]] - 1 and b[F["flags"]] == PROPER | RESCUED | MATE_PLACED
    assert a[F["tlen"]] == -101 and b[F["tlen"]] == 101  # (the reverse mate lies first)
    a, b, T = model_pair(S, *at_end)
    assert T is None and a[F["ref_start"]] == block(3) + 731 and b[F["record"]] == UNPLACED and b[F["n_anchors"]] == 1
    check(S, oracle, dcn, list(before) + list(at_end) + list(before[::-1]) + list(at_end[::-1]), "begin")


def test_equal_ref_start_gives_mate_one_the_positive_tlen(seams, oracle, dcn):
    S = seams
    f, v = cut(S, 0, 4, 0, 111), rc(S, 0, 4, 0, 71)
    for m1, m2 in ((f, v), (v, f)):
        a, b, T = model_pair(S, m1, m2)
        assert T == 111 and a[F["ref_start"]] == b[F["ref_start"]] == block(4) and a[F["tlen"]] == 111 and b[F["tlen"]] == -111
    check(S, oracle, dcn, [f, v, v, f], "tie of ref_start")


def test_ties_between_combinations(seams, oracle, dcn):
    S = seams
    # (0, 0) and (1, 1) at 2 + 2 votes
    m1 = cut(S, 0, 5, 0, 71) + cut(S, 1, 5, 0, 71)
    m2 = rc(S, 0, 5, 600, 671) + rc(S, 1, 5, 600, 671)
    r1, r2 = (PPW.mate_rounds(S.model, m, W)[0] for m in (m1, m2))
    assert [x.votes for x in r1] == [2, 2] == [x.votes for x in r2]
    assert all(PPW.template(r1[t], r2[t], 1000, 2) == 671 for t in (0, 1)) and PPW.template(r1[0], r2[1], 1000, 2) is None
    a, b, _ = model_pair(S, m1, m2)
    assert (a[F["rank"]], b[F["rank"]]) == (0, 0) and a[F["pair_votes"]] == 4 and a[F["record"]] == 0
    reads = [m1, m2]
    # (0, 1) and (1, 0) at 3 + 2 and 2 + 3 votes: the smaller a
    m1 = cut(S, 0, 6, 0, 111) + cut(S, 1, 6, 0, 71)
    m2 = rc(S, 0, 6, 600, 671) + rc(S, 1, 6, 600, 711)
    r1, r2 = (PPW.mate_rounds(S.model, m, W)[0] for m in (m1, m2))
    assert [(x.R, x.votes) for x in r1] == [(0, 3), (1, 2)] and [(x.R, x.votes) for x in r2] == [(1, 3), (0, 2)]
    assert PPW.template(r1[0], r2[1], 1000, 2) == 671 and PPW.template(r1[1], r2[0], 1000, 2) == 711
    a, b, _ = model_pair(S, m1, m2)
    assert (a[F["rank"]], b[F["rank"]]) == (0, 1) and a[F["pair_votes"]] == b[F["pair_votes"]] == 5
    reads += [m1, m2, m2, m1]
    # (0, 0) and (0, 1) at 2 + 2 votes: the smaller b
    m1 = cut(S, 0, 7, 0, 71)
    m2 = rc(S, 0, 7, 300, 371) + rc(S, 0, 7, 600, 671)
    r1, r2 = (PPW.mate_rounds(S.model, m, W)[0] for m in (m1, m2))
    assert [x.votes for x in r2] == [2, 2] and r2[0].p0 == block(7) + 300
    assert [PPW.template(r1[0], y, 1000, 2) for y in r2] == [371, 671]
    a, b, T = model_pair(S, m1, m2)
    assert (a[F["rank"]], b[F["rank"]], T) == (0, 0, 371)
    reads += [m1, m2, m2, m1]
    check(S, oracle, dcn, reads, "ties")


def test_a_concordant_round_at_t_equal_n_is_no_candidate(seams, oracle, dcn):
    S = seams
    m1 = cut(S, 1, 8, 0, 111) + cut(S, 0, 8, 0, 71)
    m2 = rc(S, 0, 8, 600, 671)
    r1 = PPW.mate_rounds(S.model, m1, W, 0, 1)[0]
    assert [(x.R, x.votes) for x in r1] == [(1, 3), (0, 2)]  # (round 1 = N is computed)
    a, b, T = model_pair(S, m1, m2, max_placements=1)
    assert T is None and a[F["record"]] == 1 and a[F["flags"]] == b[F["flags"]] == MATE_PLACED
    a, b, T = model_pair(S, m1, m2, max_placements=2)
    assert T == 671 and (a[F["rank"]], b[F["rank"]]) == (1, 0) and a[F["record"]] == 0
    for n in (1, 2):
        check(S, oracle, dcn, [m1, m2, m2, m1], "t = N", max_placements=n)


def test_one_mate_must_reach_min_votes(seams, oracle, dcn):
    S = seams
    m1, m2 = cut(S, 0, 9, 0, 71), rc(S, 0, 9, 600, 631)
    a, b, T = model_pair(S, m1, m2, min_votes=3)
    assert T is None and a[F["n_anchors"]] == 2 and b[F["n_anchors"]] == 1 and a[F["record"]] == b[F["record"]] == UNPLACED
    a, b, T = model_pair(S, m1, m2, min_votes=2)
    assert T == 631 and b[F["flags"]] == PROPER | RESCUED | MATE_PLACED and a[F["flags"]] == PROPER | MATE_PLACED
    for votes in (3, 2):
        check(S, oracle, dcn, [m1, m2, m2, m1], "min_votes", min_votes=votes)


def rival_read(S):
    """record 0's hits at read positions 0, 40 and 120 with record 1's single hit at 71 between them"""
    return cut(S, 0, 10, 0, 71) + cut(S, 1, 10, 71, 102) + cut(S, 0, 10, 102, 151)


def test_the_rival_is_taken_from_the_unreported_round_n(seams, oracle, dcn):
    S = seams
    m1 = rival_read(S)
    r1 = PPW.mate_rounds(S.model, m1, W, 0, 1)[0]
    assert [(x.R, x.votes, x.q0, x.q1) for x in r1] == [(0, 3, 0, 151), (1, 1, 71, 102)]
    on0, on1 = rc(S, 0, 10, 600, 671), rc(S, 1, 10, 600, 671)
    a, b, T = model_pair(S, m1, on0, max_placements=1)
    assert T == 671 and a[F["pair_votes"]] == 5 and a[F["rival_votes"]] == 1 and a[F["mapq"]] == 48  # (the rival is round 1 = N)
    a, b, T = model_pair(S, m1, on1, max_placements=1)
    assert T is None and a[F["rival_votes"]] == 1 and a[F["pair_votes"]] == 3  # (round N gets nothing from the partner)
    a, b, T = model_pair(S, m1, on1, max_placements=2)  # (as a candidate the single hit is the concordant one)
    assert T == 600 and a[F["rank"]] == 1 and a[F["flags"]] == PROPER | RESCUED | MATE_PLACED
    assert a[F["pair_votes"]] == 3 and a[F["rival_votes"]] == 3 and a[F["mapq"]] == 0
    for n in (1, 2):
        check(S, oracle, dcn, [m1, on0, m1, on1, on1, m1, on0, m1], "rival", max_placements=n)


def test_intervals_that_touch_and_that_overlap_by_one_base(seams, oracle, dcn):
    S = seams
    c = overlap_base(S.records)
    touch = cut(S, 0, 11, 0, 71) + cut(S, 1, 11, 300, 331)
    over = cut(S, 0, 11, 0, 71) + S.records[1][c + 1:c + K]
    assert over[70:70 + K] == S.records[1][c:c + K]
    m2 = rc(S, 0, 11, 600, 671)
    for m1, q0, rival in ((touch, 71, 0), (over, 70, 1)):
        r1 = PPW.mate_rounds(S.model, m1, W)[0]
        assert [(x.R, x.votes, x.q0, x.q1) for x in r1] == [(0, 2, 0, 71), (1, 1, q0, q0 + K)]
        a, b, T = model_pair(S, m1, m2)
        assert T == 671 and a[F["rival_votes"]] == rival and a[F["mapq"]] == 60 * (4 - rival) // 4
    check(S, oracle, dcn, [touch, m2, over, m2, m2, over, m2, touch], "intervals")


def test_the_pair_boundary_at_every_offset_mod_32(seams, oracle, dcn):
    """the mates of a pair share a word of the bitmaps wherever the boundary is no multiple of 32"""
    S = seams
    reads = []
    for i in range(64):  # (a pair of 193 or 225 bases: the pair's first base moves on by one bit of the word per pair)
        reads += [cut(S, 0, 12, 0, 111 + 32 * (i % 2)), rc(S, 0, 12, 589, 671)]
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in reads])])
    assert {int(x) % 32 for x in offsets[1::2]} == set(range(32)) and {int(x) % 32 for x in offsets[2::2]} == set(range(32))
    rows, _, _ = check(S, oracle, dcn, reads, "offsets")
    assert (rows["flags"] & PROPER).all() and (rows["tlen"][0::2] == 671).all()


def proper_pairs(S):
    return [(cut(S, 0, 1, 0, 111), rc(S, 0, 1, 600, 671)), (cut(S, 0, 4, 0, 111), rc(S, 0, 4, 0, 71)),
            (rc(S, 0, 2, 690, 731), cut(S, 0, 2, 730, 801))]


@pytest.mark.parametrize("n_pairs", [255, 256, 257, 513])
def test_workgroup_edges_of_the_pair_kernel(seams, oracle, dcn, n_pairs):
    """one lane per pair, 256 lanes per workgroup: the last workgroup full, one lane short, one lane over; at 513 every
    pair is proper and the histogram is summed over three workgroups"""
    S = seams
    cycle = proper_pairs(S)
    if n_pairs != 513:
        cycle = cycle + [(cut(S, 0, 3, 731, 801), rc(S, 0, 3, 690, 731))]  # (not proper)
    reads = [m for u in range(n_pairs) for m in cycle[u % len(cycle)]]
    rows, hist, _ = check(S, oracle, dcn, reads, "edges")
    n_proper = int((rows["flags"] & PROPER).astype(bool).sum()) // 2
    assert int(hist.sum()) == n_proper == (513 if n_pairs == 513 else n_pairs - n_pairs // 4)
    assert sorted(np.flatnonzero(hist).tolist()) == [101 // 8, 111 // 8, 671 // 8]


def test_histogram_bin_edges_and_the_overflow_bin(seams, oracle, dcn):
    S = seams
    m1, m2 = proper_pairs(S)[0]  # T = 671
    for hbin, where in ((671, 1), (672, 0), (11, 61), (3, 223), (2, 255), (1, 255)):
        assert min(671 // hbin, 255) == where
        _, hist, _ = check(S, oracle, dcn, [m1, m2] * 3, "bins", hist_bin_bases=hbin)
        assert hist[where] == 3 and int(hist.sum()) == 3

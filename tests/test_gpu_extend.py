"""dcn_extend_batch on the rows the three placement calls return, against the model of tests/_extend_worker.py (a full table
per flank: no wavefront, no lanes, no early stop): reads cut from three 3 kbp random records -- error-free, with 5 % mixed
edits, on both strands, chimeras, unplaced reads, reads with N and lower case -- at (k, w) = (31, 15) and (31, 1).  What the
extended rows are to the calls that take them next: verify, align and pileup.  How a batch is cut and ordered, and one
context serving every call.  Every comparison is exact."""
import numpy as np
import pytest

import _extend_worker as XW
import _pileup_worker as PW
import _verify_worker as VW
from conftest import random_reads, revcomp

pytestmark = pytest.mark.gpu

CASES = [(31, 15), (31, 1)]
OVER, UNPLACED = VW.OVER, VW.UNPLACED
LR = 3000


def make_records():
    recs = random_reads(np.random.default_rng(1611), 3, LR, LR)
    low = bytearray(recs[2])
    low[500:700] = bytes(low[500:700]).lower()
    low[1500:1503] = b"NNN"
    return [recs[0], recs[1], bytes(low)]


def make_reads(records):
    rng = np.random.default_rng(1612)

    def cut(lo, hi):
        while True:  # (not across the record's NNN)
            R, ln = int(rng.integers(0, 3)), int(rng.integers(lo, hi + 1))
            at = int(rng.integers(0, LR - ln))
            if not (R == 2 and at < 1510 and at + ln > 1490):
                return records[R][at:at + ln]

    reads = []
    for _ in range(10):
        reads.append(cut(100, 300))
        reads.append(revcomp(cut(100, 300)))
        reads.append(VW.mutate_mixed(rng, cut(150, 300), 0.05))
        reads.append(revcomp(VW.mutate_mixed(rng, cut(150, 300), 0.05)))
    for _ in range(3):
        reads.append(cut(150, 250) + revcomp(cut(150, 250)))  # chimeras: a flank of the other part's length, clipped
        s = bytearray(cut(200, 300))
        s[8:10] = b"NN"
        reads.append(bytes(s))                                # N in a flank of the read
        reads.append(cut(150, 300).lower())
    reads += [records[2][400:800], revcomp(records[2][1400:1600]), records[0][:150], records[1][LR - 150:], revcomp(records[0][:150])]
    reads += random_reads(rng, 4, 50, 200) + [b"", b"ACGT"]   # unplaced
    if len(reads) % 2:
        reads.append(records[0][700:900])
    return reads


@pytest.fixture(scope="module")
def built(dcn, oracle):
    records = make_records()
    reads = make_reads(records)
    out = {}
    for k, w in CASES:
        amap = VW.build_map(oracle, dcn, records, k, w)
        placer = dcn.Placer(amap, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
        out[(k, w)] = (amap, placer)
    yield records, reads, oracle.concat_reads(reads), out
    for amap, placer in out.values():
        placer.close()
        amap.close()


def assert_same(got, want, rows):
    (got_rows, got_ext), (want_rows, want_ext) = got, want
    assert got_rows.dtype == rows.dtype == want_rows.dtype and got_ext.dtype == np.dtype(XW.EXTENSION_FIELDS)
    bad = np.nonzero(got_ext != want_ext)[0]
    assert len(bad) == 0, [(int(t), rows[t], got_ext[t], want_ext[t]) for t in bad[:5]]
    assert got_rows.tobytes() == want_rows.tobytes()


@pytest.mark.parametrize("k,w", CASES)
def test_rows_of_the_three_placement_calls(built, dcn, k, w):
    records, reads, (b, o), maps = built
    amap, placer = maps[(k, w)]
    po, srows, _ = placer.place_split_batch(b, o, max_placements=4)
    prows, _ = placer.place_pair_batch(b, o)
    for rows, ro in ((placer.place_batch(b, o), None), (srows, po), (prows, None)):
        before = rows.copy()
        got = placer.extend_batch(b, o, rows, row_offsets=ro)
        assert rows.tobytes() == before.tobytes()  # the caller's rows are not written
        want = XW.extend_rows(reads, records, rows, row_offsets=ro)
        assert_same(got, want, rows)
        xrows, ext = got
        placed = rows["record"] != UNPLACED
        assert placed.sum() > 40 and (ro is not None or (~placed).sum() >= 5)
        gained = (xrows["read_end"] - xrows["read_start"]).astype(np.int64) - (rows["read_end"] - rows["read_start"]).astype(np.int64)
        # (at w = 1 every k-mer of an error-free read is an anchor hit: only reads with edits near an end have flanks)
        assert (gained >= 0).all() and (gained[placed] > 0).sum() > (25 if w > 1 else 5) and (gained[~placed] == 0).all()
        assert (ext["left_edits"] > 0).any() and (ext["right_edits"] > 0).any()
        # what the extended rows are to verify: accepted, and no worse than the edits of the three parts (the threshold is
        # the longer extent, so that every placed row has a distance)
        edits = placer.verify_batch(b, o, rows, row_offsets=ro, max_permille=1000)
        xedits = placer.verify_batch(b, o, xrows, row_offsets=ro, max_permille=1000)
        assert (xedits[~placed] == UNPLACED).all() and (edits[placed] < OVER).all() and (xedits[placed] < OVER).all()
        assert (xedits[placed].astype(np.int64) <= edits[placed].astype(np.int64) + ext["left_edits"][placed] + ext["right_edits"][placed]).all()
        assert xedits.tolist() == VW.verify_rows(reads, records, xrows, row_offsets=ro, max_permille=1000).tolist()


@pytest.mark.parametrize("k,w", CASES)
def test_error_free_reads_extend_to_their_whole_length(dcn, oracle, built, k, w):
    """reads cut error-free from the reference, on both strands: 0 .. L on the interval they were cut from"""
    records, _, _, maps = built
    amap, placer = maps[(k, w)]
    rng = np.random.default_rng(1613)
    reads, truth = [], []
    for n in range(60):
        R, ln = n % 3, int(rng.integers(100, 200))
        at = int(rng.integers(0, LR - ln)) if n >= 6 else (0 if n < 3 else LR - ln)  # ... and at either end of a record
        if R == 2 and at < 1510 and at + ln > 1490:
            at = 1510
        s = records[R][at:at + ln]
        reads.append(revcomp(s) if n % 2 else s)
        truth.append((R, n % 2, at, at + ln, ln))
    b, o = oracle.concat_reads(reads)
    rows = placer.place_batch(b, o)
    xrows, ext = placer.extend_batch(b, o, rows)
    assert (rows["record"] != UNPLACED).all()
    short = ((rows["read_end"] - rows["read_start"]) < [t[4] for t in truth]).sum()
    assert short > 50 or w == 1  # the anchors' extents stop short of the read's ends: there is something to extend
    for t, (R, rev, lo, hi, ln) in enumerate(truth):
        assert (int(xrows["record"][t]), int(xrows["reverse"][t]), int(xrows["read_start"][t]), int(xrows["read_end"][t]),
                int(xrows["ref_start"][t]), int(xrows["ref_end"][t])) == (R, rev, 0, ln, lo, hi), t
    assert not ext["left_edits"].any() and not ext["right_edits"].any()
    assert not placer.verify_batch(b, o, xrows).any()


def test_pileup_over_extended_rows_has_the_true_coverage(dcn, oracle):
    """error-free reads tiled over a record, every base covered by exactly 3 of them (fewer at the record's ends): the
    pileup over the extended rows has that coverage at every base; over the original rows it is lower at read ends"""
    rng = np.random.default_rng(1614)
    record = random_reads(rng, 1, 2400, 2400)[0]
    amap = VW.build_map(oracle, dcn, [record])
    amap.pileup_enable()
    placer = dcn.Placer(amap, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    reads, truth = [], np.zeros(2400, np.int64)
    for n, at in enumerate(range(0, 2400 - 150 + 1, 50)):
        s = record[at:at + 150]
        reads.append(revcomp(s) if n % 2 else s)
        truth[at:at + 150] += 1
    b, o = oracle.concat_reads(reads)
    rows = placer.place_batch(b, o)
    assert (rows["record"] == 0).all()
    xrows, _ = placer.extend_batch(b, o, rows)
    _, n_added = placer.pileup_batch(b, o, xrows)
    extended = amap.pileup_fetch(0)
    assert n_added == len(reads)
    assert np.array_equal(extended[:, :6].sum(axis=1), truth) and truth[200:-200].min() == 3 == truth.max()
    codes = np.frombuffer(record, np.uint8)
    for col, letter in ((PW.A, b"A"), (PW.C, b"C"), (PW.G, b"G"), (PW.T, b"T")):
        assert np.array_equal(extended[:, col], np.where(codes == letter[0], truth, 0))
    amap.pileup_reset()
    placer.pileup_batch(b, o, rows)
    original = amap.pileup_fetch(0)[:, :6].sum(axis=1)
    assert (original <= truth).all() and (original < truth).sum() > 100
    placer.close()
    amap.close()


def test_cut_and_order_do_not_matter(built, dcn):
    """one batch = the same rows in three calls = the rows in reverse order (rule X8)"""
    records, reads, (b, o), maps = built
    amap, placer = maps[(31, 15)]
    po, srows, _ = placer.place_split_batch(b, o, max_placements=4)
    po = po.astype(np.int64)
    whole_rows, whole = placer.extend_batch(b, o, srows, row_offsets=po)
    parts = []
    for lo, hi in ((0, 17), (17, 18), (18, len(reads))):
        cb, co = dcn.concat_reads(reads[lo:hi])
        parts.append(placer.extend_batch(cb, co, srows[po[lo]:po[hi]], row_offsets=po[lo:hi + 1] - po[lo]))
    assert np.concatenate([p[1] for p in parts]).tobytes() == whole.tobytes()
    assert np.concatenate([p[0] for p in parts]).tobytes() == whole_rows.tobytes()
    rows = placer.place_batch(b, o)
    forwards = placer.extend_batch(b, o, rows)[1]
    rb, ro = dcn.concat_reads(reads[::-1])
    backwards = placer.extend_batch(rb, ro, rows[::-1].copy())[1]
    assert backwards[::-1].tobytes() == forwards.tobytes()


def test_one_context_serves_every_call(built, dcn):
    """place, split, extend, align, extend and pileup on one context; verify, align and pileup on the original rows are byte
    for byte what they were before an extend call; the six counters stay; profiling sees pack and finish"""
    records, reads, (b, o), maps = built
    amap, placer = maps[(31, 15)]
    placer.place_batch(b, o)
    po, srows, _ = placer.place_split_batch(b, o)
    amap.pileup_enable()
    verify_before = placer.verify_batch(b, o, srows, row_offsets=po)
    align_before = placer.align_batch(b, o, srows, row_offsets=po)
    placer.pileup_batch(b, o, srows, row_offsets=po)
    pile_before = [amap.pileup_fetch(R).copy() for R in range(3)]
    first = placer.extend_batch(b, o, srows, row_offsets=po)
    want = XW.extend_rows(reads, records, srows, row_offsets=po)
    assert_same(first, want, srows)
    assert placer.verify_batch(b, o, srows, row_offsets=po).tobytes() == verify_before.tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(placer.align_batch(b, o, srows, row_offsets=po), align_before))
    before = placer.stats()
    placer.set_profiling(True)
    again = placer.extend_batch(b, o, srows, row_offsets=po)
    ms, n = placer.profile()
    placer.set_profiling(False)
    assert n == 1 and ms["pack"] > 0 and ms["finish"] > 0 and placer.stats() == before
    assert again[1].tobytes() == first[1].tobytes() and again[0].tobytes() == first[0].tobytes()
    amap.pileup_reset()
    placer.pileup_batch(b, o, srows, row_offsets=po)
    assert all(np.array_equal(amap.pileup_fetch(R), pile_before[R]) for R in range(3))
    # ... and the extended rows through align and pileup: every read base of the extent is in the runs
    edits, co, cigar = placer.align_batch(b, o, first[0], row_offsets=po)
    ok = edits < OVER
    assert ok.sum() > 40
    for t in np.nonzero(ok)[0][:40]:
        runs = cigar[int(co[t]):int(co[t + 1])]
        on_read = sum(int(x) >> 4 for x in runs if int(x) & 15 != 2)
        assert on_read == int(first[0]["read_end"][t]) - int(first[0]["read_start"][t])
    amap.pileup_reset()
    assert placer.pileup_batch(b, o, first[0], row_offsets=po)[1] == ok.sum()
    amap.pileup_disable()
    # the argument errors come from dcn_verify_batch's walk, with its messages and row numbers
    bad = srows.copy()
    bad["ref_end"][3] = LR + 1
    with pytest.raises(dcn.DeaconHipError) as e:
        placer.extend_batch(b, o, bad, row_offsets=po)
    assert e.value.code == dcn._native.DCN_ERR_ARG and "row 3: ref_end %d is past the record's %d bases" % (LR + 1, LR) in e.value.message

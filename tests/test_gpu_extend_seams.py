"""The seams of dcn_extend_batch and its kernel (extend.hip), with rows written by hand: no hashing decides anything here.
The map keeps the bases of two short records, the second starting mid-word of the store; every case is compared with the
model of tests/_extend_worker.py exactly (a full table per flank: it has no wavefront and shares nothing with the kernel),
and says what it expects of the model's answer, so that a case cannot quietly stop meeting its seam.

A case is built by put(): R' = left + S + right is the read as the row's strand reads it, S lies on records[R][a:b], and
what left and right are is the case."""
import numpy as np
import pytest

import _extend_worker as XW
import _verify_worker as VW
from conftest import random_reads, revcomp

pytestmark = pytest.mark.gpu

UNPLACED = VW.UNPLACED
L0, L1 = 3989, 1777


def make_records():
    rng = np.random.default_rng(1621)
    a, b = bytearray(random_reads(rng, 1, L0, L0)[0]), bytearray(random_reads(rng, 1, L1, L1)[0])
    b[100:103] = b"NNN"                      # N against N, N against a base
    b[200:260] = bytes(b[200:260]).lower()   # lower case in the record
    b[700:760] = b"A" * 60                   # a homopolymer
    b[-2:] = b"CA"                           # (the tie on i at the record's last two bases)
    return [bytes(a), bytes(b)]  # (3989 % 16 != 0: the second record starts mid-word of the store)


@pytest.fixture(scope="module")
def env(dcn, oracle):
    records = make_records()
    amap = VW.build_map(oracle, dcn, records)
    placer = dcn.Placer(amap, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    yield dcn, oracle, records, amap, placer
    placer.close()
    amap.close()


def other(c):
    """a letter that is not c"""
    return b"C" if bytes(c).upper() == b"A" else b"A"


def sub(s, at):
    return s[:at] + other(s[at:at + 1]) + s[at + 1:]


class Case:
    """reads and hand-written rows of one call"""

    def __init__(self, dcn, records, seed, dtype=None, lead=True):
        self.dcn, self.records, self.rng = dcn, records, np.random.default_rng(seed)
        self.dtype = dtype or dcn.filter.PLACEMENT_DTYPE
        self.reads, self.rows = [], []
        if lead:  # a first read of 37 bases, so that no read of the batch starts on a word of the stream
            self.reads, self.rows = [random_reads(self.rng, 1, 37, 37)[0]], [VW.make_row(self.dtype, UNPLACED, 0, 0, 0, 0, 0)]

    def put(self, left, S, right, R, a, b, rev=0):
        oriented = left + S + right
        L = len(oriented)
        lo, hi = len(left), len(left) + len(S)
        self.reads.append(revcomp(oriented) if rev else oriented)
        self.rows.append(VW.make_row(self.dtype, R, rev, L - hi if rev else lo, L - lo if rev else hi, a, b))
        return len(self.rows) - 1

    def run(self, placer, oracle, **kw):
        rows = np.concatenate(self.rows)
        b, o = oracle.concat_reads(self.reads)
        got_rows, got = placer.extend_batch(b, o, rows, **kw)
        want_rows, want = XW.extend_rows(self.reads, self.records, rows, **kw)
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, [(int(t), rows[t], got[t], want[t]) for t in bad[:5]]
        assert got_rows.tobytes() == want_rows.tobytes()
        return rows, want

    @staticmethod
    def gained(rows, ext, t):
        """(read bases gained on the record's left, on its right) of row t"""
        lo, hi = int(rows["read_start"][t]) - int(ext["read_start"][t]), int(ext["read_end"][t]) - int(rows["read_end"][t])
        return (hi, lo) if int(rows["reverse"][t]) else (lo, hi)


def test_empty_flanks_and_the_ends_of_a_record(env):
    """f = 0 on one side and on both; ref_start = 0 and ref_end = Lr with f > 0: g = 0, nothing to extend over"""
    dcn, O, records, _, placer = env
    c = Case(dcn, records, 1)
    T = records[0][500:560]
    for rev in (0, 1):
        c.put(b"", T, records[0][560:575], 0, 500, 560, rev)          # f = 0 on the left
        c.put(records[0][485:500], T, b"", 0, 500, 560, rev)          # ... on the right
        c.put(b"", T, b"", 0, 500, 560, rev)                           # ... on both
        c.put(b"ACGTACGTAC", records[0][:50], records[0][50:70], 0, 0, 50, rev)               # ref_start = 0, f = 10
        c.put(records[1][L1 - 80:L1 - 50], records[1][L1 - 50:], b"ACGTACGTAC", 1, L1 - 50, L1, rev)  # ref_end = Lr, f = 10
        c.put(b"ACGTACGTAC", records[0][:50], b"", 0, 0, 50, rev)
    rows, want = c.run(placer, O)
    per = [Case.gained(rows, want, t) for t in range(1, len(rows))]
    assert per[:6] == [(0, 15), (15, 0), (0, 0), (0, 20), (30, 0), (0, 0)] and per[6:] == per[:6]
    assert not want["left_edits"].any() and not want["right_edits"].any()


def test_a_flank_stops_at_the_end_of_its_record(env):
    """a read hanging over the end of record 0 while record 1 begins with the read's continuation, and the mirror of that
    at base 0 of record 1: in the store the two records lie side by side, and a match run that were not limited to the
    record would go on"""
    dcn, O, records, _, placer = env
    c = Case(dcn, records, 2)
    for rev in (0, 1):
        c.put(b"", records[0][L0 - 89:L0 - 29], records[0][L0 - 29:] + records[1][:30], 0, L0 - 89, L0 - 29, rev)
        c.put(records[0][L0 - 30:] + records[1][:20], records[1][20:80], b"", 1, 20, 80, rev)
    rows, want = c.run(placer, O)
    for t in (1, 3):
        assert Case.gained(rows, want, t) == (0, 29) and int(want["ref_end"][t]) == L0
        assert Case.gained(rows, want, t + 1) == (20, 0) and int(want["ref_start"][t + 1]) == 0


def test_a_flank_stops_at_the_end_of_its_read(env):
    """a read whose neighbours in the batch continue the reference, on either side and either strand; the first and the
    last read of the batch"""
    dcn, O, records, _, placer = env
    for rev in (0, 1):
        c = Case(dcn, records, 3 + rev, lead=False)
        pieces = [records[0][1000 + 100 * q:1100 + 100 * q] for q in range(5)]  # consecutive stretches of the record
        order = pieces[::-1] if rev else pieces  # (reverse reads lie the other way round in the stream)
        for q, piece in enumerate(pieces):
            at = 1000 + 100 * q
            c.put(piece[:20], piece[20:80], piece[80:], 0, at + 20, at + 80, rev)
        if rev:
            c.reads, c.rows = c.reads[::-1], c.rows[::-1]
        assert [revcomp(r) if rev else r for r in c.reads] == order
        rows, want = c.run(placer, O)
        assert all(Case.gained(rows, want, t) == (20, 20) for t in range(5))
        assert (want["read_start"] == 0).all() and (want["read_end"] == 100).all()


def test_left_flanks_at_the_first_bases_of_the_store(env):
    """ref_start = 0 .. 17 on record 0, whose base 0 is base 0 of the store, on both strands: the side that is read backwards
    asks for the word in front of the store there.  The read's flank is longer than the record's, and error-free as far as
    the record goes."""
    dcn, O, records, _, placer = env
    c = Case(dcn, records, 5)
    for rev in (0, 1):
        for fs in range(18):
            c.put(b"GATTACA" + records[0][:fs], records[0][fs:fs + 40], b"", 0, fs, fs + 40, rev)
            c.put(b"GATTACA" + (sub(records[0][:fs], fs // 2) if fs > 3 else records[0][:fs]), records[0][fs:fs + 40], b"", 0, fs, fs + 40, rev)
    rows, want = c.run(placer, O)
    t = 1
    for rev in (0, 1):
        for fs in range(18):
            assert Case.gained(rows, want, t) == (fs, 0) and int(want["ref_start"][t]) == 0, (rev, fs)
            t += 2
    assert (want["left_edits"] == 1).sum() >= 10


FLANKS = (15, 16, 17, 31, 32, 33, 64, 65)


def test_clean_flanks_of_every_word_length(env):
    dcn, O, records, _, placer = env
    c = Case(dcn, records, 6)
    for rev in (0, 1):
        for f in FLANKS:
            for at in (1200, 1207):
                c.put(records[0][at - f:at], records[0][at:at + 50], records[0][at + 50:at + 50 + f], 0, at, at + 50, rev)
                c.put(b"TT" + records[0][at - f:at], records[0][at:at + 50], records[0][at + 50:at + 50 + f] + b"GG", 0, at, at + 50, rev)
    rows, want = c.run(placer, O)
    fs = [f for _ in (0, 1) for f in FLANKS for _ in range(4)]
    for t, f in enumerate(fs, start=1):
        left, right = Case.gained(rows, want, t)
        assert left >= f and right >= f and left <= f + 2 and right <= f + 2, (t, f)
    assert not want["left_edits"][1::2].any()


@pytest.mark.parametrize("rev", (0, 1))
def test_one_edit_of_each_kind_at_the_seams_of_a_word(env, rev):
    """a substitution, a base of the read alone and a base of the record alone at flank bases 0, 1, 15, 16, 31, 32, f - 2 and
    f - 1 of a 48-base flank, on both sides"""
    dcn, O, records, _, placer = env
    c = Case(dcn, records, 7 + rev)
    f, at = 48, 2000
    T = records[0][at:at + 50]
    right, left = records[0][at + 50:at + 50 + f], records[0][at - f:at]
    for where in (0, 1, 15, 16, 31, 32, f - 2, f - 1):
        for kind in range(3):
            def edited(flank):  # `where` counts from the placement's edge: the flank is given in that direction
                if kind == 0:
                    return sub(flank, where)
                if kind == 1:
                    return flank[:where] + other(flank[where:where + 1]) + flank[where:]
                return flank[:where] + flank[where + 1:]
            c.put(left, T, edited(right), 0, at, at + 50, rev)
            c.put(edited(left[::-1])[::-1], T, right, 0, at, at + 50, rev)
    rows, want = c.run(placer, O)
    assert (want["left_edits"][2::2] <= 1).all() and (want["right_edits"][1::2] <= 1).all()
    assert (want["right_edits"][1::2] == 1).sum() >= 12 and (want["left_edits"][2::2] == 1).sum() >= 12  # the rest is clipped
    assert not want["left_edits"][1::2].any() and not want["right_edits"][2::2].any()


def test_both_sides_of_each_tie(env):
    """rule X5: a mismatch at f - 1 with end_bonus 4 (a tie of values: the smaller D, clipped) and 5 (extended); (1, 2) and
    (2, 1) at the record's last two bases, penalty 2 and no bonus: the larger i"""
    dcn, O, records, _, placer = env
    c = Case(dcn, records, 9)
    at = 2500
    flank = records[0][at + 50:at + 62]
    for rev in (0, 1):
        c.put(b"", records[0][at:at + 50], sub(flank, 11), 0, at, at + 50, rev)
        c.put(sub(records[0][at - 12:at], 0), records[0][at:at + 50], b"", 0, at, at + 50, rev)
    rows, want = c.run(placer, O)
    assert [Case.gained(rows, want, t) for t in range(1, 5)] == [(0, 11), (11, 0)] * 2 and not want["left_edits"].any() and not want["right_edits"].any()
    rows, want = c.run(placer, O, end_bonus=5)
    assert [Case.gained(rows, want, t) for t in range(1, 5)] == [(0, 12), (12, 0)] * 2
    assert want["right_edits"][1::2].tolist() == [1, 1] and want["left_edits"][2::2].tolist() == [1, 1]
    c = Case(dcn, records, 10)
    assert records[1][-2:] == b"CA"
    for rev in (0, 1):
        c.put(b"", records[1][L1 - 52:L1 - 2], b"AC", 1, L1 - 52, L1 - 2, rev)
    rows, want = c.run(placer, O, penalty=2, end_bonus=0)
    for t in (1, 2):
        assert Case.gained(rows, want, t) == (0, 2) and int(want["ref_end"][t]) == L1 - 1 and int(want["right_edits"][t]) == 1
    rows, want = c.run(placer, O, penalty=3, end_bonus=0)  # ... at penalty 3 neither cell is worth its edit
    assert all(Case.gained(rows, want, t) == (0, 0) for t in (1, 2))


def test_invalid_bases_and_case(env):
    """N against N, N against a base, a base against N, and lower case on either side"""
    dcn, O, records, _, placer = env
    c = Case(dcn, records, 11)
    for rev in (0, 1):
        c.put(b"", records[1][40:90], records[1][90:130], 1, 40, 90, rev)                                     # N against N
        c.put(b"", records[1][40:90], records[1][90:100] + b"ACG" + records[1][103:130], 1, 40, 90, rev)      # a base against N
        c.put(b"", records[0][40:90], records[0][90:100] + b"NNN" + records[0][103:130], 0, 40, 90, rev)      # N against a base
        c.put(records[1][120:180], records[1][180:190], records[1][190:280].upper(), 1, 180, 190, rev)         # lower case in the record
        c.put(records[0][120:180].lower(), records[0][180:190], records[0][190:280].lower(), 0, 180, 190, rev)  # ... in the read
    rows, want = c.run(placer, O)
    for t0 in (1, 6):
        assert want["right_edits"][t0:t0 + 3].tolist() == [3, 3, 3] and all(Case.gained(rows, want, t)[1] == 40 for t in range(t0, t0 + 3))
        assert [Case.gained(rows, want, t) for t in (t0 + 3, t0 + 4)] == [(60, 90), (60, 90)]
        assert not want["right_edits"][t0 + 3:t0 + 5].any()


def test_max_edits(env):
    """three mismatches in a flank: max_edits 0 and 1 exclude the better cell, 2 still does, and from 3 on the cap no longer
    binds"""
    dcn, O, records, _, placer = env
    c = Case(dcn, records, 12)
    at = 3000
    flank = sub(sub(sub(records[0][at + 50:at + 110], 10), 25), 40)
    for rev in (0, 1):
        c.put(b"", records[0][at:at + 50], flank, 0, at, at + 50, rev)
        c.put(sub(sub(sub(records[0][at - 60:at], 49), 34), 19), records[0][at:at + 50], b"", 0, at, at + 50, rev)  # (10, 25 and 40 bases from the edge)
    seen = []
    for max_edits in (0, 1, 2, 3, 4, 1023):
        rows, want = c.run(placer, O, max_edits=max_edits)
        seen.append([sum(Case.gained(rows, want, t)) for t in range(1, 5)])
    assert seen == [[10] * 4, [25] * 4, [40] * 4, [60] * 4, [60] * 4, [60] * 4]


@pytest.mark.parametrize("D", (31, 32, 33))
def test_wavefront_widths(env, D):
    """D* of 31, 32 and 33 (63, 65 and 67 diagonals: more than the 16 lanes of a flank, and than 64) at penalty 2 and 3 on
    flanks of a few hundred bases: substitutions ten bases apart, with a base of the read alone and one of the record alone
    among them"""
    dcn, O, records, _, placer = env
    c = Case(dcn, records, 13 + D)
    at = 500
    clean = records[0][at + 50:at + 50 + 10 * D + 40]
    flank = clean
    for q in range(D - 2):
        flank = sub(flank, 10 * q + 25)
    flank = flank[:7] + flank[8:15] + other(flank[15:16]) + flank[15:]  # one deletion, one insertion
    for rev in (0, 1):
        c.put(b"", records[0][at:at + 50], flank, 0, at, at + 50, rev)
        c.put(flank, records[0][at + 50 + len(clean):at + 100 + len(clean)], b"", 0, at + 50 + len(clean), at + 100 + len(clean), rev)
    for penalty in (2, 3):
        rows, want = c.run(placer, O, penalty=penalty)
        assert want["right_edits"][1::2].tolist() == [D, D] and want["left_edits"][2::2].tolist() == [D, D]
        assert all(sum(Case.gained(rows, want, t)) == len(flank) for t in range(1, 5))


def test_three_thousand_bases_and_junk(env):
    """a 3,000-base flank with 10 % mixed edits, and a 2,000-base flank that has nothing to do with the record"""
    dcn, O, records, _, placer = env
    c = Case(dcn, records, 14)
    flank = VW.mutate_mixed(c.rng, records[0][60:3060], 0.10)
    junk = random_reads(c.rng, 1, 2000, 2000)[0]
    c.put(b"", records[0][10:60], flank, 0, 10, 60, 0)
    c.put(flank, records[0][3060:3110], b"", 0, 3060, 3110, 1)
    c.put(b"", records[0][10:60], junk, 0, 10, 60, 1)
    c.put(junk, records[0][3060:3110], b"", 0, 3060, 3110, 0)
    rows, want = c.run(placer, O)
    assert Case.gained(rows, want, 1)[1] > 2900 and Case.gained(rows, want, 2)[0] > 2900
    assert 200 < int(want["right_edits"][1]) < 500 and 200 < int(want["left_edits"][2]) < 500
    assert sum(Case.gained(rows, want, 3)) < 30 and sum(Case.gained(rows, want, 4)) < 30
    rows, want = c.run(placer, O, penalty=2, end_bonus=65535)  # ... the bonus buys the junk: the cap of 1023 edits decides
    assert int(want["right_edits"][1]) < 500


def test_row_counts_and_row_offsets(env):
    """0 rows; a read with 8 rows, out of order; 1, 255, 256 and 257 rows; UNPLACED rows among placed ones; the three row
    types' strides"""
    dcn, O, records, _, placer = env
    rng = np.random.default_rng(15)
    F = dcn.filter
    read = records[0][100:900]
    reads = [random_reads(rng, 1, 37, 37)[0], read, b"", revcomp(read)]
    b, o = O.concat_reads(reads)
    for dtype in (F.PLACEMENT_DTYPE, F.SPLIT_PLACEMENT_DTYPE, F.PAIR_PLACEMENT_DTYPE):
        xrows, ext = placer.extend_batch(b, o, np.zeros(0, dtype), row_offsets=np.zeros(5, np.uint64))
        assert len(xrows) == 0 == len(ext) and xrows.dtype == dtype
        parts = [(q + 30, q + 70) for q in (700, 0, 300, 600, 100, 500, 200, 400)]  # 8 rows, not in read order
        rows = [VW.make_row(dtype, 0, 0, q0, q1, 100 + q0, 100 + q1) for q0, q1 in parts]
        rows += [VW.make_row(dtype, 0, 1, 800 - q1, 800 - q0, 100 + q0, 100 + q1) for q0, q1 in parts[:3]]
        rows.insert(3, VW.make_row(dtype, UNPLACED, 7, 9, 3, 5, 1))  # (an unplaced row's other fields are not looked at)
        rows = np.concatenate(rows)
        rows["votes"] = np.arange(len(rows)) + 5  # (the other fields of a row come back as they were)
        ro = np.array([0, 0, 9, 9, 12], np.uint64)
        got_rows, got = placer.extend_batch(b, o, rows, row_offsets=ro)
        want_rows, want = XW.extend_rows(reads, records, rows, row_offsets=ro)
        assert got.tobytes() == want.tobytes() and got_rows.tobytes() == want_rows.tobytes()
        assert got[3].tolist() == (9, 3, 5, 1, 0, 0)  # rule X7
        keep = np.arange(len(rows)) != 3
        assert (got["read_start"][keep] == 0).all() and (got["read_end"][keep] == 800).all()  # every row grows to the whole read
    for n in (1, 255, 256, 257):
        reads = [records[1][(7 * i) % 1500:(7 * i) % 1500 + 60] for i in range(n)]
        rows = np.concatenate([VW.make_row(F.SPLIT_PLACEMENT_DTYPE, 1 if i % 5 else UNPLACED, 0, 10, 50, (7 * i) % 1500 + 10, (7 * i) % 1500 + 50)
                               for i in range(n)])
        b, o = O.concat_reads(reads)
        got = placer.extend_batch(b, o, rows)[1]
        assert got.tobytes() == XW.extend_rows(reads, records, rows)[1].tobytes()
        assert got.tobytes() == placer.extend_batch(b, o, rows, row_offsets=np.arange(n + 1, dtype=np.uint64))[1].tobytes()


def test_host_validation_names_the_row(env, oracle):
    """every error of a row, with its number in the message, the errors of row_offsets and of the parameters: all before any
    device work, with dcn_verify_batch's messages"""
    dcn, O, records, _, placer = env
    D = dcn.filter.PLACEMENT_DTYPE
    reads = [records[0][:100], records[0][100:300], records[1][:50]]
    b, o = O.concat_reads(reads)
    good = [VW.make_row(D, 0, 0, 0, 100, 0, 100), VW.make_row(D, 0, 0, 0, 200, 100, 300), VW.make_row(D, 1, 1, 0, 50, 0, 50)]
    for at, bad, word in ((1, VW.make_row(D, 2, 0, 0, 10, 0, 10), "row 1: record 2 of 2 added"),
                          (2, VW.make_row(D, 1, 2, 0, 10, 0, 10), "row 2: reverse must be 0 or 1"),
                          (0, VW.make_row(D, 0, 0, 11, 10, 0, 10), "row 0: read_start is behind read_end"),
                          (1, VW.make_row(D, 0, 0, 0, 201, 0, 10), "row 1: read_end 201 is past the read's 200 bases"),
                          (2, VW.make_row(D, 1, 0, 0, 10, 11, 10), "row 2: ref_start is behind ref_end"),
                          (2, VW.make_row(D, 1, 0, 0, 10, 0, 1778), "row 2: ref_end 1778 is past the record's 1777 bases"),
                          (0, VW.make_row(D, 0, 0, 0, 10, 3980, 3990), "row 0: ref_end 3990 is past the record's 3989 bases")):
        rows = list(good)
        rows[at] = bad
        for call in (placer.extend_batch, placer.verify_batch):
            with pytest.raises(dcn.DeaconHipError) as e:
                call(b, o, np.concatenate(rows))
            assert e.value.code == dcn._native.DCN_ERR_ARG and word in e.value.message, e.value.message
    rows = np.concatenate(good)
    for ro, word in (([0, 2, 1, 3], "non-decreasing"), ([0, 1, 2, 2], "end at n_rows"), ([0, 1, 2, 4], "end at n_rows"), ([1, 1, 2, 3], "row_offsets[0]")):
        with pytest.raises(dcn.DeaconHipError) as e:
            placer.extend_batch(b, o, rows, row_offsets=np.array(ro, np.uint64))
        assert e.value.code == dcn._native.DCN_ERR_ARG and word in e.value.message, e.value.message
    with pytest.raises(dcn.DeaconHipError) as e:
        placer.extend_batch(b, o, rows[:2])
    assert "n_rows must equal n_reads" in e.value.message
    for kw, word in ((dict(penalty=1), "params.penalty must be 2..255"), (dict(penalty=256), "params.penalty must be 2..255"),
                     (dict(end_bonus=65536), "params.end_bonus must be 0..65535"), (dict(max_edits=1024), "params.max_edits must be 0..1023")):
        with pytest.raises(dcn.DeaconHipError) as e:
            placer.extend_batch(b, o, rows, **kw)
        assert e.value.code == dcn._native.DCN_ERR_ARG and word in e.value.message, e.value.message
    # out == NULL with rows: refused, behind the checks of the rows (the header says so)
    import ctypes as C
    N, F = dcn._native, dcn.filter
    bb, oo, n_reads = F._batch(b, o)
    prm = N.ExtendParams(6, 4, 1023, rows.dtype.itemsize, (C.c_uint32 * 2)(0, 0))
    for these, word in ((rows, b"out is NULL"), (np.concatenate([good[0], VW.make_row(D, 0, 0, 0, 201, 0, 10), good[2]]), b"row 1: read_end 201")):
        assert N.lib().dcn_extend_batch(placer._h, placer.anchor_map._h, F._ptr(bb), F._ptr(oo), n_reads, C.byref(prm), None, F._ptr(these), 3, None) == N.DCN_ERR_ARG
        assert word in N.lib().dcn_last_error()
    plain = VW.build_map(oracle, dcn, records[:1], keep_bases=False)
    bare = dcn.Placer(plain, max_batch_bases=1 << 16, max_batch_reads=1 << 8)
    with pytest.raises(dcn.DeaconHipError) as e:
        bare.extend_batch(b, o, rows)
    assert "keeps no bases" in e.value.message
    bare.close()
    plain.close()
    got = placer.extend_batch(b, o, rows)[1]
    assert got.tobytes() == XW.extend_rows(reads, records, rows)[1].tobytes()

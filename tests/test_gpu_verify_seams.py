"""The seams of dcn_verify_batch and its kernel (verify.hip), with rows written by hand: no hashing decides anything here.
The map keeps the bases of two short records; every case is a few hundred rows at most and is compared with the model of
tests/_verify_worker.py exactly (a plain dynamic programme: it has no wavefront and shares nothing with the kernel).

A case is built by put(): the read is flank + S + flank, so that read_start takes any value mod 32, behind a first read of
37 bases, so that no read of the batch starts on a word of the stream."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _verify_worker as VW
from conftest import random_reads, revcomp

pytestmark = pytest.mark.gpu

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_verify_worker.py")
OVER, UNPLACED = VW.OVER, VW.UNPLACED


def make_records():
    rng = np.random.default_rng(1311)
    a, b = random_reads(rng, 1, 3989, 3989)[0], bytearray(random_reads(rng, 1, 1777, 1777)[0])
    b[100:103] = b"NNN"                      # N against N, N against a base
    b[200:260] = bytes(b[200:260]).lower()   # lower case in the record
    b[400:520] = b"ACG" * 40                 # a tandem repeat
    b[700:760] = b"A" * 60                   # a homopolymer
    return [a, bytes(b)]  # (3989 % 16 != 0: the second record starts mid-word of the store)


@pytest.fixture(scope="module")
def env(dcn, oracle):
    records = make_records()
    amap = VW.build_map(oracle, dcn, records)
    placer = dcn.Placer(amap, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    yield dcn, oracle, records, amap, placer
    placer.close()
    amap.close()


class Case:
    """reads and hand-written rows of one call"""

    def __init__(self, dcn, records, seed, dtype=None):
        self.dcn, self.records, self.rng = dcn, records, np.random.default_rng(seed)
        self.dtype = dtype or dcn.filter.PLACEMENT_DTYPE
        self.reads, self.rows = [random_reads(self.rng, 1, 37, 37)[0]], [VW.make_row(self.dtype, UNPLACED, 0, 0, 0, 0, 0)]

    def put(self, S, R, a, b, rev=0, pre=None):
        """a read that holds S (as the row's strand reads it) at offset pre, placed on records[R][a:b]"""
        pre = int(self.rng.integers(0, 40)) if pre is None else pre
        flank = random_reads(self.rng, 2, pre, pre)[0], random_reads(self.rng, 1, 0, 20)[0]
        self.reads.append(flank[0] + (revcomp(S) if rev else S) + flank[1])
        self.rows.append(VW.make_row(self.dtype, R, rev, pre, pre + len(S), a, b))

    def run(self, placer, oracle, **kw):
        rows = np.concatenate(self.rows)
        b, o = oracle.concat_reads(self.reads)
        got = placer.verify_batch(b, o, rows, **kw)
        want = VW.verify_rows(self.reads, self.records, rows, **kw)
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, [(int(i), int(got[i]), int(want[i]), rows[i]) for i in bad[:5]]
        return want[1:]  # (without the first read's unplaced row)


def test_every_offset_mod_32_on_both_strands(env):
    """1. read_start and ref_start at every value mod 32, both strands, two edits each"""
    dcn, O, records, _, placer = env
    for rev in (0, 1):
        c = Case(dcn, records, 10 + rev)
        for rs in range(32):
            for fs in range(32):
                a = 640 + fs
                T = records[0][a:a + 70]
                c.put(VW.edit(c.rng, T, n_sub=1, n_ins=(rs + fs) % 2, n_del=(rs + fs + 1) % 2), 0, a, a + 70, rev, pre=rs)
        want = c.run(placer, O)
        assert (want <= 2).all() and (want > 0).any()


LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65)


def test_interval_lengths(env):
    """2. every pair of lengths on the two sides, m != n and m == n: S a prefix of T or T a prefix of S (d = |n - m|), and
    unrelated bases; E = the longer side (max_permille = 1000), and once E = 0"""
    dcn, O, records, _, placer = env
    c = Case(dcn, records, 20)
    for m in LENGTHS:
        for n in LENGTHS:
            for rev in (0, 1):
                a = 1000 + (m * 7 + n) % 32
                longer = records[0][a:a + max(m, n)]
                c.put(longer[:m], 0, a, a + n, rev)
                c.put(random_reads(c.rng, 1, m, m)[0], 0, a, a + n, rev)
    want = c.run(placer, O, max_permille=1000)
    assert sorted(set(want[0::2].tolist())) == sorted({abs(m - n) for m in LENGTHS for n in LENGTHS})
    want0 = c.run(placer, O, max_permille=0)
    assert set(want0.tolist()) == {0, OVER}


def test_one_edit_at_the_seams_of_a_word(env):
    """3. one substitution, one inserted and one deleted base at the first base, the last base and bases 15, 16, 31, 32"""
    dcn, O, records, _, placer = env
    c = Case(dcn, records, 30)
    for at in (0, 15, 16, 31, 32, 63):
        for rev in (0, 1):
            for pre in (0, 5, 16, 31):
                T = records[0][2000 + pre:2064 + pre]
                sub = bytearray(T)
                sub[at] = ord("A") if T[at:at + 1] != b"A" else ord("C")
                c.put(bytes(sub), 0, 2000 + pre, 2064 + pre, rev, pre=pre)
                c.put(T[:at] + T[at + 1:], 0, 2000 + pre, 2064 + pre, rev, pre=pre)
                c.put(T[:at] + (b"G" if T[at:at + 1] != b"G" else b"T") + T[at:], 0, 2000 + pre, 2064 + pre, rev, pre=pre)
    want = c.run(placer, O)
    assert (want == 1).all()


def test_invalid_bases_and_case(env):
    """4. N against N and N against a base cost one each; lower case equals upper case on either side"""
    dcn, O, records, _, placer = env
    c = Case(dcn, records, 40)
    r1 = records[1]
    for rev in (0, 1):
        c.put(r1[60:160], 1, 60, 160, rev)                                  # NNN against NNN: 3
        c.put(r1[60:100] + b"ACG" + r1[103:160], 1, 60, 160, rev)           # bases against NNN: 3
        c.put(r1[300:330] + b"N" + r1[331:380], 1, 300, 380, rev)           # N against a base: 1
        c.put(r1[300:330] + b"R-" + r1[332:380], 1, 300, 380, rev)          # other bytes outside the alphabet: 2
        c.put(r1[180:300].upper(), 1, 180, 300, rev)                        # upper case against the record's lower case: 0
        c.put(r1[180:300].lower(), 1, 180, 300, rev)                        # 0
        c.put(records[0][50:150].lower(), 0, 50, 150, rev)                  # 0
        c.put(b"N" * 40, 1, 60, 100, rev)                                   # 40
    want = c.run(placer, O, max_permille=1000)
    assert want.tolist() == [3, 3, 1, 2, 0, 0, 0, 40] * 2


def spaced_subs(T, count):
    """T with `count` substitutions spread evenly"""
    s = bytearray(T)
    for i in range(count):
        at = (2 * i + 1) * len(T) // (2 * count)
        s[at] = ord("A") if s[at] != ord("A") else ord("C")
    return bytes(s)


def test_threshold(env):
    """5. d == E and d == E + 1; E = 0 with identical bases and with one mismatch; the permille floor: max(m, n) = 199 at
    permille 5 gives E = 0, 200 gives E = 1; max_permille = 0"""
    dcn, O, records, _, placer = env
    c = Case(dcn, records, 50)
    T = records[0][300:700]
    for rev in (0, 1):
        c.put(spaced_subs(T, 7), 0, 300, 700, rev)
        c.put(T, 0, 300, 700, rev)
        c.put(spaced_subs(T, 1), 0, 300, 700, rev)
    for max_edits, want in ((7, [7, 0, 1]), (6, [OVER, 0, 1]), (8, [7, 0, 1]), (1, [OVER, 0, 1]), (0, [OVER, 0, OVER])):
        assert c.run(placer, O, max_edits=max_edits, max_permille=1000).tolist() == want * 2
    assert c.run(placer, O, max_permille=0).tolist() == [OVER, 0, OVER] * 2
    c = Case(dcn, records, 51)
    for ln in (199, 200):
        for rev in (0, 1):
            T = records[0][900:900 + ln]
            c.put(T, 0, 900, 900 + ln, rev)
            c.put(spaced_subs(T, 1), 0, 900, 900 + ln, rev)
            c.put(spaced_subs(T, 1)[:ln - 3], 0, 900, 900 + ln, rev)  # the longer side counts: max(m, n)
    assert c.run(placer, O, max_permille=5).tolist() == [0, OVER, OVER] * 2 + [0, 1, OVER] * 2


@pytest.mark.parametrize("E", [31, 32, 33, 63, 64, 65])
def test_wavefront_widths(env, E):
    """6. d at E = 31 .. 65: the diagonals of the last scores cross one and two waves' worth of lanes.  Substitutions spread
    over 700 bases (d is what the model says, E is set to it and to one less), and a pure gap of E and of E + 1 bases"""
    dcn, O, records, _, placer = env
    c = Case(dcn, records, 60 + E)
    T = records[0][1200:1900]
    for rev in (0, 1):
        c.put(spaced_subs(T, E), 0, 1200, 1900, rev)
        c.put(VW.mutate_mixed(c.rng, T, E / 700), 0, 1200, 1900, rev)
        c.put(T[:700 - E], 0, 1200, 1900, rev)       # |n - m| == E
        c.put(T + random_reads(c.rng, 1, E, E)[0], 0, 1200, 1900, rev)
        c.put(T[:700 - E - 1], 0, 1200, 1900, rev)   # |n - m| == E + 1
        c.put(T[E:], 0, 1200, 1900, rev)             # the gap at the front
    d = c.run(placer, O, max_permille=1000)
    assert d[0] == d[6] == E and d[2] == d[3] == d[5] == E and d[4] == E + 1
    for max_edits in (E - 1, E, E + 1):
        want = c.run(placer, O, max_edits=max_edits, max_permille=1000)
        assert want.tolist() == [x if x <= max_edits else OVER for x in d.tolist()]


def test_the_cap_on_three_thousand_bases(env):
    """7. max_edits = 1023 on a 3,000-base interval: mutated at about 30 % (d near 700: the model says what it is), at 40 %
    and at 60 % (OVER), both strands"""
    dcn, O, records, _, placer = env
    c = Case(dcn, records, 70)
    T = records[0][500:3500]
    for rate in (0.3, 0.4, 0.6):
        for rev in (0, 1):
            c.put(VW.mutate_mixed(c.rng, T, rate), 0, 500, 3500, rev)
    want = c.run(placer, O, max_edits=1023, max_permille=1000)
    assert 500 < want[0] < 1000 and 500 < want[1] < 1000 and want[4] == want[5] == OVER
    assert c.run(placer, O, max_edits=1023, max_permille=200).tolist() == [x if x <= 600 else OVER for x in want.tolist()]


def test_repeats_have_one_distance(env):
    """8. a tandem repeat and a homopolymer with a length change: many optimal alignments, one distance"""
    dcn, O, records, _, placer = env
    c = Case(dcn, records, 80)
    r1 = records[1]
    for rev in (0, 1):
        for units in (-3, -1, 1, 2):
            c.put(r1[380:400] + b"ACG" * (40 + units) + r1[520:540], 1, 380, 540, rev)
        for extra in (-5, -1, 1, 4):
            c.put(r1[680:700] + b"A" * (60 + extra) + r1[760:790], 1, 680, 790, rev)
    want = c.run(placer, O)
    assert want.tolist() == [9, 3, 3, 6, 5, 1, 1, 4] * 2


def test_ends_of_the_records(env):
    """9. rows that touch base 0 and the last base of the first and of the last record of the add call; whole records"""
    dcn, O, records, amap, placer = env
    c = Case(dcn, records, 90)
    for R, rec in enumerate(records):
        L = len(rec)
        for rev in (0, 1):
            c.put(VW.edit(c.rng, rec[:90], n_sub=2), R, 0, 90, rev)
            c.put(VW.edit(c.rng, rec[L - 90:], n_del=2), R, L - 90, L, rev)
            c.put(VW.edit(c.rng, rec, n_sub=3, n_ins=2), R, 0, L, rev, pre=0)
            c.put(b"", R, L, L, rev)
            c.put(b"", R, 0, 0, rev)
    c.run(placer, O, max_permille=1000)
    for R, rec in enumerate(records):
        assert amap.fetch(R, 0, len(rec)) == VW.fetched_text(rec)
        assert amap.fetch(R, len(rec) - 33, 33) == VW.fetched_text(rec[-33:]) and amap.fetch(R, len(rec), 0) == b""


def test_store_grown_twice():
    """10. DCN_ANCHOR_STORE_BASES = 64 in a process of its own: the store grows with every add call but the first"""
    p = subprocess.run([sys.executable, WORKER, "growth"], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, DCN_ANCHOR_STORE_BASES="64"))
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "verify growth ok" in p.stdout


def test_row_counts_and_row_offsets(env):
    """11. 0 rows; a read with 8 rows; rows whose order within a read is not their order on the read; row counts 1, 255, 256
    and 257; UNPLACED rows among placed ones; the three row types' strides"""
    dcn, O, records, _, placer = env
    rng = np.random.default_rng(110)
    F = dcn.filter
    read = records[0][100:900]
    reads = [random_reads(rng, 1, 37, 37)[0], read, b"", revcomp(read)]
    b, o = O.concat_reads(reads)
    for dtype in (F.PLACEMENT_DTYPE, F.SPLIT_PLACEMENT_DTYPE, F.PAIR_PLACEMENT_DTYPE):
        assert len(placer.verify_batch(b, o, np.zeros(0, dtype), row_offsets=np.zeros(5, np.uint64))) == 0
        parts = [(q, q + 100) for q in (700, 0, 300, 600, 100, 500, 200, 400)]  # 8 rows, not in read order
        rows = [VW.make_row(dtype, 0, 0, q0, q1, 100 + q0, 100 + q1 - (q0 // 100) % 3) for q0, q1 in parts]
        rows += [VW.make_row(dtype, 0, 1, 800 - q1, 800 - q0, 100 + q0, 100 + q1) for q0, q1 in parts[:3]]
        rows.insert(3, VW.make_row(dtype, UNPLACED, 7, 9, 3, 5, 1))  # (an unplaced row's other fields are not looked at)
        rows = np.concatenate(rows)
        ro = np.array([0, 0, 9, 9, 12], np.uint64)
        got = placer.verify_batch(b, o, rows, row_offsets=ro)
        want = VW.verify_rows(reads, records, rows, row_offsets=ro)
        assert got.tolist() == want.tolist() and want[3] == UNPLACED and (np.delete(want, 3) <= 2).all()
    for n in (1, 255, 256, 257):
        reads = [records[1][(7 * i) % 1500:(7 * i) % 1500 + 60] for i in range(n)]
        rows = np.concatenate([VW.make_row(F.SPLIT_PLACEMENT_DTYPE, 1 if i % 5 else UNPLACED, 0, 0, 60, (7 * i) % 1500 + i % 2, (7 * i) % 1500 + 60)
                               for i in range(n)])
        b, o = O.concat_reads(reads)
        got = placer.verify_batch(b, o, rows)
        assert got.tolist() == VW.verify_rows(reads, records, rows).tolist()
        assert got.tolist() == placer.verify_batch(b, o, rows, row_offsets=np.arange(n + 1, dtype=np.uint64)).tolist()


def test_host_validation_names_the_row(env):
    """12. every error of a row, with its number in the message, and the errors of row_offsets: all before any device work"""
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
        with pytest.raises(dcn.DeaconHipError) as e:
            placer.verify_batch(b, o, np.concatenate(rows))
        assert e.value.code == dcn._native.DCN_ERR_ARG and word in e.value.message, e.value.message
    rows = np.concatenate(good)
    for ro, word in (([0, 2, 1, 3], "non-decreasing"), ([0, 1, 2, 2], "end at n_rows"), ([0, 1, 2, 4], "end at n_rows"), ([1, 1, 2, 3], "row_offsets[0]")):
        with pytest.raises(dcn.DeaconHipError) as e:
            placer.verify_batch(b, o, rows, row_offsets=np.array(ro, np.uint64))
        assert e.value.code == dcn._native.DCN_ERR_ARG and word in e.value.message, e.value.message
    with pytest.raises(dcn.DeaconHipError) as e:
        placer.verify_batch(b, o, rows[:2])
    assert "n_rows must equal n_reads" in e.value.message
    assert placer.verify_batch(b, o, rows).tolist() == [0, 0, VW.verify_rows(reads, records, rows)[2]]

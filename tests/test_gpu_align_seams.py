"""The seams of dcn_align_batch and its kernel (align.hip), with rows written by hand: no hashing decides anything here.
The map keeps the bases of two short records, the second starting mid-word of the store; every case is a few hundred rows at
most and is compared with the model of tests/_align_worker.py run for run (a full table walked by rule A3: it has no
wavefront and shares nothing with the kernel).

A case is built by put(): the read is flank + S + flank, so that read_start takes any value mod 32, behind a first read of
37 bases, so that no read of the batch starts on a word of the stream."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _align_worker as AW
import _verify_worker as VW
from conftest import random_reads, revcomp

pytestmark = pytest.mark.gpu

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_align_worker.py")
OVER, UNPLACED = VW.OVER, VW.UNPLACED


def make_records():
    rng = np.random.default_rng(1411)
    a, b = random_reads(rng, 1, 3989, 3989)[0], bytearray(random_reads(rng, 1, 1777, 1777)[0])
    b[100:103] = b"NNN"
    b[200:260] = bytes(b[200:260]).lower()
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
        """-> (edits, [the CIGAR text of each row]) without the first read's unplaced row, after comparing with the model"""
        rows = np.concatenate(self.rows)
        b, o = oracle.concat_reads(self.reads)
        got = placer.align_batch(b, o, rows, **kw)
        want = AW.align_rows(self.reads, self.records, rows, **kw)
        AW.assert_same(got, want, rows)
        assert got[0].tolist() == placer.verify_batch(b, o, rows, **kw).tolist()
        return want[0][1:], [AW.cigar_text(want[2][int(want[1][i]):int(want[1][i + 1])]) for i in range(1, len(rows))]


def other(base, *avoid):
    """a letter that is none of the given bases"""
    return next(bytes([x]) for x in b"ACGT" if all(bytes([x]) != y.upper() for y in (base,) + avoid))


def text(*runs):
    """(len, op) ... -> CIGAR text without the empty runs"""
    return "".join("%d%s" % r for r in runs if r[0] > 0)


def test_one_edit_at_the_seams_of_a_word(env):
    """one substitution, one inserted and one deleted base at bases 0, 15, 16, 31, 32 and the last, on both strands, at read
    offsets that leave the interval at four offsets of a word.  The substitution's CIGAR is written out here; a gap's
    depends on its neighbours (rule A3 moves it within a run of equal bases) and is the model's"""
    dcn, O, records, _, placer = env
    c = Case(dcn, records, 30)
    expect = []
    for at in (0, 15, 16, 31, 32, 63):
        for rev in (0, 1):
            for pre in (0, 5, 16, 31):
                a = 2000 + pre
                T = records[0][a:a + 64]
                c.put(T[:at] + other(T[at:at + 1]) + T[at + 1:], 0, a, a + 64, rev, pre=pre)
                expect.append(text((at, "="), (1, "X"), (63 - at, "=")))
                c.put(T[:at] + T[at + 1:], 0, a, a + 64, rev, pre=pre)
                expect.append(None)
                c.put(T[:at] + other(T[at:at + 1], T[at - 1:at] if at else T[at:at + 1]) + T[at:], 0, a, a + 64, rev, pre=pre)
                expect.append(None)
    edits, cigars = c.run(placer, O)
    assert (edits == 1).all()
    for want, got in zip(expect, cigars):
        assert want is None or want == got
    assert all("D" in x for x in cigars[1::3]) and all("I" in x for x in cigars[2::3])


def test_two_edits_adjacent_and_one_apart(env):
    """XI, IX, ID, DI, XD, DX pairs, adjacent and one base apart: the order of preference of rule A3 decides what is printed"""
    dcn, O, records, _, placer = env
    c = Case(dcn, records, 31)
    for p in (15, 16, 31, 40):
        for rev in (0, 1):
            for gap in (0, 1):
                a = 2200 + p
                T = records[0][a:a + 80]
                q = p + 1 + gap
                X = lambda s, at: s[:at] + other(s[at:at + 1]) + s[at + 1:]  # noqa: E731
                I = lambda s, at: s[:at] + other(s[at:at + 1], s[at - 1:at]) + s[at:]  # noqa: E731
                Dl = lambda s, at: s[:at] + s[at + 1:]  # noqa: E731
                c.put(I(X(T, p), q), 0, a, a + 80, rev)    # XI
                c.put(X(I(T, p), q + 1), 0, a, a + 80, rev)  # IX
                c.put(Dl(I(T, p), q + 1), 0, a, a + 80, rev)  # ID
                c.put(I(Dl(T, p), q - 1), 0, a, a + 80, rev)  # DI
                c.put(Dl(X(T, p), q), 0, a, a + 80, rev)   # XD
                c.put(X(Dl(T, p), q - 1), 0, a, a + 80, rev)  # DX
    edits, cigars = c.run(placer, O)
    assert set(edits.tolist()) <= {1, 2} and (edits == 2).sum() > len(edits) // 2
    assert any("X" in x and "I" in x for x in cigars) and any("I" in x and "D" in x for x in cigars) and any("2X" in x for x in cigars)


def test_preference_order_on_repeats(env):
    """a tandem repeat and a homopolymer with a length change, and AC against CA: many optimal alignments, one printed"""
    dcn, O, records, _, placer = env
    c = Case(dcn, records, 32)
    r1 = records[1]
    for rev in (0, 1):
        for units in (-3, -1, 1, 2):
            c.put(r1[380:400] + b"ACG" * (40 + units) + r1[520:540], 1, 380, 540, rev)
        for extra in (-5, -1, 1, 4):
            c.put(r1[680:700] + b"A" * (60 + extra) + r1[760:790], 1, 680, 790, rev)
        T = r1[900:940]
        swap = other(T[20:21])
        c.put(T[:19] + swap + T[19:20] + T[21:], 1, 900, 940, rev)  # (two bases in the other order, or two substitutions)
    edits, cigars = c.run(placer, O)
    assert edits.tolist()[:8] == [9, 3, 3, 6, 5, 1, 1, 4]
    assert all(x.count("D") == 1 and "I" not in x and "X" not in x for x in cigars[0:2] + cigars[4:6])  # one run of D
    assert all(x.count("I") == 1 and "D" not in x and "X" not in x for x in cigars[2:4] + cigars[6:8])


def test_empty_sides(env):
    """pure gaps: m = 0 (n D), n = 0 (m I), and m = n = 0 (no run), on both strands; lengths around a word"""
    dcn, O, records, _, placer = env
    c = Case(dcn, records, 33)
    expect = []
    for ln in (1, 15, 16, 17, 33, 64):
        for rev in (0, 1):
            c.put(b"", 0, 1000, 1000 + ln, rev)
            expect.append("%dD" % ln)
            c.put(records[0][1000:1000 + ln], 0, 1000, 1000, rev)
            expect.append("%dI" % ln)
    c.put(b"", 0, 1000, 1000, 0)
    c.put(b"", 1, 1777, 1777, 1)
    expect += ["", ""]
    edits, cigars = c.run(placer, O, max_permille=1000)
    assert cigars == expect and edits.tolist()[-2:] == [0, 0]


def spaced_subs(T, count):
    s = bytearray(T)
    for i in range(count):
        at = (2 * i + 1) * len(T) // (2 * count)
        s[at] = ord("A") if s[at] != ord("A") else ord("C")
    return bytes(s)


@pytest.mark.parametrize("d", [0, 1, 31, 32, 33, 63, 64, 65])
def test_score_seams(env, d):
    """d where the diagonals of the last scores cross one and two waves' worth of lanes, and the s * s index of the trace
    around them: substitutions spread over 700 bases, mixed edits near that rate, and pure gaps of d at either end and on
    either side"""
    dcn, O, records, _, placer = env
    c = Case(dcn, records, 60 + d)
    T = records[0][1200:1900]
    for rev in (0, 1):
        c.put(spaced_subs(T, d) if d else T, 0, 1200, 1900, rev)
        c.put(VW.mutate_mixed(c.rng, T, d / 700), 0, 1200, 1900, rev)
        c.put(T[:700 - d], 0, 1200, 1900, rev)       # n - m == d
        c.put(T + random_reads(c.rng, 1, d, d)[0], 0, 1200, 1900, rev)
        c.put(T[d:], 0, 1200, 1900, rev)             # the gap at the front
    edits, cigars = c.run(placer, O, max_permille=1000)
    assert edits[0] == edits[5] == d and edits[2] == edits[4] == d and edits[3] <= d
    assert cigars[0].count("X") == d and cigars[0].count("=") == (d + 1 if d else 1)  # 2 d + 1 runs: the bound is met
    if d:
        assert cigars[2] == "%d=%dD" % (700 - d, d)


def test_threshold_and_mixed_rows(env):
    """d = E and d = E + 1: the second is OVER and has no run; an UNPLACED and an OVER row between aligned ones leave the
    offsets right"""
    dcn, O, records, _, placer = env
    c = Case(dcn, records, 50)
    T = records[0][300:700]
    for rev in (0, 1):
        c.put(spaced_subs(T, 7), 0, 300, 700, rev)
        c.put(T, 0, 300, 700, rev)
        c.rows.append(VW.make_row(c.dtype, UNPLACED, 1, 5, 3, 9, 2))  # (its other fields are not looked at)
        c.reads.append(b"ACGTACGT")
        c.put(spaced_subs(T, 8), 0, 300, 700, rev)
        c.put(random_reads(c.rng, 1, 400, 400)[0], 0, 300, 700, rev)  # unrelated: OVER at any threshold used here
        c.put(spaced_subs(T, 1), 0, 300, 700, rev)
    for max_edits, want in ((7, [7, 0, UNPLACED, OVER, OVER, 1]), (8, [7, 0, UNPLACED, 8, OVER, 1]), (6, [OVER, 0, UNPLACED, OVER, OVER, 1]),
                            (0, [OVER, 0, UNPLACED, OVER, OVER, OVER])):
        edits, cigars = c.run(placer, O, max_edits=max_edits, max_permille=1000)
        assert edits.tolist() == want * 2
        assert [x == "" for x in cigars] == [e >= OVER for e in want] * 2


def test_row_order_and_counts(env):
    """0 rows; 8 rows of one read out of read order; 1 / 255 / 256 / 257 rows; the three row types' strides"""
    dcn, O, records, _, placer = env
    rng = np.random.default_rng(110)
    F = dcn.filter
    read = VW.mutate_mixed(rng, records[0][100:900], 0.02)
    read = read[:800] if len(read) >= 800 else read + records[0][900:900 + 800 - len(read)]
    reads = [random_reads(rng, 1, 37, 37)[0], read, b"", revcomp(read)]
    b, o = O.concat_reads(reads)
    for dtype in (F.PLACEMENT_DTYPE, F.SPLIT_PLACEMENT_DTYPE, F.PAIR_PLACEMENT_DTYPE):
        e, co, cg = placer.align_batch(b, o, np.zeros(0, dtype), row_offsets=np.zeros(5, np.uint64))
        assert len(e) == 0 and co.tolist() == [0] and len(cg) == 0
        parts = [(q, q + 100) for q in (700, 0, 300, 600, 100, 500, 200, 400)]  # 8 rows, not in read order
        rows = [VW.make_row(dtype, 0, 0, q0, q1, 100 + q0, 100 + q1 - (q0 // 100) % 3) for q0, q1 in parts]
        rows += [VW.make_row(dtype, 0, 1, 800 - q1, 800 - q0, 100 + q0, 100 + q1) for q0, q1 in parts[:3]]
        rows.insert(3, VW.make_row(dtype, UNPLACED, 7, 9, 3, 5, 1))
        rows = np.concatenate(rows)
        ro = np.array([0, 0, 9, 9, 12], np.uint64)
        got = placer.align_batch(b, o, rows, row_offsets=ro, max_permille=1000)
        AW.assert_same(got, AW.align_rows(reads, records, rows, row_offsets=ro, max_permille=1000), rows)
        assert got[0][3] == UNPLACED and got[1][3] == got[1][4]
    for n in (1, 255, 256, 257):
        reads = [records[1][(7 * i) % 1500:(7 * i) % 1500 + 60] for i in range(n)]
        rows = np.concatenate([VW.make_row(F.SPLIT_PLACEMENT_DTYPE, 1 if i % 5 else UNPLACED, 0, 0, 60, (7 * i) % 1500 + i % 2, (7 * i) % 1500 + 60)
                               for i in range(n)])
        b, o = O.concat_reads(reads)
        got = placer.align_batch(b, o, rows)
        AW.assert_same(got, AW.align_rows(reads, records, rows), rows)
        again = placer.align_batch(b, o, rows, row_offsets=np.arange(n + 1, dtype=np.uint64))
        assert all(np.array_equal(x, y) for x, y in zip(got, again))


def test_the_cap_on_three_thousand_bases(env):
    """one row with d near 1,023 on 3,000 bases (a trace of 4 MiB, 16 KB of LDS), and one at about 30 %, both strands"""
    dcn, O, records, _, placer = env
    c = Case(dcn, records, 70)
    T = records[0][500:3500]
    for rev in (0, 1):
        c.put(spaced_subs(T, 1023 - 3 * rev), 0, 500, 3500, rev)  # (d is what the model says: a few below what was planted)
        c.put(VW.mutate_mixed(c.rng, T, 0.3), 0, 500, 3500, rev)
    c.put(VW.mutate_mixed(c.rng, T, 0.6), 0, 500, 3500, 0)
    edits, cigars = c.run(placer, O, max_edits=1023, max_permille=1000)
    assert 1000 <= edits[0] <= 1023 and 1000 <= edits[2] <= 1020 and 500 < edits[1] < 1023 and edits[4] == OVER
    assert cigars[0].count("X") >= 990 and cigars[4] == ""


def groups_default(env):
    dcn, O, _, _, _ = env
    records, reads, rows = AW.groups_batch(dcn)
    amap = VW.build_map(O, dcn, records)
    placer = dcn.Placer(amap, max_batch_bases=1 << 16, max_batch_reads=1 << 10)
    try:
        b, o = O.concat_reads(reads)
        got = placer.align_batch(b, o, rows)
        AW.assert_same(got, AW.align_rows(reads, records, rows), rows)
        assert int(got[0][got[0] < OVER].max()) >= 40
        return "align groups " + "".join(np.ascontiguousarray(x).tobytes().hex() + ":" for x in got)
    finally:
        placer.close()
        amap.close()


@pytest.fixture(scope="module")
def default_line(env):
    return groups_default(env)


LARGEST = 4 * 41 * 41  # the trace of the batch's largest row, d = 40, in bytes


@pytest.mark.parametrize("budget", [64, LARGEST, LARGEST - 1], ids=["64", "largest", "largest-1"])
def test_groups_do_not_change_the_result(default_line, budget):
    """the same batch in a process of its own under DCN_ALIGN_TRACE_BYTES = 64 (16 words: groups of one row, and almost every
    row larger than the budget), = the largest row's trace, and one byte less (that row alone in a group of a buffer it
    outgrows): byte-identical to the default budget's result"""
    env_ = dict(os.environ, DCN_ALIGN_TRACE_BYTES=str(budget))
    p = subprocess.run([sys.executable, WORKER, "groups"], capture_output=True, text=True, timeout=300, env=env_)
    assert p.returncode == 0, p.stderr[-2000:]
    assert default_line in p.stdout.splitlines()

"""The seams of dcn_pileup_batch, dcn_anchor_map_pileup_call and their kernels (pileup.hip), with rows written by hand: no
hashing decides anything here.  The map keeps the bases of two short records, the second starting mid-word of the store;
every case is a call of a few hundred rows (a thousand copies of one read in one case) whose whole pileup, both records
from their first base to their last, is compared with the model of tests/_pileup_worker.py.  Every comparison is exact.

A case is built by put(): the read is flank + S + flank, so that read_start takes any value mod 32, behind a first read of
37 bases with an unplaced row, so that no read of the batch starts on a word of the stream."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _align_worker as AW
import _pileup_worker as PW
import _verify_worker as VW
from conftest import random_reads, revcomp

pytestmark = pytest.mark.gpu

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_pileup_worker.py")
OVER, UNPLACED = VW.OVER, VW.UNPLACED
LEN0, LEN1 = 3989, 1777


def make_records():
    rng = np.random.default_rng(1521)
    a, b = random_reads(rng, 1, LEN0, LEN0)[0], bytearray(random_reads(rng, 1, LEN1, LEN1)[0])
    b[100:103] = b"NNN"
    b[200:260] = bytes(b[200:260]).lower()
    a = a[:1300] + b"A" * 70 + a[1370:]  # a homopolymer: a gap of any length inside it is one run
    return [a, bytes(b)]  # (3989 % 16 != 0: the second record starts mid-word of the store, and of every plane)


@pytest.fixture(scope="module")
def env(dcn, oracle):
    records = make_records()
    amap = VW.build_map(oracle, dcn, records)
    amap.pileup_enable()
    placer = dcn.Placer(amap, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    yield dcn, oracle, records, amap, placer
    placer.close()
    amap.close()


class Case:
    """reads and hand-written rows of one call"""

    def __init__(self, dcn, records, seed):
        self.dcn, self.records, self.rng = dcn, records, np.random.default_rng(seed)
        self.dtype = dcn.filter.PLACEMENT_DTYPE
        self.reads, self.rows = [random_reads(self.rng, 1, 37, 37)[0]], [VW.make_row(self.dtype, UNPLACED, 0, 0, 0, 0, 0)]

    def put(self, S, R, a, b, rev=0, pre=None):
        """a read that holds S (as the row's strand reads it) at offset pre, placed on records[R][a:b]"""
        pre = int(self.rng.integers(0, 40)) if pre is None else pre
        flank = random_reads(self.rng, 2, pre, pre)[0], random_reads(self.rng, 1, 0, 20)[0]
        self.reads.append(flank[0] + (revcomp(S) if rev else S) + flank[1])
        self.rows.append(VW.make_row(self.dtype, R, rev, pre, pre + len(S), a, b))

    def unplaced(self):
        self.reads.append(random_reads(self.rng, 1, 50, 50)[0])
        self.rows.append(VW.make_row(self.dtype, UNPLACED, 0, 0, 0, 0, 0))

    def run(self, amap, placer, oracle, reset=True, **kw):
        """resets, adds, compares both records with the model -> (edits, [CIGAR text per row], counts, n_added), the first
        read's unplaced row left out of the first two"""
        rows = np.concatenate(self.rows)
        b, o = oracle.concat_reads(self.reads)
        if reset:
            amap.pileup_reset()
        edits, n_added = placer.pileup_batch(b, o, rows, **kw)
        counts = PW.new_counts(self.records)
        want_edits, want_added = PW.pile_rows(counts, self.reads, self.records, rows, **kw)
        assert edits.tolist() == want_edits.tolist() and n_added == want_added
        if reset:
            PW.assert_counts(amap, self.records, counts)
        _, offs, cigar = AW.align_rows(self.reads, self.records, rows, **kw)
        return want_edits[1:], [AW.cigar_text(cigar[int(offs[i]):int(offs[i + 1])]) for i in range(1, len(rows))], counts, n_added


def other(base, *avoid):
    """a letter that is none of the given bases"""
    return next(bytes([x]) for x in b"ACGT" if all(bytes([x]) != y.upper() for y in (base,) + avoid))


def spaced(T, positions):
    """T with a substitution at each position"""
    s = bytearray(T)
    for at in positions:
        s[at] = other(bytes(s[at:at + 1]))[0]
    return bytes(s)


def test_one_edit_at_the_seams_of_a_word(env):
    """each op kind at bases 0, 15, 16, 31, 32 and the last of a 64-base interval, on both strands, at read offsets that
    leave the interval at four offsets of a word; on record 1, whose bases lie mid-word, as well"""
    dcn, O, records, amap, placer = env
    c = Case(dcn, records, 40)
    for R, base in ((0, 2000), (1, 1000)):
        for at in (0, 15, 16, 31, 32, 63):
            for rev in (0, 1):
                for pre in (0, 5, 16, 31):
                    a = base + pre
                    T = records[R][a:a + 64]
                    c.put(T[:at] + other(T[at:at + 1]) + T[at + 1:], R, a, a + 64, rev, pre=pre)
                    c.put(T[:at] + T[at + 1:], R, a, a + 64, rev, pre=pre)
                    c.put(T[:at] + other(T[at:at + 1], T[at - 1:at] if at else T[at:at + 1]) + T[at:], R, a, a + 64, rev, pre=pre)
    edits, cigars, counts, n_added = c.run(amap, placer, O)
    assert (edits == 1).all() and n_added == len(edits)
    assert all("X" in x for x in cigars[0::3]) and all("D" in x for x in cigars[1::3]) and all("I" in x for x in cigars[2::3])
    assert any(x[:2] == op for x in cigars for op in ("1I", "1X")) and any(x.endswith("1X") for x in cigars)  # an edit as the first run, and the last
    for R in (0, 1):
        assert counts[R][:, PW.REV].sum() > 0 and counts[R][:, PW.INS].sum() == len(edits) // 6 and counts[R][:, PW.DEL].sum() == len(edits) // 6


def test_record_ends_do_not_cross(env):
    """a row that ends on the last base of record 0 and one that starts on base 0 of record 1, with every op kind near the
    seam: nothing of one record's rows reaches the other's counters (record 1 follows record 0 in every plane)"""
    dcn, O, records, amap, placer = env
    c = Case(dcn, records, 41)
    for rev in (0, 1):
        T = records[0][LEN0 - 80:]
        c.put(T, 0, LEN0 - 80, LEN0, rev)
        c.put(T[:-1] + other(T[-1:]), 0, LEN0 - 80, LEN0, rev)               # X on the last base
        c.put(T[:-1], 0, LEN0 - 80, LEN0, rev)                                # a base of T alone near the end
        c.put(T + other(T[-1:]), 0, LEN0 - 80, LEN0, rev)                     # I as the last run: INS on the last base
        T = records[1][:80]
        c.put(T, 1, 0, 80, rev)
        c.put(other(T[:1]) + T[1:], 1, 0, 80, rev)                            # X on base 0
        c.put(T[1:], 1, 0, 80, rev)
        c.put(other(T[:1]) + T, 1, 0, 80, rev)                                # I as the first run: INS on base 0
    edits, cigars, counts, _ = c.run(amap, placer, O)
    assert (edits <= 1).all()
    assert cigars[3] == "80=1I" and cigars[7] == "1I80=" and counts[0][LEN0 - 1, PW.INS] == 2 and counts[1][0, PW.INS] == 2
    assert counts[0][LEN0 - 1, :6].sum() == 8 and counts[1][0, :6].sum() == 8 and not counts[0][:LEN0 - 80].any() and not counts[1][80:].any()


def test_rows_that_add_nothing(env):
    """an n = 0 row and an m = 0 row (aligned under max_permille = 1000: all I, all D), an UNPLACED and an OVER row between
    adding ones, N in the read and in the record, lower case"""
    dcn, O, records, amap, placer = env
    c = Case(dcn, records, 42)
    T = records[1][60:300]  # NNN at 100, lower case from 200
    c.put(T, 1, 60, 300)
    c.put(records[0][500:520], 0, 700, 700)        # n = 0: 20I, adds nothing
    c.put(b"", 0, 800, 820, pre=7)                 # m = 0: 20D
    c.unplaced()
    c.put(random_reads(c.rng, 1, 100, 100)[0], 0, 900, 1000)  # unrelated, but within 1000 permille: it aligns
    c.put(b"", 0, 1200, 1200, pre=3)               # m = n = 0: no run
    s = bytearray(T)
    s[50:52] = b"NN"
    c.put(bytes(s).swapcase(), 1, 60, 300, rev=1)
    edits, cigars, counts, n_added = c.run(amap, placer, O, max_permille=1000)
    assert cigars[1] == "20I" and cigars[2] == "20D" and cigars[5] == "" and edits[5] == 0 and edits[3] == UNPLACED
    assert n_added == 4 and not counts[0][700 - 5:700 + 5].any() and (counts[0][800:820, PW.DEL] == 1).all()
    assert counts[1][100:103, PW.N].tolist() == [2, 2, 2] and counts[1][110:112, PW.N].tolist() == [1, 1]  # N counts as N under X
    # the default threshold: the unrelated read is OVER, and so are the all-I and the all-D row
    edits, _, counts, n_added = c.run(amap, placer, O)
    assert edits[1] == edits[2] == edits[4] == OVER and n_added == 2 and not counts[0].any()


def test_many_runs_and_long_runs(env):
    """rows with 63, 64, 65 and 129 runs (the chunks of 64 runs and what they carry over), and runs of 63, 64 and 65 bases of
    every op kind (the lanes' stride)"""
    dcn, O, records, amap, placer = env
    c = Case(dcn, records, 43)
    T = records[0][1000:1700]
    for rev in (0, 1):
        c.put(spaced(T, [10 + 10 * q for q in range(31)]), 0, 1000, 1700, rev)          # 31 X: 63 runs
        c.put(spaced(T, [0] + [10 + 10 * q for q in range(31)]), 0, 1000, 1700, rev)    # X first: 64 runs
        c.put(spaced(T, [10 + 10 * q for q in range(32)]), 0, 1000, 1700, rev)          # 65 runs
        c.put(spaced(T, [5 + 10 * q for q in range(64)]), 0, 1000, 1700, rev)           # 129 runs
        c.put(spaced(T, [63, 63 + 65, 63 + 65 + 66]), 0, 1000, 1700, rev)               # '=' runs of 63, 64, 65
        assert T[300:370] == b"A" * 70
        for ln in (63, 64, 65):  # inside the homopolymer
            c.put(T[:300] + b"A" * (70 - ln) + T[370:], 0, 1000, 1700, rev)                            # a D run of ln
            c.put(T[:300] + b"A" * (70 + ln) + T[370:], 0, 1000, 1700, rev)                            # an I run of ln
            c.put(T[:300] + b"AA" + b"C" * ln + b"A" * (68 - ln) + T[370:], 0, 1000, 1700, rev)        # an X run of ln
    edits, cigars, counts, n_added = c.run(amap, placer, O)
    assert n_added == len(edits)
    n_runs = [len(AW.parse_cigar(x)) for x in cigars]
    assert {63, 64, 65, 129} <= set(n_runs), sorted(set(n_runs))
    lengths = {(int(x) >> 4, AW.LETTER[int(x) & 15]) for t in cigars for x in AW.parse_cigar(t)}
    assert {(ln, op) for ln in (63, 64, 65) for op in "=XID"} <= lengths, sorted(lengths)


@pytest.mark.parametrize("n_rows", [0, 1, 255, 256, 257])
def test_row_counts(env, n_rows):
    """0 rows, one, and the counts around a grid of 256-thread workgroups"""
    dcn, O, records, amap, placer = env
    c = Case(dcn, records, 44)
    if n_rows == 0:
        c.reads, c.rows = [], []
        amap.pileup_reset()
        b, o = O.concat_reads([])
        edits, n_added = placer.pileup_batch(b, o, np.zeros(0, c.dtype))
        assert len(edits) == 0 and n_added == 0 and not amap.pileup_fetch(0).any() and not amap.pileup_fetch(1).any()
        return
    c.reads, c.rows = [], []
    for q in range(n_rows):
        a = (37 * q) % (LEN1 - 60)
        T = records[1][a:a + 60]
        c.put(T[:20] + other(T[20:21]) + T[21:] if q % 3 == 0 else T, 1, a, a + 60, rev=q % 2)
    c.reads.insert(0, b"ACG")  # (a first read that no row belongs to shifts every read off the words of the stream)
    c.rows.insert(0, VW.make_row(c.dtype, UNPLACED, 0, 0, 0, 0, 0))
    _, _, counts, n_added = c.run(amap, placer, O)
    assert n_added == n_rows and counts[1][:, :6].sum() == 60 * n_rows


@pytest.mark.parametrize("depth", [1, 64, 65, 1000])
def test_depth_of_one_identical_read(env, depth):
    """the same read `depth` times: every wave of the grid adds to the same 150 words of each plane"""
    dcn, O, records, amap, placer = env
    c = Case(dcn, records, 45)
    T = records[0][3000:3150]
    S = T[:40] + other(T[40:41]) + T[41:90] + T[92:120] + b"GG" + T[120:]
    for q in range(depth):
        c.put(S, 0, 3000, 3150, rev=0, pre=q % 33)
    edits, cigars, counts, n_added = c.run(amap, placer, O)
    assert n_added == depth and (counts[0][3000:3150, :6].sum(axis=1) == depth).all() and counts[0][:, PW.INS].sum() == depth
    assert counts[0][:, PW.DEL].sum() == 2 * depth and not counts[0][:3000].any() and not counts[0][3150:].any()


def groups_default(env):
    dcn, O, _, _, _ = env
    records, reads, rows = AW.groups_batch(dcn)
    amap = VW.build_map(O, dcn, records)
    amap.pileup_enable()
    placer = dcn.Placer(amap, max_batch_bases=1 << 16, max_batch_reads=1 << 10)
    try:
        b, o = O.concat_reads(reads)
        _, n_added = placer.pileup_batch(b, o, rows)
        return "pileup groups %d " % n_added + "".join(np.ascontiguousarray(amap.pileup_fetch(R)).tobytes().hex() + ":" for R in range(len(records)))
    finally:
        placer.close()
        amap.close()


def test_trace_groups_do_not_change_the_result(env):
    """the same batch in a process of its own under DCN_ALIGN_TRACE_BYTES = 64 (groups of one row, almost every row larger
    than the budget): the pileup is byte-identical to the default budget's, and the worker compares it with the model"""
    line = groups_default(env)
    p = subprocess.run([sys.executable, WORKER, "groups"], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, DCN_ALIGN_TRACE_BYTES="64"))
    assert p.returncode == 0, p.stderr[-2000:]
    assert line in p.stdout.splitlines() and int(line.split()[2]) >= 10


# ---- calls ------------------------------------------------------------------------------------------------------------
SETTINGS = [(3, 500), (4, 500), (5, 500), (4, 750), (4, 751), (1, 0), (1, 1000), (0, 250), (2, 501)]


def call_case(env):
    """record 1 under four reads over its first 600 bases: three carry the same substitution at bases 0, 255, 256, 257 and
    599 (3 of 4: called at 750 permille, not at 751), two of them one at base 50 (a tie, 2 : 2), three lack base 300.  Four
    more rows start at base 700 with the four letters there, two of them behind an inserted run: I as the first run adds
    at ref_start, so base 700 has INS = 2 over a best count of 1 (INS flagged on a position without a call).  Bases
    100-102 of the record are N."""
    dcn, O, records, amap, placer = env
    T = records[1][:600]
    alt = {p: other(T[p:p + 1]) for p in (0, 50, 255, 256, 257, 599)}

    def read(subs, delete):
        s = [T[p:p + 1] for p in range(600)]
        for p in subs:
            s[p] = alt[p]
        if delete:
            s[300] = b""
        s[100:103] = [b"G", b"g", b"G"]  # where the record has N the reads have a base
        return b"".join(s)

    c = Case(dcn, records, 46)
    c.put(read((0, 50, 255, 256, 257, 599), True), 1, 0, 600)
    c.put(read((0, 50, 255, 256, 257, 599), True), 1, 0, 600, rev=1)
    c.put(read((0, 255, 256, 257, 599), True), 1, 0, 600)
    c.put(read((), False), 1, 0, 600, rev=1)
    U = records[1][700:760]
    behind = [x for x in b"ACGT" if bytes([x]) != U[1:2].upper()][:2]  # (a letter that the next base repeats would move the run)
    for q, letter in enumerate(b"ACGT"):
        run = other(U[:1], bytes([letter]), U[1:2]) * 3 if letter in behind else b""
        c.put(run + bytes([letter]) + U[1:], 1, 700, 760, rev=q // 2)
    return c


def test_calls_and_sites(env):
    dcn, O, records, amap, placer = env
    c = call_case(env)
    edits, cigars, counts, n_added = c.run(amap, placer, O)
    k = counts[1]
    assert n_added == 8 and (k[:600, :6].sum(axis=1) == 4).all() and (k[700:760, :6].sum(axis=1) == 4).all()
    assert sorted(k[50, :4].tolist()) == [0, 0, 2, 2] and (k[295:305, PW.DEL] == 3).sum() == 1
    assert k[700, :4].tolist() == [1, 1, 1, 1] and k[700, PW.INS] == 2 and [x[:2] for x in cigars[4:]].count("3I") == 2
    for p in (0, 255, 256, 257, 599):
        assert sorted(k[p, :4].tolist()) == [0, 0, 1, 3]
    gone = 295 + int(np.argmax(k[295:305, PW.DEL]))
    for min_depth, min_permille in SETTINGS:
        kw = dict(min_depth=min_depth, min_permille=min_permille)
        calls, pos, info = PW.assert_calls(amap, records, counts, 1, **kw)             # the whole record
        for start, n in ((0, 600), (0, 1), (255, 1), (255, 2), (256, 2), (257, 343), (1, 255), (1, 256), (300, 101), (599, 1), (600, 1177), (37, 0)):
            PW.assert_calls(amap, records, counts, 1, start, n, **kw)                   # ranges that start mid-record
        at = {int(p): int(x) for p, x in zip(pos, info)}
        if (min_depth, min_permille) == (4, 750):  # best * 1000 = depth * permille: called
            assert all(at[p] & 0xFF == PW.SITE_SUB for p in (0, 255, 256, 257, 599)) and at[gone] & 0xFFFF == PW.SITE_DEL | 4 << 8
            assert 50 not in at and calls[gone:gone + 1] == b"-" and calls[50:51] == b"N" and calls[800:801] == b"N"
        if (min_depth, min_permille) in ((4, 751), (5, 500)):  # one permille more, or depth = min_depth - 1: not called
            assert not any(p in at for p in (0, 255, 256, 257, 599, gone)) and calls[:1] == b"N"
        if (min_depth, min_permille) == (4, 500):
            assert at[700] & 0xFFFF == PW.SITE_INS | PW.NO_CODE << 8 and calls[700:701] == b"N"  # INS on a position without a call
            first = min(col for col in range(4) if k[50, col] == 2)
            assert calls[50:51] == b"ACGT"[first:first + 1]                                       # the tie calls the first
        if (min_depth, min_permille) == (1, 0):
            text = np.frombuffer(calls, np.uint8)
            assert (text[:600] != ord("N")).all() and (text[600:700] == ord("N")).all() and (text[760:] == ord("N")).all()
    # a reference N differs from every call: bases 100-102 are sites wherever they are called
    _, pos, info = PW.call_range(counts[1], records[1], 0, 600, 3, 500)
    assert [int(x) for p, x in zip(pos, info) if 100 <= p <= 102] == [PW.SITE_SUB | PW.G << 8 | PW.NO_CODE << 16] * 3


def test_call_capacity_protocol(env):
    """capacity 0 with NULL, one short, exact, more: n_sites and calls complete, no site written until they fit"""
    dcn, O, records, amap, placer = env
    c = call_case(env)
    _, _, counts, _ = c.run(amap, placer, O)
    N = dcn._native
    L = N.lib()
    want_calls, want_pos, want_info = PW.call_range(counts[1], records[1], 0, LEN1, 3, 500)
    total = len(want_pos)
    assert total >= 10
    prm = N.PileupCallParams(3, 500, (C.c_uint32 * 2)(0, 0))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def raw(capacity, nulls=False, want_calls_too=True):
        calls = np.full(LEN1, 0xAB, np.uint8)
        pos, info = np.full(max(capacity, 1), 0xABABABABABABABAB, np.uint64), np.full(max(capacity, 1), 0xABABABAB, np.uint32)
        n = C.c_uint64(12345)
        rc = L.dcn_anchor_map_pileup_call(amap._h, C.byref(prm), 1, 0, LEN1, ptr(calls) if want_calls_too else None, None if nulls else ptr(pos),
                                          None if nulls else ptr(info), capacity, C.byref(n))
        return rc, calls.tobytes(), pos, info, n.value

    rc, calls, _, _, n = raw(0, nulls=True)
    assert rc == N.DCN_ERR_CAPACITY and n == total and calls == want_calls and str(total).encode() in L.dcn_last_error()
    rc, _, _, _, n = raw(0, nulls=True, want_calls_too=False)
    assert rc == N.DCN_ERR_CAPACITY and n == total
    rc, calls, pos, info, n = raw(total - 1)
    assert rc == N.DCN_ERR_CAPACITY and n == total and calls == want_calls and (pos == 0xABABABABABABABAB).all() and (info == 0xABABABAB).all()
    rc, calls, pos, info, n = raw(total)
    assert rc == 0 and n == total and calls == want_calls and pos.tolist() == want_pos.tolist() and info.tolist() == want_info.tolist()
    rc, _, pos, info, n = raw(total + 3)
    assert rc == 0 and n == total and pos[:total].tolist() == want_pos.tolist() and (pos[total:] == 0xABABABABABABABAB).all()
    assert info[:total].tolist() == want_info.tolist() and (info[total:] == 0xABABABAB).all()
    rc, *_ = raw(total, nulls=True)
    assert rc == N.DCN_ERR_ARG and b"site_pos/site_info is NULL" in L.dcn_last_error()
    # a range without a site: capacity 0 with NULLs succeeds
    n = C.c_uint64(9)
    assert L.dcn_anchor_map_pileup_call(amap._h, C.byref(prm), 0, 0, LEN0, None, None, None, 0, C.byref(n)) == 0 and n.value == 0
    for bad, word in ((N.PileupCallParams(3, 1001, (C.c_uint32 * 2)(0, 0)), b"min_permille must be 0..1000"),
                      (N.PileupCallParams(3, 500, (C.c_uint32 * 2)(0, 1)), b"reserved")):
        assert L.dcn_anchor_map_pileup_call(amap._h, C.byref(bad), 1, 0, 10, None, None, None, 0, C.byref(n)) == N.DCN_ERR_ARG
        assert word in L.dcn_last_error()
    assert L.dcn_anchor_map_pileup_call(amap._h, C.byref(prm), 1, 0, 10, None, None, None, 0, None) == N.DCN_ERR_ARG
    assert L.dcn_anchor_map_pileup_call(amap._h, C.byref(prm), 1, LEN1, 1, None, None, None, 0, C.byref(n)) == N.DCN_ERR_ARG
    assert b"past the record's 1777 bases" in L.dcn_last_error()

"""The seams of the insertion ledger's kernels (insertions.hip) and of dcn_anchor_map_insertions_fetch / _call, with rows
written by hand as tests/test_gpu_pileup_seams.py writes them: two short records, the second starting mid-word of the
store; every case is a call of a few hundred rows (a thousand copies of one read in one case) whose whole ledger, both
records from their first base to their last, is compared with the model of tests/_insertion_worker.py, with the counters
beside it.  Every comparison is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _align_worker as AW
import _insertion_worker as IW
import _pileup_worker as PW
import _verify_worker as VW
from conftest import random_reads
from test_gpu_pileup_seams import LEN0, LEN1, Case, make_records, other

pytestmark = pytest.mark.gpu

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_insertion_worker.py")
UNPLACED, OVER = VW.UNPLACED, VW.OVER


@pytest.fixture(scope="module")
def env(dcn, oracle):
    records = make_records()
    amap = VW.build_map(oracle, dcn, records)
    amap.pileup_enable()
    amap.pileup_keep_insertions()
    placer = dcn.Placer(amap, max_batch_bases=1 << 21, max_batch_reads=1 << 12)
    yield dcn, oracle, records, amap, placer
    placer.close()
    amap.close()


def run(c, amap, placer, oracle, row_offsets=None, settings=((3, 500), (1, 0)), **kw):
    """resets, adds the case's rows, compares counters and ledger of both records with the model -> (counts, ledger, edits,
    [CIGAR text per row])"""
    rows = np.concatenate(c.rows)
    b, o = oracle.concat_reads(c.reads)
    amap.pileup_reset()
    edits, n_added = placer.pileup_batch(b, o, rows, row_offsets=row_offsets, **kw)
    counts, ledger = PW.new_counts(c.records), IW.new_ledger(c.records)
    want_edits, want_added = IW.pile_rows(counts, ledger, c.reads, c.records, rows, row_offsets=row_offsets, **kw)
    assert edits.tolist() == want_edits.tolist() and n_added == want_added
    PW.assert_counts(amap, c.records, counts)
    IW.assert_ledger(amap, c.records, counts, ledger, settings=settings)
    _, offs, cigar = AW.align_rows(c.reads, c.records, rows, row_offsets, **kw)
    return counts, ledger, want_edits, [AW.cigar_text(cigar[int(offs[i]):int(offs[i + 1])]) for i in range(len(rows))]


def behind(T, at, ins):
    """T with `ins` behind its base `at`"""
    return T[:at + 1] + ins + T[at + 1:]


def foreign(T, at, n=1):
    """n bases that are neither T[at] nor T[at + 1]: a run of them behind base `at` cannot move"""
    return other(T[at:at + 1], T[at + 1:at + 2] or T[at:at + 1]) * n


def test_one_run_at_the_seams_of_a_word(env):
    """an I run behind bases 0, 15, 16, 31, 32 and the last of a 64-base interval, and in front of base 0, on both strands,
    at read offsets that leave the interval at four offsets of a word; on record 1, whose bases lie mid-word, as well"""
    dcn, O, records, amap, placer = env
    c = Case(dcn, records, 60)
    for R, base in ((0, 2000), (1, 1000)):
        for at in (0, 15, 16, 31, 32, 63):
            for rev in (0, 1):
                for pre in (0, 5, 16, 31):
                    a = base + pre
                    T = records[R][a:a + 64]
                    c.put(behind(T, at, foreign(T, at, 1 + at % 3)), R, a, a + 64, rev, pre=pre)
        for rev in (0, 1):
            T = records[R][base:base + 64]
            c.put(other(T[:1]) * 2 + T, R, base, base + 64, rev)  # in front of base 0 of the interval
    counts, ledger, edits, cigars = run(c, amap, placer, O)
    assert (edits[1:] <= 3).all() and all(x.count("I") == 1 for x in cigars[1:])
    assert sum(x.endswith("I") for x in cigars) == 16 and sum(x[1:2] == "I" or x[2:3] == "I" for x in cigars) >= 4
    for R in (0, 1):
        assert {e[1] for e in ledger[R]} == {0, 1} and {e[4] for e in ledger[R]} == {0, 1} and {e[2] for e in ledger[R]} == {1, 2, 3}


def test_record_ends_do_not_cross(env):
    """front at base 0 of each record; an insertion behind the last base of record 0 belongs to record 0 and does not appear in
    record 1's range, whose first base follows it in the store"""
    dcn, O, records, amap, placer = env
    c = Case(dcn, records, 61)
    for rev in (0, 1):
        for q in range(3):
            T = records[0][LEN0 - 80:]
            c.put(T + other(T[-1:]) * 2, 0, LEN0 - 80, LEN0, rev)   # I as the last run: behind the last base of record 0
            T = records[0][:80]
            c.put(other(T[:1]) * 3 + T, 0, 0, 80, rev)             # I as the first run: in front of base 0
            T = records[1][:80]
            c.put(other(T[:1]) + T, 1, 0, 80, rev)
            T = records[1][LEN1 - 80:]
            c.put(T + other(T[-1:]), 1, LEN1 - 80, LEN1, rev)
    counts, ledger, edits, cigars = run(c, amap, placer, O)
    assert sorted({(e[0], e[1], e[2]) for e in ledger[0]}) == [(0, 1, 3), (LEN0 - 1, 0, 2)]
    assert sorted({(e[0], e[1], e[2]) for e in ledger[1]}) == [(0, 1, 1), (LEN1 - 1, 0, 1)]
    # called insertions at position 0 and at the last, in front and behind
    al, bases = amap.insertions_call(0)
    assert [(int(a["pos"]), int(a["flags"]), int(a["count"]), int(a["events"])) for a in al] == [(0, 1, 6, 6), (LEN0 - 1, 0, 6, 6)]
    got = amap.consensus(0, fill_ref=True)
    assert got == bases[:3] + VW.fetched_text(records[0]) + bases[3:] and len(got) == LEN0 + 5
    ev, _ = amap.insertions_fetch(1, 0, 1)
    assert len(ev) == 6 and (ev["pos"] == 0).all() and (ev["flags"] & 1).all()
    ev, _ = amap.insertions_fetch(0, LEN0 - 1, 1)
    assert len(ev) == 6 and (ev["pos"] == LEN0 - 1).all() and not (ev["flags"] & 1).any()


def runs_row(T0, n_runs, i_index):
    """(S, T) whose alignment has n_runs runs, '=' of three bases at the even indices and X of one at the odd ones, but an I
    run of two bases at i_index (odd)"""
    S, T, at = bytearray(), bytearray(), 0
    for r in range(n_runs):
        if r % 2 == 0:
            S += T0[at:at + 3]
            T += T0[at:at + 3]
            at += 3
        elif r == i_index:
            S += other(T0[at - 1:at], T0[at:at + 1]) * 2
        else:
            S += other(T0[at:at + 1])
            T += T0[at:at + 1]
            at += 1
    return bytes(S), at


def test_many_runs_and_long_runs(env):
    """rows of 63, 64, 65 and 129 runs with an I run at index 63 and at index 64 (the chunks of 64 runs and what they carry
    over: offsets of events and of bases), and I runs of 1, 63, 64, 65 and 1,023 bases (the lanes' stride)"""
    dcn, O, records, amap, placer = env
    c = Case(dcn, records, 62)
    shapes = [(63, 61), (64, 63), (65, 63), (129, 63), (129, 65), (129, 127), (67, 1)]
    for rev in (0, 1):
        for n_runs, i_index in shapes:
            S, n = runs_row(records[0][1000:1400], n_runs, i_index)
            c.put(S, 0, 1000, 1000 + n, rev)
        # an I run as run 64 (index 64 is even here: X first)
        T = records[0][1500:1800]
        S = bytearray(other(T[:1]) + T[1:])
        for q in range(31):
            S[4 + 4 * q] = other(T[4 + 4 * q:5 + 4 * q])[0]
        S = bytes(S[:140]) + foreign(T, 139, 2) + bytes(S[140:])
        c.put(S, 0, 1500, 1800, rev)
        T = records[1][400:464]
        for ln in (1, 63, 64, 65, 1023):
            c.put(behind(T, 20, b"N" * ln), 1, 400, 464, rev)               # invalid bases equal nothing: one run
        for ln in (63, 64, 65):
            c.put(behind(T, 40, foreign(T, 40, ln)), 1, 400, 464, rev)      # letters that neither neighbour has
    counts, ledger, edits, cigars = run(c, amap, placer, O, max_permille=1000, settings=((3, 500),))
    assert (edits[1:] < OVER).all()
    parsed = [AW.parse_cigar(x) for x in cigars[1:]]
    for k, (n_runs, i_index) in enumerate(shapes):
        assert len(parsed[k]) == n_runs and int(parsed[k][i_index]) & 15 == AW.OP_I, (n_runs, i_index, cigars[1 + k])
    assert len(parsed[len(shapes)]) >= 66 and int(parsed[len(shapes)][64]) & 15 == AW.OP_I, cigars[1 + len(shapes)]
    assert {1, 63, 64, 65, 1023} <= {e[2] for e in ledger[1] if e[3] == b"N" * e[2]}
    assert {63, 64, 65} <= {e[2] for e in ledger[1] if b"N" not in e[3]}


def test_rows_that_add_nothing(env):
    """UNPLACED, OVER, n = 0 (all I: no event, by P2) and I-free rows between adding ones"""
    dcn, O, records, amap, placer = env
    c = Case(dcn, records, 63)
    T = records[1][60:300]
    c.put(behind(T, 30, foreign(T, 30, 2)), 1, 60, 300)
    c.put(records[0][500:520], 0, 700, 700)           # n = 0: 20I, adds nothing
    c.unplaced()
    c.put(T, 1, 60, 300, rev=1)                        # no I run
    c.put(random_reads(c.rng, 1, 100, 100)[0], 0, 900, 1000)  # OVER under the default threshold
    c.put(b"", 0, 800, 820, pre=7)                    # m = 0: OVER under the default threshold
    c.put(behind(T, 100, foreign(T, 100, 3)), 1, 60, 300, rev=1)
    # under 1000 permille the all-I row aligns and still adds nothing (P2); the unrelated read aligns, with whatever runs
    counts, ledger, edits, cigars = run(c, amap, placer, O, max_permille=1000, settings=((1, 0),))
    assert edits[2] == 20 and cigars[2] == "20I" and edits[3] == UNPLACED and cigars[6] == "20D" and not any(690 <= e[0] < 830 for e in ledger[0])
    counts, ledger, edits, cigars = run(c, amap, placer, O)
    assert edits[2] == OVER and edits[3] == UNPLACED and edits[5] == OVER and edits[6] == OVER
    assert ledger[0] == [] and sorted((e[0], e[2], e[4]) for e in ledger[1]) == [(90, 2, 0), (160, 3, 1)]
    assert amap.insertions_info() == (2, 5)
    # a batch without an I run leaves the ledger as it is
    c = Case(dcn, records, 64)
    c.put(T, 1, 60, 300)
    counts, ledger, _, _ = run(c, amap, placer, O)
    assert amap.insertions_info() == (0, 0) and counts[1][:, :6].sum() == 240


@pytest.mark.parametrize("n_rows", [0, 1, 255, 256, 257])
def test_row_counts(env, n_rows):
    """0 rows, one, and the counts around a grid of 256-thread workgroups (of rows, of events, of positions)"""
    dcn, O, records, amap, placer = env
    c = Case(dcn, records, 65)
    if n_rows == 0:
        amap.pileup_reset()
        b, o = O.concat_reads([])
        edits, n_added = placer.pileup_batch(b, o, np.zeros(0, c.dtype))
        assert len(edits) == 0 and n_added == 0 and amap.insertions_info() == (0, 0)
        assert len(amap.insertions_fetch(0)[0]) == 0 and len(amap.insertions_call(1)[0]) == 0
        return
    c.reads, c.rows = [], []
    for q in range(n_rows):
        a = (37 * q) % (LEN1 - 60)
        T = records[1][a:a + 60]
        c.put(behind(T, 20 + q % 7, foreign(T, 20 + q % 7, 1 + q % 2)) if q % 3 else T, 1, a, a + 60, rev=q % 2)
    c.reads.insert(0, b"ACG")
    c.rows.insert(0, VW.make_row(c.dtype, UNPLACED, 0, 0, 0, 0, 0))
    counts, ledger, _, _ = run(c, amap, placer, O)
    assert len(ledger[1]) == n_rows - (n_rows + 2) // 3


@pytest.mark.parametrize("depth", [1, 2, 63, 64, 65, 1000])
def test_events_at_one_position(env, depth):
    """one read `depth` times through row_offsets: every event in one bucket, one allele"""
    dcn, O, records, amap, placer = env
    c = Case(dcn, records, 66)
    T = records[0][3000:3150]
    S = behind(T, 70, foreign(T, 70, 3))
    c.reads, c.rows = [S], [VW.make_row(c.dtype, 0, 0, 0, len(S), 3000, 3150)] * depth
    counts, ledger, _, _ = run(c, amap, placer, O, row_offsets=np.array([0, depth], np.uint64), settings=((1, 500),))
    al, bases = amap.insertions_call(0, min_depth=1)
    assert IW.alleles_as_tuples(al, bases) == [(3070, 0, 3, S[71:74], depth, depth)]


@pytest.mark.parametrize("first,second", [(500, 500), (501, 499), (499, 501)])
def test_two_alleles_at_one_position(env, first, second):
    """a thousand events of two alleles at one position: 500 : 500 goes to the one that comes first in the canonical order,
    one event more decides otherwise (the quadratic pass over a bucket of a thousand)"""
    dcn, O, records, amap, placer = env
    c = Case(dcn, records, 67)
    T = records[0][3000:3150]
    S1, S2 = behind(T, 70, b"NT" + foreign(T, 70, 1)), behind(T, 70, b"NN" + foreign(T, 70, 1))  # (N before T: S2's comes first)
    c.reads = [S1, S2]
    c.rows = [VW.make_row(c.dtype, 0, 0, 0, len(S1), 3000, 3150)] * first + [VW.make_row(c.dtype, 0, 0, 0, len(S2), 3000, 3150)] * second
    counts, ledger, _, _ = run(c, amap, placer, O, row_offsets=np.array([0, first, 1000], np.uint64), settings=((3, 500),))
    (al,), bases = amap.insertions_call(0)
    want = S1[71:74] if first > second else S2[71:74]
    assert (int(al["pos"]), int(al["count"]), int(al["events"]), bases) == (3070, max(first, second), 1000, want)
    assert int(counts[0][3070, PW.INS]) == 1000


def call_case(env):
    """record 1 under three reads over its first 600 bases, each with the same insertion behind bases 0, 255, 256, 257 and 599
    (called), one of them with another behind base 300 (1 of 3: not called at 500 permille) and two with two different ones
    behind base 400 (2 events of 3 reads: called, a 1 : 1 tie)"""
    dcn, O, records, amap, placer = env
    T = records[1][:600]

    def read(extra):
        s = [T[p:p + 1] for p in range(600)]
        for p in (0, 255, 256, 257, 599):
            s[p] += foreign(T, p, 2) if p < 599 else other(T[599:600]) * 2
        for p, ins in extra:
            s[p] += ins
        return b"".join(s)

    c = Case(dcn, records, 68)
    x = foreign(T, 400)
    c.put(read([(300, foreign(T, 300, 4)), (400, x + b"T" + x)]), 1, 0, 600)
    c.put(read([(400, x + b"N" + x)]), 1, 0, 600, rev=1)
    c.put(read([]), 1, 0, 600)
    return c


def test_ranges_and_called_positions(env):
    """called insertions at positions 0, 255, 256, 257 and the last of a range; ranges that start and end mid-record and
    between two events; n_bases = 0"""
    dcn, O, records, amap, placer = env
    c = call_case(env)
    counts, ledger, _, _ = run(c, amap, placer, O, settings=((3, 500), (3, 333), (1, 0), (4, 0)))
    want = IW.call_range(counts[1], ledger[1], records[1])
    assert [a[0] for a in want] == [0, 255, 256, 257, 400, 599] and want[4][2:5] == (3, want[4][3], 1) and b"N" in want[4][3]
    assert [a[0] for a in IW.call_range(counts[1], ledger[1], records[1], min_permille=333)] == [0, 255, 256, 257, 300, 400, 599]  # (1 of 3: 1000 >= 999)
    for start, n in ((0, 600), (0, 1), (1, 254), (255, 1), (255, 2), (256, 2), (256, 1), (257, 343), (1, 255), (1, 256), (258, 42), (300, 101),
                     (301, 99), (599, 1), (600, 1177), (37, 0), (0, 0), (LEN1, 0)):
        ev, bases = amap.insertions_fetch(1, start, n)
        IW.assert_dense(ev, bases)
        assert IW.events_as_tuples(ev, bases) == IW.fetch_range(ledger[1], start, n), (start, n)
        for min_depth, min_permille in ((3, 500), (1, 0)):
            al, bases = amap.insertions_call(1, start, n, min_depth, min_permille)
            IW.assert_dense(al, bases)
            assert IW.alleles_as_tuples(al, bases) == IW.call_range(counts[1], ledger[1], records[1], start, n, min_depth, min_permille), (start, n)
            for fill in (False, True):
                assert amap.consensus(1, start, n, min_depth, min_permille, fill) == IW.consensus(counts[1], ledger[1], records[1], start, n, min_depth,
                                                                                                  min_permille, fill), (start, n, fill)
    N = dcn._native
    L = N.lib()
    n, m = C.c_uint64(5), C.c_uint64(5)
    assert L.dcn_anchor_map_insertions_fetch(amap._h, 1, 7, 0, None, 0, None, 0, C.byref(n), C.byref(m)) == 0 and (n.value, m.value) == (0, 0)
    for args, word in (((2, 0, 1), b"record 2 of 2 added"), ((1, LEN1, 1), b"past the record's"), ((1, 0, LEN1 + 1), b"past the record's")):
        assert L.dcn_anchor_map_insertions_fetch(amap._h, *args, None, 0, None, 0, C.byref(n), C.byref(m)) == N.DCN_ERR_ARG
        assert word in L.dcn_last_error() and b"insertions fetch" in L.dcn_last_error()
        prm = N.PileupCallParams(3, 500, (C.c_uint32 * 2)(0, 0))
        assert L.dcn_anchor_map_insertions_call(amap._h, C.byref(prm), *args, None, 0, None, 0, C.byref(n), C.byref(m)) == N.DCN_ERR_ARG
        assert word in L.dcn_last_error() and b"insertions call" in L.dcn_last_error()


def test_capacity_protocol(env):
    """NULLs with capacity 0, either capacity one too small, exact, more: the two counts are always complete, and nothing
    else is written until both arrays fit"""
    dcn, O, records, amap, placer = env
    c = call_case(env)
    counts, ledger, _, _ = run(c, amap, placer, O)
    N = dcn._native
    L = N.lib()
    prm = N.PileupCallParams(3, 500, (C.c_uint32 * 2)(0, 0))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    want_ev = IW.fetch_range(ledger[1], 0, LEN1)
    want_al = IW.call_range(counts[1], ledger[1], records[1])
    for fetch, dtype, want, as_tuples in ((True, dcn.INSERTION_DTYPE, want_ev, IW.events_as_tuples), (False, dcn.INSERTION_ALLELE_DTYPE, want_al, IW.alleles_as_tuples)):
        total, total_bases = len(want), sum(x[2] for x in want)
        assert total >= 6 and total_bases > total

        def raw(cap, base_cap, nulls=False):
            items, bases = np.full(max(cap, 1) * dtype.itemsize, 0xAB, np.uint8), np.full(max(base_cap, 1), 0xAB, np.uint8)
            n, m = C.c_uint64(12345), C.c_uint64(12345)
            tail = (None if nulls else ptr(items), cap, None if nulls else ptr(bases), base_cap, C.byref(n), C.byref(m))
            rc = (L.dcn_anchor_map_insertions_fetch(amap._h, 1, 0, LEN1, *tail) if fetch else
                  L.dcn_anchor_map_insertions_call(amap._h, C.byref(prm), 1, 0, LEN1, *tail))
            return rc, items, bases, n.value, m.value

        rc, _, _, n, m = raw(0, 0, nulls=True)
        assert rc == N.DCN_ERR_CAPACITY and (n, m) == (total, total_bases) and str(total).encode() in L.dcn_last_error()
        for cap, base_cap in ((total - 1, total_bases), (total, total_bases - 1), (total - 1, total_bases - 1)):
            rc, items, bases, n, m = raw(cap, base_cap)
            assert rc == N.DCN_ERR_CAPACITY and (n, m) == (total, total_bases) and (items == 0xAB).all() and (bases == 0xAB).all()
        for cap, base_cap in ((total, total_bases), (total + 3, total_bases + 5)):
            rc, items, bases, n, m = raw(cap, base_cap)
            assert rc == 0 and (n, m) == (total, total_bases)
            assert as_tuples(items.view(dtype)[:total], bases[:total_bases].tobytes()) == want
            assert (items[total * dtype.itemsize:] == 0xAB).all() and (bases[total_bases:] == 0xAB).all()
        rc, *_ = raw(total, total_bases, nulls=True)
        assert rc == N.DCN_ERR_ARG and b"is NULL" in L.dcn_last_error()
        # a range without an event: capacity 0 with NULLs succeeds
        n, m = C.c_uint64(9), C.c_uint64(9)
        tail = (None, 0, None, 0, C.byref(n), C.byref(m))
        rc = (L.dcn_anchor_map_insertions_fetch(amap._h, 0, 0, LEN0, *tail) if fetch else L.dcn_anchor_map_insertions_call(amap._h, C.byref(prm), 0, 0, LEN0, *tail))
        assert rc == 0 and (n.value, m.value) == (0, 0)


def test_growth_and_trace_groups_in_processes_of_their_own(env):
    """DCN_INSERTION_LEDGER_EVENTS = 1 (the ledger grows with almost every one of twelve batches) and DCN_ALIGN_TRACE_BYTES = 64
    (groups of one row) in a worker each, which compares with the model; both leave the same ledger, byte for byte"""
    lines = []
    for case, extra in (("grow", dict(DCN_INSERTION_LEDGER_EVENTS="1")), ("groups", dict(DCN_ALIGN_TRACE_BYTES="64"))):
        p = subprocess.run([sys.executable, WORKER, case], capture_output=True, text=True, timeout=300, env=dict(os.environ, **extra))
        assert p.returncode == 0, p.stderr[-2000:]
        line = [x for x in p.stdout.splitlines() if x.startswith("insertions " + case)]
        assert len(line) == 1
        lines.append(line[0].split()[2:])
    assert lines[0] == lines[1] and int(lines[0][0]) >= 15 and int(lines[0][1]) >= 40

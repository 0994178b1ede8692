"""The seams of the deletion ledger's kernels and of the indel genotype (indels.hip, indels_api.hip), with rows written by hand
as tests/test_gpu_pileup_seams.py writes them: two short records, the second starting mid-word of the store; every case is
a call of a few hundred rows (a thousand copies of one read in some) whose counters, both ledgers and sites, both records
from their first base to their last, are compared with the model of tests/_indel_worker.py.  Every comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _align_worker as AW
import _indel_worker as DW
import _insertion_worker as IW
import _pileup_worker as PW
import _verify_worker as VW
from test_gpu_pileup_seams import LEN0, LEN1, Case, make_records, other

pytestmark = pytest.mark.gpu

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_indel_worker.py")
OVER = VW.OVER
LOOSE = dict(min_depth=1, min_gq=0, min_qual=0, min_count=1)


@pytest.fixture(scope="module")
def env(dcn, oracle):
    records = make_records()
    amap = VW.build_map(oracle, dcn, records)
    amap.pileup_enable()
    amap.pileup_keep_insertions()
    amap.pileup_keep_deletions()
    placer = dcn.Placer(amap, max_batch_bases=1 << 21, max_batch_reads=1 << 12)
    yield dcn, oracle, records, amap, placer
    placer.close()
    amap.close()


def run(c, amap, placer, oracle, row_offsets=None, settings=(DW.DEFAULTS, LOOSE), **kw):
    """resets, adds the case's rows, compares counters, both ledgers and the sites of both records with the model ->
    (counts, insertions, deletions, edits, [CIGAR text per row])"""
    rows = np.concatenate(c.rows)
    b, o = oracle.concat_reads(c.reads)
    amap.pileup_reset()
    edits, n_added = placer.pileup_batch(b, o, rows, row_offsets=row_offsets, **kw)
    counts, ins, dels = PW.new_counts(c.records), IW.new_ledger(c.records), DW.new_ledger(c.records)
    want_edits, want_added = DW.pile_rows(counts, ins, dels, c.reads, c.records, rows, row_offsets=row_offsets, **kw)
    assert edits.tolist() == want_edits.tolist() and n_added == want_added
    PW.assert_counts(amap, c.records, counts)
    DW.assert_ledgers(amap, c.records, counts, ins, dels, settings=settings)
    _, offs, cigar = AW.align_rows(c.reads, c.records, rows, row_offsets, **kw)
    return counts, ins, dels, want_edits, [AW.cigar_text(cigar[int(offs[i]):int(offs[i + 1])]) for i in range(len(rows))]


def without(T, at, n=1):
    """T with n bases gone from `at`"""
    return T[:at] + T[at + n:]


def one_run(T, at, n):
    """whether T without n bases from `at` aligns with exactly that D run: rule A3 puts a gap where it meets it first, so bases
    that repeat their neighbours move or split it"""
    want = ([at << 4 | AW.OP_EQ] if at else []) + [n << 4 | AW.OP_D] + ([(len(T) - at - n) << 4 | AW.OP_EQ] if at + n < len(T) else [])
    return [int(x) for x in AW.align_pair(without(T, at, n), T)[1]] == want


def interval_with(record, a0, step, length, at, n):
    """the first a = a0, a0 + step, ... at which record[a : a + length] takes one_run(at, n)"""
    return next(a for a in range(a0, len(record) - length, step) if one_run(record[a:a + length], at, n))


def test_one_run_at_the_seams_of_a_word(env):
    """a D run that begins at bases 0, 15, 16, 31, 32 and 63 of a 64-base interval (at 0 it is the row's first run, at 63 its
    last), on both strands, at read offsets that leave the interval at four offsets of a word; on record 1, whose bases lie
    mid-word, as well"""
    dcn, O, records, amap, placer = env
    c = Case(dcn, records, 80)
    for R, base in ((0, 2000), (1, 1000)):
        for at in (0, 15, 16, 31, 32, 63):
            for rev in (0, 1):
                for pre in (0, 5, 16, 31):
                    n = min(1 + at % 3, 64 - at)
                    a = interval_with(records[R], base + pre, 32, 64, at, n)  # (the same offset in a word of the store)
                    c.put(without(records[R][a:a + 64], at, n), R, a, a + 64, rev, pre=pre)
    counts, ins, dels, edits, cigars = run(c, amap, placer, O)
    assert (edits[1:] <= 3).all() and all(x.count("D") == 1 for x in cigars[1:])
    assert sum(x.endswith("D") for x in cigars) == 16 and sum(x[1:2] == "D" for x in cigars) == 16  # last runs and first runs
    for R in (0, 1):
        assert {e[2] for e in dels[R]} == {0, 1} and {e[1] for e in dels[R]} == {1, 2, 3} and len(dels[R]) == 48


def test_record_ends_do_not_cross(env):
    """a deletion of the last bases of record 0 beside one of the first of record 1, whose first base follows in the store:
    each belongs to its record; candidates at p = 0 of a record"""
    dcn, O, records, amap, placer = env
    c = Case(dcn, records, 81)
    last = next(n for n in range(1, 9) if one_run(records[0][LEN0 - 80:], 80 - n, n))  # the last bases of record 0 ...
    first = [next(n for n in range(1, 9) if one_run(rec[:80], 0, n)) for rec in records]  # ... and the first of each record
    for rev in (0, 1):
        for q in range(3):
            c.put(records[0][LEN0 - 80:LEN0 - last], 0, LEN0 - 80, LEN0, rev)  # D as the last run
            c.put(records[1][first[1]:80], 1, 0, 80, rev)                      # D as the first run
            c.put(records[0][first[0]:80], 0, 0, 80, rev)
            T = records[1][:80]
            c.put(other(T[:1]) * 2 + T, 1, 0, 80, rev)                         # ... and an insertion in front of base 0
    counts, ins, dels, edits, cigars = run(c, amap, placer, O, settings=(dict(min_depth=3), LOOSE))
    assert sorted(set(dels[0])) == [(0, first[0], 0), (0, first[0], 1), (LEN0 - last, last, 0), (LEN0 - last, last, 1)]
    assert sorted(set(dels[1])) == [(0, first[1], 0), (0, first[1], 1)]
    assert len(amap.deletions_fetch(0, LEN0 - last, last)) == 6 and len(amap.deletions_fetch(1, 0, 1)) == 6
    assert len(amap.deletions_fetch(0, LEN0 - last + 1, last - 1)) == 0 if last > 1 else True  # by p alone
    sites = DW.sites_range(counts[1], ins[1], dels[1], 0, LEN1, min_depth=3)
    assert [(s[0], s[1], s[2]) for s in sites] == [(0, DW.INDEL_FRONT, 2), (0, DW.INDEL_DELETION, first[1])]  # I6 at p = 0


def runs_row(T0, n_runs, d_index):
    """(S, n) whose alignment against T0[:n] has n_runs runs, '=' of three bases at the even indices and X of one at the odd
    ones, but a D run of two bases at every index in d_index (odd)"""
    S, at = bytearray(), 0
    for r in range(n_runs):
        if r % 2 == 0:
            S += T0[at:at + 3]
            at += 3
        elif r in d_index:
            at += 2
        else:
            S += other(T0[at:at + 1])
            at += 1
    return bytes(S), at


def test_many_runs_and_long_runs(env):
    """rows of 63, 64, 65 and 129 runs with a D run at the chunks' edges, a row whose runs alternate '=' and D over more than a
    chunk, and deletions of 1, 63, 64 and 65 bases"""
    dcn, O, records, amap, placer = env
    c = Case(dcn, records, 82)
    shapes = [(63, {61}), (64, {63}), (65, {63}), (129, {63}), (129, {65}), (129, {127}), (67, {1}), (129, {1, 63, 65, 127})]

    def fits(a, n_runs, d_index):  # the runs are the ones meant: rule A3 has not moved or split a gap
        S, n = runs_row(records[0][a:a + 700], n_runs, d_index)
        got = AW.align_pair(S, records[0][a:a + n])[1]
        return len(got) == n_runs and {i for i, x in enumerate(got) if int(x) & 15 == AW.OP_D} == d_index

    starts = [next(a for a in range(1500, 3200, 13) if fits(a, *shape)) for shape in shapes]
    for rev in (0, 1):
        for a, (n_runs, d_index) in zip(starts, shapes):
            S, n = runs_row(records[0][a:a + 700], n_runs, d_index)
            c.put(S, 0, a, a + n, rev)
        # a D run at every other index over more than two chunks (rule A3 moves some of them: the model says where)
        S, n = runs_row(records[0][200:900], 141, set(range(1, 141, 2)))
        c.put(S, 0, 200, 200 + n, rev)
        T = records[0][1280:1400]  # (the homopolymer: a gap of any length inside it is one run; elsewhere a long gap is split)
        for ln in (1, 63, 64, 65):
            c.put(without(T, 22, ln), 0, 1280, 1400, rev)
    counts, ins, dels, edits, cigars = run(c, amap, placer, O, max_permille=1000)
    assert (edits[1:] < OVER).all()
    parsed = [AW.parse_cigar(x) for x in cigars[1:]]
    for k, (n_runs, d_index) in enumerate(shapes):
        got = {i for i, x in enumerate(parsed[k]) if int(x) & 15 == AW.OP_D}
        assert len(parsed[k]) == n_runs and got == d_index, (n_runs, sorted(d_index)[:4], cigars[1 + k])
    dense = parsed[len(shapes)]
    # (64 runs of one chunk that are all D cannot exist: runs are maximal, rule A4.  Every other run is the most there can be:
    # 32 of the 64 lanes of each full chunk hold a D run, and 25 of the 51 of the last)
    assert len(dense) == 179 and [sum(int(x) & 15 == AW.OP_D for x in dense[k:k + 64]) for k in (0, 64, 128)] == [32, 32, 25], cigars[1 + len(shapes)]
    assert {1, 63, 64, 65} <= {e[1] for e in dels[0] if 1280 <= e[0] < 1400}


@pytest.mark.parametrize("depth", [1, 64, 1000])
def test_events_at_one_position(env, depth):
    """one read `depth` times through row_offsets: every event in one bucket (the plane's and the cursor's atomic adds)"""
    dcn, O, records, amap, placer = env
    c = Case(dcn, records, 83)
    T = records[0][3000:3150]
    S = without(T, 70, 2)
    c.reads, c.rows = [S], [VW.make_row(c.dtype, 0, 0, 0, len(S), 3000, 3150)] * depth
    counts, ins, dels, _, _ = run(c, amap, placer, O, row_offsets=np.array([0, depth], np.uint64))
    ev = amap.deletions_fetch(0)
    assert len(ev) == depth and len(set(ev["pos"].tolist())) == 1 and (ev["len"] == 2).all()
    sites, _ = amap.indels_genotype(0, min_depth=1, min_gq=0, min_qual=0, min_count=1)
    assert [(int(s["count"]), int(s["events"]), int(s["depth"])) for s in sites] == [(depth, depth, depth)]


@pytest.mark.parametrize("first,second", [(3, 3), (3, 4), (500, 500), (499, 501)])
def test_two_lengths_at_one_start(env, first, second):
    """two deletions of different lengths that begin at one position: a tie goes to the shorter, one event more decides
    otherwise (at a thousand events the quadratic pass over one bucket)"""
    dcn, O, records, amap, placer = env
    c = Case(dcn, records, 84)
    T = records[0][3000:3150]
    at = next(x for x in range(40, 110) if one_run(T, x, 2) and one_run(T, x, 3))
    S1, S2 = without(T, at, 2), without(T, at, 3)
    c.reads = [S1, S2]
    c.rows = [VW.make_row(c.dtype, 0, 0, 0, len(S1), 3000, 3150)] * first + [VW.make_row(c.dtype, 0, 0, 0, len(S2), 3000, 3150)] * second
    counts, ins, dels, _, cigars = run(c, amap, placer, O, row_offsets=np.array([0, first, first + second], np.uint64))
    starts = {e[0] for e in dels[0]}
    assert len(starts) == 1 and {e[1] for e in dels[0]} == {2, 3}, cigars[:1]  # (the two runs begin at one position)
    (site,), _ = amap.indels_genotype(0, min_count=1)
    want = (2, first) if first >= second else (3, second)
    assert (int(site["len"]), int(site["count"]), int(site["events"])) == want + (first + second,)


def genotype_case(env, copies, carriers, ins_carriers=0):
    """`copies` reads over record 1's first 600 bases; `carriers` of them carry a 2-base deletion at 300, `ins_carriers` an
    insertion behind base 330"""
    dcn, O, records, amap, placer = env
    T = records[1][:600]
    c = Case(dcn, records, 85)
    for q in range(copies):
        s = [T[p:p + 1] for p in range(600)]
        if q < carriers:
            s[300] = s[301] = b""
        if q < ins_carriers:
            s[330] += other(T[330:331], T[331:332]) * 2
        c.put(b"".join(s), 1, 0, 600, rev=q % 2)
    return c


def test_thresholds_at_their_boundaries(env):
    """min_count at a - 1, a, a + 1; depth at min_depth - 1 and min_depth; GQ at min_gq - 1 and min_gq; QUAL at min_qual - 1 and
    min_qual; ploidy 1; an insertion site and a deletion site at neighbouring and at one position"""
    dcn, O, records, amap, placer = env
    c = genotype_case(env, 8, 4, 4)
    counts, ins, dels, _, _ = run(c, amap, placer, O)
    base = DW.sites_range(counts[1], ins[1], dels[1], 0, LEN1)
    assert len(base) == 2 and {s[1] for s in base} == {0, DW.INDEL_DELETION} and all(s[6] == 4 and s[5] == 8 and s[8] == 1 for s in base)
    gq, qual = base[0][9], base[0][4]
    assert gq == qual == 55  # 8000 - 2408
    kinds = []
    for params in (dict(min_count=3), dict(min_count=4), dict(min_count=5), dict(min_depth=8), dict(min_depth=9), dict(min_gq=gq), dict(min_gq=gq + 1),
                   dict(min_qual=qual), dict(min_qual=qual + 1), dict(ploidy=1), dict(ploidy=1, min_gq=0, min_qual=0), dict(indel_centi=301, het_centi=2000),
                   dict(indel_centi=0), dict(het_centi=0), dict(indel_centi=100000, het_centi=100000)):
        for start, n in ((0, LEN1), (250, 100)):
            kinds.append(len(DW.assert_sites(amap, counts[1], ins[1], dels[1], 1, start, n, **params)))
    assert kinds[:18:2] == [2, 2, 0, 2, 0, 2, 0, 2, 0]


def test_equal_costs_and_caps(env):
    """equal costs, where the first genotype in order wins; PL at 255 and 256; GQ at 99 and 100"""
    dcn, O, records, amap, placer = env
    for copies, carriers in ((2, 1), (256, 256), (255, 255), (100, 100), (99, 99)):
        c = genotype_case(env, copies, carriers)
        counts, ins, dels, _, _ = run(c, amap, placer, O, settings=(dict(LOOSE, indel_centi=100, het_centi=100), dict(LOOSE, ploidy=1, indel_centi=100)))
        if copies == 2:  # 100, 200, 100: R/R before V/V, so no site
            assert DW.sites_range(counts[1], ins[1], dels[1], 0, LEN1, **dict(LOOSE, indel_centi=100, het_centi=100)) == []
        else:
            (site,) = DW.sites_range(counts[1], ins[1], dels[1], 0, LEN1, **dict(LOOSE, ploidy=1, indel_centi=100))
            assert site[10][0] == min(255, copies) and site[9] == min(99, copies)


def test_sites_around_a_workgroup_edge_and_in_the_last_position(env):
    """sites at positions 255, 256 and 257 of a range, in its last position, and ranges that begin and end between them"""
    dcn, O, records, amap, placer = env
    T = records[1][:600]
    c = Case(dcn, records, 86)
    for q in range(7):
        s = [T[p:p + 1] for p in range(600)]
        for p in (255, 256, 257, 599):
            s[p] += other(T[p:p + 1], T[p + 1:p + 2] or T[p:p + 1]) * (1 + p % 2)
        s[100] = s[101] = b""
        s[400] = b""
        c.put(b"".join(s), 1, 0, 600, rev=q % 2)
    counts, ins, dels, _, _ = run(c, amap, placer, O, settings=(dict(min_depth=3), LOOSE))
    want = DW.sites_range(counts[1], ins[1], dels[1], 0, LEN1, min_depth=3)
    assert {255, 256, 257, 599} <= {s[0] for s in want} and len(want) >= 6
    d0 = min(e[0] for e in dels[1])
    for start, n in ((0, 600), (0, 256), (0, 257), (255, 1), (255, 2), (256, 2), (256, 1), (257, 343), (1, 255), (1, 256), (258, 42), (599, 1), (0, 1),
                     (d0, 1), (d0 + 1, 5), (d0 - 3, 4), (600, LEN1 - 600), (37, 0), (LEN1, 0)):
        DW.assert_sites(amap, counts[1], ins[1], dels[1], 1, start, n, min_depth=3)
        assert DW.deletions_as_tuples(amap.deletions_fetch(1, start, n)) == DW.fetch_range(dels[1], start, n), (start, n)


def test_a_front_insertion_and_one_behind_at_one_position(env):
    """a row that begins with an I run and has another behind its first base: two events at p = 0 of the interval, one
    candidate (L5: on a tie the one behind the position)"""
    dcn, O, records, amap, placer = env
    c = Case(dcn, records, 87)
    T = records[0][3200:3300]
    x, y = other(T[:1]), other(T[:1], T[1:2])
    for q in range(8):
        c.put(x * 2 + T[:1] + y + T[1:], 0, 3200, 3300, rev=q % 2)
    counts, ins, dels, _, cigars = run(c, amap, placer, O, max_permille=1000)
    assert int(counts[0][3200, PW.INS]) == 16, cigars[1]
    (site,) = DW.sites_range(counts[0], ins[0], dels[0], 0, LEN0)
    assert (site[0], site[1], site[6], site[7]) == (3200, 0, 8, 16)  # the one behind wins the tie; a = 8 of e = 16


def worker(case, **extra):
    """one case of tests/_indel_worker.py in a process of its own, which compares with the model -> the fields behind its name"""
    p = subprocess.run([sys.executable, WORKER, case], capture_output=True, text=True, timeout=300, env=dict(os.environ, **extra))
    assert p.returncode == 0, p.stderr[-2000:]
    line = [x for x in p.stdout.splitlines() if x.startswith("indels " + case)]
    assert len(line) == 1
    return line[0].split()[2:]


def test_growth_and_trace_groups_in_processes_of_their_own(env):
    """DCN_DELETION_LEDGER_EVENTS = 1 (the ledger grows with almost every one of twelve batches) and DCN_ALIGN_TRACE_BYTES = 256
    (several trace groups) leave the same ledger and sites, byte for byte"""
    grow, groups = worker("grow", DCN_DELETION_LEDGER_EVENTS="1"), worker("groups", DCN_ALIGN_TRACE_BYTES="256")
    assert grow == groups and int(grow[0]) >= 15 and int(grow[1]) == 2 * int(grow[0])


def test_the_second_trip_of_the_appends_work_loop(env):
    """DCN_GRID_CUS = 1 with three hundred rows: 128 waves a trip"""
    assert int(worker("trips", DCN_GRID_CUS="1")[0]) >= 200

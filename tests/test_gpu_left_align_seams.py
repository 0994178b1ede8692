"""The seams of the left-align kernel (left_align.hip, dcn_left_align.h) through dcn_left_align_batch, with rows written by
hand as tests/test_gpu_pileup_seams.py writes them: its two short records, the second starting mid-word of the store, with
homopolymers, tandem repeats and two-letter stretches written into both.  Every case is one call of a handful to a few
hundred rows of tens to a few hundred bases; edits, offsets, runs and the four totals are compared with the model of
tests/_left_align_worker.py, which moves gaps one column at a time.  What a case is meant to reach (a gap that takes 64
steps, a row whose run count grows, two gaps that merge ...) is asserted on the model's own runs before and after, so a
change to the records cannot turn a case into another one silently.  Every comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _align_worker as AW
import _left_align_worker as LW
import _verify_worker as VW
from conftest import random_reads
from test_gpu_pileup_seams import Case, make_records, other

pytestmark = pytest.mark.gpu

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_left_align_worker.py")
OVER, UNPLACED = VW.OVER, VW.UNPLACED
STEPS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129)
HP0, HP1, HP_LEN = 600, 500, 140  # a homopolymer of 140 in each record: A in record 0, T in record 1
TWO0, TWO1, TWO_LEN = 2400, 900, 600  # stretches over two letters: a gap almost always has a repeat in front of it


def seam_records():
    rng = np.random.default_rng(2230)
    a, b = (bytearray(r) for r in make_records())
    a[HP0 - 1:HP0 + HP_LEN + 1] = b"C" + b"A" * HP_LEN + b"G"
    b[HP1 - 1:HP1 + HP_LEN + 1] = b"G" + b"T" * HP_LEN + b"C"
    a[1999:2041] = b"G" + b"AC" * 20 + b"T"
    a[2099:2146] = b"G" + b"ACT" * 15 + b"G"
    a[TWO0:TWO0 + TWO_LEN] = random_reads(rng, 1, TWO_LEN, TWO_LEN, alphabet=b"AC")[0]
    b[TWO1:TWO1 + TWO_LEN] = random_reads(rng, 1, TWO_LEN, TWO_LEN, alphabet=b"GT")[0]
    b[88:100], b[103:118] = b"A" * 12, b"A" * 15  # around the three N of record 1
    return [bytes(a), bytes(b)]


@pytest.fixture(scope="module")
def env(dcn, oracle):
    records = seam_records()
    amap = VW.build_map(oracle, dcn, records)
    placer = dcn.Placer(amap, max_batch_bases=1 << 21, max_batch_reads=1 << 12)
    yield dcn, oracle, records, amap, placer
    placer.close()
    amap.close()


def modelled(c, **kw):
    """the model alone -> (per row the runs as text before, after, the info)"""
    rows = np.concatenate(c.rows)
    _, o0, c0 = AW.align_rows(c.reads, c.records, rows, **kw)
    want = LW.left_align_rows(c.reads, c.records, rows, **kw)
    _, o1, c1, info = want
    text = [(AW.cigar_text(c0[int(o0[i]):int(o0[i + 1])]), AW.cigar_text(c1[int(o1[i]):int(o1[i + 1])])) for i in range(1, len(rows))]
    return want, [t[0] for t in text], [t[1] for t in text], info


def run(c, placer, oracle, **kw):
    """one call against the model -> (runs as text before, after, info), the first read's unplaced row left out"""
    rows = np.concatenate(c.rows)
    b, o = oracle.concat_reads(c.reads)
    want, before, after, info = modelled(c, **kw)
    got = placer.left_align_batch(b, o, rows, **kw)
    AW.assert_same(got[:3], want[:3], rows)
    assert got[3] == info, (got[3], info)
    return before, after, info


def gap_at(cigar, kind):
    """the bases in front of the first run of `kind` in a row's runs, counted in its own sequence (T for D, S for I)"""
    at = 0
    for x in AW.parse_cigar(cigar):
        ln, op = int(x) >> 4, int(x) & 15
        if AW.LETTER[op] == kind:
            return at
        if op != (AW.OP_I if kind == "D" else AW.OP_D):
            at += ln
    return None


def homopolymer_case(dcn, records):
    """a one-base D and a one-base I that take k steps each, k in STEPS, in both records on both strands: the row begins inside
    the homopolymer, k + 2 bases in front of its end (k + 1 for the I, whose read has a base more), so the row's first column
    stops the gap; read offsets and record offsets leave the passed stretch over the edges of the store's words"""
    c = Case(dcn, records, 2231)
    for R, hp in ((0, HP0), (1, HP1)):
        end = hp + HP_LEN
        for k in STEPS:
            for rev in (0, 1):
                a = end - (k + 2)
                T = records[R][a:end + 9]
                c.put(T[1:], R, a, end + 9, rev, pre=(k + rev) % 7)              # D: a base of the homopolymer gone
                T = records[R][a + 1:end + 9]
                c.put(T[:1] + T, R, a + 1, end + 9, rev, pre=(3 * k + rev) % 11)  # I: one more
    return c


def test_homopolymer_steps(env):
    dcn, O, records, amap, placer = env
    c = homopolymer_case(dcn, records)
    before, after, info = run(c, placer, O, max_permille=1000)
    k_of = [k for _ in (0, 1) for k in STEPS for _ in range(4)]
    for i, k in enumerate(k_of):
        kind = "DI"[(i % 2)]
        assert before[i].count(kind) == 1 and gap_at(before[i], kind) - gap_at(after[i], kind) == k, (k, kind, before[i], after[i])
        assert after[i].startswith("1=1" + kind)  # stopped by the row's first column: the gap is the second run, never the first
    assert info["rows_changed"] == info["rows_aligned"] == 88 and info["gaps_merged"] == 0 and info["columns_passed"] == 8 * sum(STEPS)


def test_tandem_repeats_and_long_gaps(env):
    """gaps of 2 and 3 bases in the period-2 and the period-3 repeat, and gaps of 1 - 65 bases cut out of a homopolymer (a D)
    or put into it (an I): each ends directly behind the base in front of the repeat"""
    dcn, O, records, amap, placer = env
    c = Case(dcn, records, 2232)
    for rev in (0, 1):
        T = records[0][1990:2050]
        c.put(T[:40] + T[42:], 0, 1990, 2050, rev)             # a unit of AC gone
        c.put(T[:40] + b"AC" + T[40:], 0, 1990, 2050, rev)     # ... and come
        c.put(T[:30] + T[34:], 0, 1990, 2050, rev)             # two units
        T = records[0][2090:2160]
        c.put(T[:40] + T[43:], 0, 2090, 2160, rev)             # a unit of ACT
        c.put(T[:40] + b"ACT" + T[40:], 0, 2090, 2160, rev)
    for ln in list(range(1, 66, 7)) + [63, 64, 65]:
        T = records[1][HP1 - 5:HP1 + HP_LEN + 5]
        c.put(T[:60] + T[60 + ln:], 1, HP1 - 5, HP1 + HP_LEN + 5, ln % 2)
        c.put(T[:60] + b"T" * ln + T[60:], 1, HP1 - 5, HP1 + HP_LEN + 5, 1 - ln % 2)
    before, after, info = run(c, placer, O, max_permille=1000)
    assert [x[:5] for x in after[:5]] == ["10=2D", "10=2I", "10=4D", "10=3D", "10=3I"] and after[5:10] == after[:5], after[:10]
    assert all(x != y for x, y in zip(before, after))
    assert all(x.startswith("5=%d%s" % (ln, kind)) for x, (ln, kind) in zip(after[10:], [(ln, k) for ln in list(range(1, 66, 7)) + [63, 64, 65] for k in "DI"]))
    assert info["rows_changed"] == info["rows_aligned"]


def read_n_spot(record, lo, hi):
    """p in [lo, hi): record[p] is followed by two equal bases that differ from it and from the base behind them.  A read with N
    for record[p] and one more of the repeated base aligns with an X at the N and an I that moves up to it"""
    for p in range(lo, hi):
        T = record[p - 20:p + 20]
        if len({T[20], T[21]}) == 2 and T[21] == T[22] != T[23] and T[19] != T[21]:
            S = T[:20] + b"N" + T[21:23] + T[21:22] + T[23:]
            d, runs = AW.align_pair(S, T)
            new = LW.left_align(S, T, runs)[0]
            if d == 2 and "1X1I" in AW.cigar_text(new) and new != [int(x) for x in runs]:
                return p, S
    raise AssertionError("no spot")


def test_stops(env):
    """an invalid base of the record, which stops a D; an invalid base of the read, which stops an I; a gap that A3 put first,
    which stays first; rows whose gaps cannot move and rows without gaps, which come back as dcn_align_batch gives them; OVER
    and UNPLACED rows, which have no runs (a base that differs stops the gaps of the case above)"""
    dcn, O, records, amap, placer = env
    c = Case(dcn, records, 2233)
    p, S_n = read_n_spot(records[0], 3400, 3900)
    for rev in (0, 1):
        T = records[1][80:130]  # ... 12 A, NNN, 15 A ...
        c.put(T[:35] + T[36:], 1, 80, 130, rev)                                  # an A gone behind the N: stops at the N
        c.put(S_n, 0, p - 20, p + 20, rev)                                       # an A more behind the read's N: stops at the N
        a = next(a for a in range(3300, 3400) if AW.cigar_text(AW.align_pair(records[0][a + 2:a + 40], records[0][a:a + 40])[1]) == "2D38=")
        T = records[0][a:a + 40]
        c.put(T[2:], 0, a, a + 40, rev)                                          # a D run first
        c.put(other(T[:1]) * 2 + T, 0, a, a + 40, rev)                           # an I run first
        T = records[0][3300:3380]
        c.put(T, 0, 3300, 3380, rev)                                             # no gap
        c.put(T[:40] + other(T[39:40], T[40:41]) + T[40:], 0, 3300, 3380, rev)   # an insertion that cannot move
        c.put(random_reads(c.rng, 1, 80, 80)[0], 0, 3300, 3380, rev)             # OVER
        c.unplaced()
    before, after, info = run(c, placer, O)
    for at in (0, 8):
        x, y = before[at:at + 8], after[at:at + 8]
        assert "3X1D" in y[0] and x[0] != y[0], (x[0], y[0])
        assert "1X1I" in y[1] and x[1] != y[1], (x[1], y[1])
        assert x[2] == y[2] == "2D38=" and x[3] == y[3] == "2I40="  # first gaps stay first
        assert x[4] == y[4] == "80=" and x[5] == y[5] and "I" in y[5] and y[6] == "" and y[7] == ""
    assert info["rows_aligned"] == 12 and info["rows_changed"] == 4


def two_letter_case(dcn, records, seed, n_rows, length, edits):
    c = Case(dcn, records, seed)
    rng = np.random.default_rng(seed)
    for q in range(n_rows):
        R, two, other_letters = ((0, TWO0, b"AC"), (1, TWO1, b"GT"))[q % 2]
        a = two + int(rng.integers(0, TWO_LEN - length))
        T = records[R][a:a + length]
        S = bytearray(T)
        for _ in range(edits(q)):
            at, kind, ln = int(rng.integers(1, len(S))), int(rng.integers(0, 3)), int(rng.integers(1, 4))
            if kind == 0:
                S[at] = other_letters[int(S[at] == other_letters[0])]
            elif kind == 1:
                del S[at:at + ln]
            else:
                S[at:at] = bytes(rng.choice(np.frombuffer(other_letters, np.uint8), ln))
        c.put(bytes(S), R, a, a + length, rev=(q // 2) % 2)
    return c


def test_passing_runs_and_merging_gaps(env):
    """a hundred and sixty short rows over two letters with two to five planted edits: gaps that pass X columns, run counts
    that grow and that shrink, gaps of either kind that merge, a gap that merges into a leading gap"""
    dcn, O, records, amap, placer = env
    c = two_letter_case(dcn, records, 2234, 160, 48, lambda q: 2 + q % 4)
    T = records[0][HP0 - 1:HP0 + 12]
    c.put(T[2:8] + T[9:], 0, HP0 - 1, HP0 + 12)  # C and an A gone, then another A: a gap that merges into a leading gap
    before, after, info = run(c, placer, O, max_permille=1000)
    runs = [(AW.parse_cigar(x), AW.parse_cigar(y)) for x, y in zip(before, after)]
    assert sum(len(y) == len(x) + 1 for x, y in runs) >= 3 and sum(len(y) < len(x) for x, y in runs) >= 3
    assert info["gaps_merged"] >= 5 and info["rows_changed"] >= 60

    def gap_bases_in_front_of_each_x(rs):
        out, gaps = [], 0
        for r in rs:
            if (int(r) & 15) in LW.GAPS:
                gaps += int(r) >> 4
            elif (int(r) & 15) == AW.OP_X:
                out += [gaps] * (int(r) >> 4)
        return out
    assert sum(any(q > p for p, q in zip(gap_bases_in_front_of_each_x(x), gap_bases_in_front_of_each_x(y))) for x, y in runs) >= 3  # X columns that a gap passed
    kinds = {AW.LETTER[int(r) & 15] for x, y in runs if len(y) < len(x) for r in y}
    assert {"D", "I"} <= kinds
    lead_before, lead_after = runs[-1]
    assert (int(lead_before[0]) & 15) == AW.OP_D and (int(lead_after[0]) & 15) == AW.OP_D and (int(lead_after[0]) >> 4) > (int(lead_before[0]) >> 4), (before[-1], after[-1])


def test_run_count_seams(env):
    """long rows over two letters with dozens of edits: from under 64 runs to over 129 (the kernel reads 64 runs a round), more
    than 64 gaps in one row, gaps in every round, gaps that merge across rounds"""
    dcn, O, records, amap, placer = env
    c = two_letter_case(dcn, records, 2235, 48, 500, lambda q: 20 + 7 * (q % 24))
    before, after, info = run(c, placer, O, max_permille=1000)
    runs = [(AW.parse_cigar(x), AW.parse_cigar(y)) for x, y in zip(before, after)]
    counts = sorted(len(x) for x, _ in runs)
    assert counts[0] < 64 < 129 < counts[-1] and sum(64 < n < 128 for n in counts) >= 5, counts
    assert max(sum((int(r) & 15) in LW.GAPS for r in x) for x, _ in runs) > 64
    assert info["rows_changed"] >= 40 and info["gaps_merged"] >= 20


def exact_runs_row(record, n_runs):
    """(S, T, a): T = record[a : ...] in the two-letter stretch, S = T with a single-base edit behind every three bases such that
    rule A3's alignment has exactly n_runs runs of which every second is one edit, so n_runs = 2 d + 1 when it is odd: a full
    slot.  Some edits are D runs in front of which the base repeats, so that they move, and the left-aligned row has n_runs
    runs again"""
    for a in range(TWO0, TWO0 + 150):
        T = record[a:a + 2 * n_runs + 3]
        S, at, n = bytearray(), 0, 0
        while n + 2 < n_runs:
            S += T[at:at + 3]
            if T[at + 3:at + 4] == T[at + 2:at + 3] and n % 8 == 0:
                pass  # a D behind a base that repeats it
            else:
                S += other(T[at + 3:at + 4], b"A", b"C")  # an X that no base of the stretch equals
            at += 4
            n += 2
        S += T[at:at + 3]
        if n_runs % 2 == 0:
            S += b"G"  # an even count: the last run is an X
            at += 1
        S, T = bytes(S), T[:at + 3]
        d, runs = AW.align_pair(S, T)
        new, (shifted, passed, merges) = LW.left_align(S, T, runs)
        if len(runs) == n_runs == len(new) and shifted >= 1 + (n_runs > 64) and sum((int(r) & 15) == AW.OP_EQ for r in runs) == (n_runs + 1) // 2 and \
                (n_runs % 2 == 0 or n_runs == 2 * d + 1):
            return S, T, a
    raise AssertionError("no row of %d runs" % n_runs)


def lane_zero_row(record):
    """(S, T, a): 62 runs in front of the homopolymer of record 0, X and '=' of three bases in turn, the last of which ends with the base in
    front of the homopolymer; then an X on its first base (run 62), nine '=' (run 63) and a D (run 64, lane 0 of the second
    round of 64), which passes both and stops behind run 61"""
    a = HP0 - 124
    T = record[a:HP0 + 11]
    S = b"".join(other(T[4 * g:4 * g + 1]) + T[4 * g + 1:4 * g + 4] for g in range(31)) + b"G" + b"A" * 9
    return S, T, a


def test_exact_run_counts(env):
    """rows of exactly 63, 64, 65 and 129 runs with gaps that move; rows at n_ops = 2 d + 1 before and after; a gap in lane 0
    of the second round whose steps pass runs 62 and 63 of the first"""
    dcn, O, records, amap, placer = env
    c = Case(dcn, records, 2236)
    want = (63, 64, 65, 129)
    for n_runs in want:
        S, T, a = exact_runs_row(records[0], n_runs)
        c.put(S, 0, a, a + len(T), rev=n_runs % 2)
    S, T, a = lane_zero_row(records[0])
    for rev in (0, 1):
        c.put(S, 0, a, a + len(T), rev)
    before, after, info = run(c, placer, O, max_permille=1000)
    for n_runs, x, y in zip(want, before, after):
        bx, ay = AW.parse_cigar(x), AW.parse_cigar(y)
        assert len(bx) == len(ay) == n_runs and bx != ay, (n_runs, x, y)
    for x, y in zip(before[4:], after[4:]):
        bx, ay = AW.parse_cigar(x), AW.parse_cigar(y)
        assert len(bx) == 65 and x.endswith("1X9=1D") and bx[:62] == ay[:62] and y.endswith("1D1X9="), (x, y)
    assert info["rows_changed"] == 6


def test_capacity_protocol(env):
    """the capacity protocol with the new counts: one run too few is DCN_ERR_CAPACITY with complete offsets and info; the exact
    capacity succeeds; NULL with capacity 0 asks"""
    dcn, O, records, amap, placer = env
    c = two_letter_case(dcn, records, 2237, 12, 60, lambda q: 3)
    rows = np.concatenate(c.rows)
    b, o = O.concat_reads(c.reads)
    want = LW.left_align_rows(c.reads, c.records, rows, max_permille=1000)
    plain = AW.align_rows(c.reads, c.records, rows, max_permille=1000)
    total = int(want[1][-1])
    assert total != int(plain[1][-1])  # (the counts are the new ones)
    for cap in (total - 1, 0):
        with pytest.raises(dcn.DeaconHipError) as e:
            placer.left_align_batch(b, o, rows, max_permille=1000, capacity=cap)
        assert e.value.code == dcn._native.DCN_ERR_CAPACITY and ("the rows have %d" % total) in str(e.value)
    got = placer.left_align_batch(b, o, rows, max_permille=1000, capacity=total)
    AW.assert_same(got[:3], want[:3], rows)
    assert got[3] == want[3]
    again = placer.align_batch(b, o, rows, max_permille=1000)  # the call beside it is what it was, on the same context
    AW.assert_same(again, plain, rows)


def worker(case, **extra):
    p = subprocess.run([sys.executable, WORKER, case], capture_output=True, text=True, timeout=300, env=dict(os.environ, **extra))
    assert p.returncode == 0, p.stderr[-2000:]
    line = [x for x in p.stdout.splitlines() if x.startswith("left_align " + case)]
    assert len(line) == 1
    return line[0].split()[2:]


def test_trace_groups_in_a_process_of_its_own():
    """DCN_ALIGN_TRACE_BYTES of a few hundred bytes: many trace groups, and the pass runs once, behind the last.  The worker
    compares with the model, which knows no groups"""
    fields = worker("groups", DCN_ALIGN_TRACE_BYTES="300")
    assert "('rows_changed',29)" in fields[-1], fields[-1]


def test_the_second_trip_of_the_work_loop():
    """DCN_GRID_CUS = 1 with a few hundred rows: 128 waves a trip"""
    aligned, changed = (int(x) for x in worker("trips", DCN_GRID_CUS="1"))
    assert aligned >= 256 and changed >= 80

"""The seams of dcn_pileup_batch_qual and of the quality form of the pileup kernel (pileup.hip), with rows and qualities written
by hand as tests/test_gpu_pileup_seams.py writes its rows: two short records, the second starting mid-word of the store;
every case is a call of a few hundred rows (a thousand copies of one read in one case) whose counters and quality sums,
both records from their first base to their last, are compared with the model of tests/_quality_worker.py, with the ledger
beside them.  Every comparison is exact.

A case is built by put(): the read is flank + S + flank behind a first read of 37 bases with an unplaced row, so the row's
read is never the batch's first and its interval starts behind a soft clip (read_start = pre) wherever pre > 0.  q is given
in S's order: on a reverse row the read's quality line holds it turned round, as the read holds S."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _align_worker as AW
import _insertion_worker as IW
import _pileup_worker as PW
import _quality_worker as QW
import _verify_worker as VW
from conftest import random_reads
from test_gpu_insertions_seams import behind, foreign
from test_gpu_pileup_seams import LEN1, Case, make_records, other

pytestmark = pytest.mark.gpu

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_quality_worker.py")
UNPLACED, OVER = VW.UNPLACED, VW.OVER
HIGH = 35


@pytest.fixture(scope="module")
def env(dcn, oracle):
    records = make_records()
    amap = VW.build_map(oracle, dcn, records)
    amap.pileup_enable()
    amap.pileup_keep_insertions()
    amap.pileup_keep_qualities()
    placer = dcn.Placer(amap, max_batch_bases=1 << 21, max_batch_reads=1 << 12)
    yield dcn, oracle, records, amap, placer
    placer.close()
    amap.close()


class QCase(Case):
    """Case with one quality line per read"""

    def __init__(self, dcn, records, seed, qual_offset=33):
        super().__init__(dcn, records, seed)
        self.qual_offset = qual_offset
        self.quals = [self.line(len(self.reads[0]))]

    def line(self, n):
        return (self.rng.integers(0, 42, n) + self.qual_offset).astype(np.uint8).tobytes()

    def put(self, S, q, R, a, b, rev=0, pre=None, raw=False):
        """q: the qualities of S's bases (raw: the bytes themselves), or one number for all of them"""
        q = [q] * len(S) if isinstance(q, int) else list(q)
        assert len(q) == len(S)
        super().put(S, R, a, b, rev, pre)
        read, row = self.reads[-1], self.rows[-1]
        pre, end = int(row["read_start"][0]), int(row["read_end"][0])
        mid = bytes(x if raw else x + self.qual_offset for x in (q[::-1] if rev else q))
        self.quals.append(self.line(pre) + mid + self.line(len(read) - end))

    def unplaced(self):
        super().unplaced()
        self.quals.append(self.line(len(self.reads[-1])))


def run(c, amap, placer, oracle, min_base_qual=20, row_offsets=None, **kw):
    """resets, adds the case's rows with their qualities, compares counters, sums and ledger of both records with the model
    -> (counts, sums, edits, [CIGAR text per row])"""
    rows = np.concatenate(c.rows)
    b, o, q = QW.concat(oracle, c.reads, c.quals)
    amap.pileup_reset()
    edits, n_added = placer.pileup_batch(b, o, rows, row_offsets=row_offsets, quals=q, min_base_qual=min_base_qual, qual_offset=c.qual_offset, **kw)
    counts, sums, ledger = PW.new_counts(c.records), QW.new_sums(c.records), IW.new_ledger(c.records)
    want_edits, want_added = QW.pile_rows(counts, sums, ledger, c.reads, c.quals, c.records, rows, row_offsets=row_offsets,
                                          min_base_qual=min_base_qual, qual_offset=c.qual_offset, **kw)
    assert edits.tolist() == want_edits.tolist() and n_added == want_added
    PW.assert_counts(amap, c.records, counts)
    QW.assert_sums(amap, c.records, sums)
    IW.assert_ledger(amap, c.records, counts, ledger, fills=(False,))
    _, offs, cigar = AW.align_rows(c.reads, c.records, rows, row_offsets, **kw)
    return counts, sums, want_edits, [AW.cigar_text(cigar[int(offs[i]):int(offs[i + 1])]) for i in range(len(rows))]


def one_low(n, at, low=3):
    q = [HIGH] * n
    q[at] = low
    return q


def test_one_low_base_at_the_seams_of_a_word(env):
    """one low-quality base at S positions 0, 15, 16, 31, 32 and the last of a 64-base interval, on both strands, at read
    offsets that leave the interval at four offsets of a word (behind a soft clip for pre > 0, never in the batch's first
    read); on record 1, whose bases lie mid-word, as well: exactly that position of T counts in N and sums nothing"""
    dcn, O, records, amap, placer = env
    c = QCase(dcn, records, 80)
    where = []
    for R, base in ((0, 2000), (1, 1000)):
        for at in (0, 15, 16, 31, 32, 63):
            for rev in (0, 1):
                for pre in (0, 5, 16, 31):
                    a = base + pre
                    c.put(records[R][a:a + 64], one_low(64, at), R, a, a + 64, rev, pre=pre)
                    where.append((R, a + at))
    counts, sums, edits, cigars = run(c, amap, placer, O)
    assert (edits[1:] == 0).all() and set(cigars[1:]) == {"64="}
    for R in (0, 1):
        low = {p for r, p in where if r == R}
        assert set(np.flatnonzero(counts[R][:, PW.N]).tolist()) == low  # (record 1's NNN is elsewhere)
        n_here = sum(1 for r, _ in where if r == R)
        assert int(counts[R][:, PW.N].sum()) == n_here and int(sums[R].sum()) == HIGH * 63 * n_here


def test_a_ramp_on_a_reverse_row(env):
    """asymmetric qualities: q(S[i]) = i on both strands over 60 bases at threshold 20; a mirrored index would put the N half
    at the other end and show in every sum"""
    dcn, O, records, amap, placer = env
    c = QCase(dcn, records, 81)
    for R, a in ((0, 500), (1, 300)):
        for rev in (0, 1):
            for pre in (0, 13):
                c.put(records[R][a:a + 60], list(range(60)), R, a, a + 60, rev, pre=pre)
    counts, sums, edits, _ = run(c, amap, placer, O)
    for R, a in ((0, 500), (1, 300)):
        assert counts[R][a:a + 20, PW.N].tolist() == [4] * 20 and not counts[R][a + 20:a + 60, PW.N].any()
        assert sums[R][a:a + 60].sum(axis=1).tolist() == [0] * 20 + [4 * i for i in range(20, 60)]
        assert counts[R][a:a + 60, PW.REV].tolist() == [2] * 60


def test_a_low_base_under_every_op(env):
    """a low-quality base under '=', under X, just behind a D run and just behind an I run; a low-quality inserted base changes
    nothing; an N of high quality stays N without a sum"""
    dcn, O, records, amap, placer = env
    c = QCase(dcn, records, 82)
    want_n = []
    for R, a in ((0, 2500), (1, 600)):
        T = records[R][a:a + 80]
        for rev in (0, 1):
            c.put(T, one_low(80, 40), R, a, a + 80, rev)                                           # '='
            X = T[:40] + other(T[40:41]) + T[41:]
            c.put(X, one_low(80, 40), R, a, a + 80, rev)                                           # X, low: N
            c.put(X, HIGH, R, a, a + 80, rev)                                                      # X, high: the other letter, with its sum
            D = T[:38] + T[40:]
            c.put(D, one_low(78, 38), R, a, a + 80, rev)                                           # behind a D run of two: S[38] on T[40]
            ins = foreign(T, 39, 2)
            c.put(behind(T, 39, ins), one_low(82, 42), R, a, a + 80, rev)                          # behind an I run of two: S[42] on T[40]
            c.put(behind(T, 39, ins), [HIGH] * 40 + [0, 0] + [HIGH] * 40, R, a, a + 80, rev)       # the inserted bases are low
            c.put(T[:40] + b"N" + T[41:], 41, R, a, a + 80, rev)                                   # an N of high quality
            want_n.append((R, a + 40, 5))
    counts, sums, edits, cigars = run(c, amap, placer, O)
    assert cigars[1:8] == ["80=", "40=1X39=", "40=1X39=", "38=2D40=", "40=2I40=", "40=2I40=", "40=1X39="], cigars[1:8]
    for R, p, n in want_n:
        assert int(counts[R][p, PW.N]) == 2 * n and int(counts[R][p, :4].sum()) == 4  # (per strand: the X of high quality and the low inserted one's '=')


def runs_row(T0, n_runs):
    """(S, bases of T) whose alignment has n_runs runs: '=' of three bases at the even indices and X of one at the odd ones"""
    S, at = bytearray(), 0
    for r in range(n_runs):
        if r % 2 == 0:
            S += T0[at:at + 3]
            at += 3
        else:
            S += other(T0[at:at + 1])
            at += 1
    return bytes(S), at


def test_many_runs_and_long_runs(env):
    """rows of 63, 64, 65 and 129 runs with the low-quality base in the 63rd, the 64th and the 65th run where the row has one
    (what a chunk of 64 runs hands the next: i), and runs of 63, 64, 65 bases with it at index 63 and 64 of the run (the
    lanes' stride)"""
    dcn, O, records, amap, placer = env
    c = QCase(dcn, records, 83)
    shapes = [63, 64, 65, 129]
    for rev in (0, 1):
        for n_runs in shapes:
            S, n = runs_row(records[0][1000:1400], n_runs)
            for run_index in (62, 63, 64):  # S's first base of that run: two bases per pair of runs in front of it
                at = (run_index // 2) * 4 + (3 if run_index % 2 else 0)
                if at < len(S):
                    c.put(S, one_low(len(S), at), 0, 1000, 1000 + n, rev)
        for ln in (63, 64, 65):  # X, one long '=' run, X: the run begins at S[1]
            T = records[1][400:402 + ln]
            S = other(T[:1]) + T[1:1 + ln] + other(T[1 + ln:])
            for k in (63, 64):
                if k < ln:
                    c.put(S, one_low(len(S), 1 + k), 1, 400, 402 + ln, rev)
            c.put(S, one_low(len(S), ln), 1, 400, 402 + ln, rev)  # the run's last base
    counts, sums, edits, cigars = run(c, amap, placer, O, max_permille=1000)
    assert (edits[1:] < OVER).all()
    assert {len(AW.parse_cigar(x)) for x in cigars[1:]} >= {63, 64, 65, 129, 3}
    assert any(x == "1X63=1X" for x in cigars) and any(x == "1X64=1X" for x in cigars) and any(x == "1X65=1X" for x in cigars)
    assert int(counts[0][:, PW.N].sum()) + int(counts[1][:, PW.N].sum()) == len(c.rows) - 1  # one low base per row, each on a base of T


def test_thresholds_offsets_and_bytes(env):
    """q at the threshold and one below; a byte below the offset; byte 255; thresholds 0 and 255; another offset"""
    dcn, O, records, amap, placer = env
    T = records[0][3000:3064]
    for offset, threshold, raw, n_low in ((33, 20, [53] * 16 + [52] * 16 + [32, 0, 10, 33] * 4 + [255] * 16, 32),
                                          (33, 0, [53] * 16 + [52] * 16 + [32, 0, 10, 33] * 4 + [255] * 16, 0),
                                          (0, 255, [255] * 16 + [254] * 16 + [0] * 32, 48),
                                          (33, 255, [255] * 64, 64),
                                          (64, 30, [94] * 32 + [93] * 32, 32),
                                          (255, 1, [255] * 32 + [254] * 32, 64),
                                          (0, 1, [0, 1] * 32, 32)):
        c = QCase(dcn, records, 84, qual_offset=offset)
        for rev in (0, 1):
            c.put(T, raw, 0, 3000, 3064, rev, raw=True)
        counts, sums, _, _ = run(c, amap, placer, O, min_base_qual=threshold)
        assert int(counts[0][:, PW.N].sum()) == 2 * n_low, (offset, threshold)
        want = sum(QW.quality(x, offset) for x in raw if QW.quality(x, offset) >= threshold)
        assert int(sums[0].sum()) == 2 * want, (offset, threshold)


def test_rows_that_add_nothing(env):
    """UNPLACED, OVER, n = 0 and m = 0 rows between adding ones: their qualities are never looked at"""
    dcn, O, records, amap, placer = env
    c = QCase(dcn, records, 85)
    T = records[1][60:300]
    c.put(T, one_low(240, 7), 1, 60, 300)
    c.put(records[0][500:520], 2, 0, 700, 700)           # n = 0: 20I, adds nothing
    c.unplaced()
    c.put(T, one_low(240, 7), 1, 60, 300, rev=1)
    c.put(random_reads(c.rng, 1, 100, 100)[0], 40, 0, 900, 1000)  # OVER under the default threshold
    c.put(b"", [], 0, 800, 820, pre=7)                   # m = 0
    c.put(T, HIGH, 1, 60, 300, rev=1)
    for permille in (1000, 200):
        counts, sums, edits, cigars = run(c, amap, placer, O, max_permille=permille)
        assert edits[3] == UNPLACED and (edits[2] == 20) == (permille == 1000)
        assert int(counts[1][60:300, :6].sum()) == 3 * 240 and int(counts[1][:, PW.N].sum()) == 2 + 3 * 3 * (60 <= 100 < 300)
        assert not counts[0][690:720].any() and not sums[0][690:720].any()


@pytest.mark.parametrize("n_rows", [0, 1, 255, 256, 257])
def test_row_counts(env, n_rows):
    """0 rows, one, and the counts around a grid of 256-thread workgroups"""
    dcn, O, records, amap, placer = env
    c = QCase(dcn, records, 86)
    if n_rows == 0:
        amap.pileup_reset()
        b, o = O.concat_reads([])
        edits, n_added = placer.pileup_batch(b, o, np.zeros(0, c.dtype), quals=np.zeros(0, np.uint8), min_base_qual=20)
        assert len(edits) == 0 and n_added == 0 and not amap.pileup_fetch(0).any() and not amap.pileup_fetch_qualities(1).any()
        return
    c.reads, c.rows, c.quals = [], [], []
    for q in range(n_rows):
        a = (37 * q) % (LEN1 - 60)
        T = records[1][a:a + 60]
        c.put(behind(T, 20 + q % 7, foreign(T, 20 + q % 7, 1 + q % 2)) if q % 3 else T, c.rng.integers(0, 42, 60 + (1 + q % 2 if q % 3 else 0)).tolist(),
              1, a, a + 60, rev=q % 2)
    c.reads.insert(0, b"ACG")
    c.quals.insert(0, b"III")
    c.rows.insert(0, VW.make_row(c.dtype, UNPLACED, 0, 0, 0, 0, 0))
    run(c, amap, placer, O)


def test_a_thousand_copies(env):
    """1,000 copies of one read at q = 93 (byte 126, FASTQ's last): count 1,000 and sum 93,000 at every position"""
    dcn, O, records, amap, placer = env
    c = QCase(dcn, records, 87)
    T = records[0][3000:3150]
    c.reads, c.quals, c.rows = [T], [bytes([126]) * 150], [VW.make_row(c.dtype, 0, 0, 0, 150, 3000, 3150)] * 1000
    counts, sums, _, _ = run(c, amap, placer, O, row_offsets=np.array([0, 1000], np.uint64))
    got_c, got_s = amap.pileup_fetch(0, 3000, 150), amap.pileup_fetch_qualities(0, 3000, 150)
    assert got_c[:, :4].sum(axis=1).tolist() == [1000] * 150 and got_s.sum(axis=1).tolist() == [93_000] * 150
    assert (got_s > 0).sum(axis=1).tolist() == [1] * 150  # (in the base's own column)


def test_trace_groups_and_a_capped_grid_in_processes_of_their_own(env):
    """DCN_ALIGN_TRACE_BYTES = 64 (trace groups of one row) against the default budget, and DCN_GRID_CUS = 1 with 300 rows (the
    capped grid of the quality kernel takes the second trip of its work loop), each in a worker that compares with the model"""
    lines = {}
    for case, extra in (("groups", dict(DCN_ALIGN_TRACE_BYTES="64")), ("groups", {}), ("grid", dict(DCN_GRID_CUS="1"))):
        env_ = {k: v for k, v in os.environ.items() if k not in ("DCN_ALIGN_TRACE_BYTES", "DCN_GRID_CUS")}
        p = subprocess.run([sys.executable, WORKER, case], capture_output=True, text=True, timeout=300, env=dict(env_, **extra))
        assert p.returncode == 0, p.stderr[-2000:]
        line = [x for x in p.stdout.splitlines() if x.startswith("quality " + case)]
        assert len(line) == 1
        lines.setdefault(case, []).append(line[0])
    assert lines["groups"][0] == lines["groups"][1] and len(lines["groups"][0]) > 1000 and len(lines["grid"][0]) > 1000

"""The model of tests/test_left_align_abi.py and tests/test_gpu_left_align*.py, and the worker of their subprocess cases.

THE DEFINITION OF A LEFT-ALIGNED PLACEMENT (include/deacon_hip.h), written as it reads.  The runs of a row come from
tests/_align_worker.py's table and walk.  left_align() unrolls them into a Python list with one op per column and follows
rules N1 - N4 literally: it finds the next gap, and while rule N2 or N3 allows a step it takes ONE column from in front of
the gap and puts it behind, comparing two bases of T (of S for an insertion) by rule 2 each time; a gap that comes to lie
behind an earlier gap of its kind is widened to hold it.  N5 merges the columns into runs again.  Nothing here is shared
with csrc/dcn_left_align.h: no stacks, no runs while a gap moves, no words of 16 bases.  The pile-up on top is
tests/_indel_worker.py's, fed with these runs.

As a program (python tests/_left_align_worker.py CASE) it runs one case in a process of its own, whose environment the
test has set, and exits non-zero with a traceback when a check fails."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import _align_worker as AW  # noqa: E402
import _indel_worker as DW  # noqa: E402
import _insertion_worker as IW  # noqa: E402
import _pileup_worker as PW  # noqa: E402
import _quality_worker as QW  # noqa: E402
import _verify_worker as VW  # noqa: E402
from _verify_worker import OVER, UNPLACED, intervals  # noqa: E402

INFO_FIELDS = ("rows_aligned", "rows_changed", "gaps_shifted", "columns_passed", "gaps_merged")
GAPS = (AW.OP_I, AW.OP_D)


def columns(runs):
    return [int(x) & 15 for x in runs for _ in range(int(x) >> 4)]


def merged(cols):
    """rule A4 / N5: equal neighbours merge into runs"""
    runs = []
    for op in cols:
        if runs and runs[-1][0] == op:
            runs[-1][1] += 1
        else:
            runs.append([op, 1])
    return [(ln << 4) | op for op, ln in runs]


def left_align(S, T, runs):
    """rules N1 - N5 -> (runs, (gaps shifted, columns passed, gaps merged))"""
    s, t = VW.encode(S, -1), VW.encode(T, -1)

    def equal(seq, a, b):  # rule 2: an invalid base equals nothing
        return seq[a] >= 0 and seq[a] == seq[b]

    cols = columns(runs)
    shifted = passed = merges = 0
    at = 0
    while True:
        p = next((c for c in range(at, len(cols)) if cols[c] in GAPS), None)
        if p is None:
            break
        op = cols[p]
        q = p
        while q < len(cols) and cols[q] == op:
            q += 1
        steps = 0
        while p > 0:  # (a gap that is first stays first)
            if cols[p - 1] == op:  # N4: directly behind an earlier gap of its kind
                while p > 0 and cols[p - 1] == op:
                    p -= 1
                merges += 1
                continue
            if cols[p - 1] in GAPS or p - 1 == 0:  # N4: the other kind; N2 / N3: the row's first column
                break
            i = sum(c != AW.OP_D for c in cols[:p])
            j = sum(c != AW.OP_I for c in cols[:p])
            ln = q - p
            if not (equal(t, j - 1, j + ln - 1) if op == AW.OP_D else equal(s, i - 1, i + ln - 1)):
                break
            cols.insert(q - 1, cols.pop(p - 1))  # the column follows the gap and keeps its op
            p, q, steps = p - 1, q - 1, steps + 1
        shifted += steps > 0
        passed += steps
        at = q
    return merged(cols), (shifted, passed, merges)


def is_alignment(S, T, runs, d):
    """the runs pair EQUAL bases in '=' and others in X, cover both intervals and cost d"""
    s, t = VW.encode(S, -1), VW.encode(T, -2)
    i = j = cost = 0
    for op in columns(runs):
        if op in (AW.OP_EQ, AW.OP_X):
            if i >= len(s) or j >= len(t) or (s[i] == t[j]) != (op == AW.OP_EQ):
                return False
        i += op != AW.OP_D
        j += op != AW.OP_I
        cost += op != AW.OP_EQ
    return (i, j, cost) == (len(s), len(t), d)


def check_properties(S, T, d, runs, new, a3=True):
    """what rules N4 - N6 promise of left_align()'s result"""
    assert is_alignment(S, T, runs, d) and is_alignment(S, T, new, d)
    assert sorted(columns(runs)) == sorted(columns(new))  # the same multiset of column ops
    AW.check_sums(new, len(S), len(T), d)  # covers m and n, n_ops <= 2 d + 1, no equal neighbours
    if runs:
        assert ((int(runs[0]) & 15) in GAPS) == ((int(new[0]) & 15) in GAPS)  # no gap became first, a first gap stayed
    if a3:
        assert not any((int(a) & 15) in GAPS and (int(b) & 15) in GAPS for a, b in zip(new, new[1:]))  # I and D never adjacent
    again, totals = left_align(S, T, new)
    assert again == new and totals == (0, 0, 0)  # idempotent
    if not any((int(x) & 15) in GAPS for x in runs):
        assert new == [int(x) for x in runs]


_PAIRS = {}  # (S, T, runs) -> (new runs, totals)


def left_align_rows(reads, records, rows, row_offsets=None, max_edits=VW.MAX_EDITS, max_permille=200):
    """the model of dcn_left_align_batch -> (edits, cigar_offsets, cigar, info dict)"""
    owner = np.arange(len(rows)) if row_offsets is None else np.repeat(np.arange(len(reads)), np.diff(np.asarray(row_offsets, np.int64)))
    edits, offs, cigar = AW.align_rows(reads, records, rows, row_offsets, max_edits, max_permille)
    info = dict.fromkeys(INFO_FIELDS, 0)
    new_offs, new_cigar = [0], []
    for r in range(len(rows)):
        if int(edits[r]) < OVER:
            S, T = intervals(reads[owner[r]], records[int(rows["record"][r])], rows[r])
            runs = tuple(int(x) for x in cigar[int(offs[r]):int(offs[r + 1])])
            if (S, T, runs) not in _PAIRS:
                _PAIRS[(S, T, runs)] = left_align(S, T, runs)
                check_properties(S, T, int(edits[r]), runs, _PAIRS[(S, T, runs)][0])
            new, (shifted, passed, merges) = _PAIRS[(S, T, runs)]
            info["rows_aligned"] += 1
            info["rows_changed"] += passed > 0
            info["gaps_shifted"] += shifted
            info["columns_passed"] += passed
            info["gaps_merged"] += merges
            new_cigar += new
        new_offs.append(len(new_cigar))
    return edits, np.array(new_offs, np.uint64), np.array(new_cigar, np.uint32), info


def add_info(total, info):
    for k in INFO_FIELDS:
        total[k] = total.get(k, 0) + info[k]
    return total


def pile_rows(counts, insertions, deletions, reads, records, rows, row_offsets=None, max_edits=VW.MAX_EDITS, max_permille=200, select=None,
              quals=None, min_base_qual=0, qual_offset=33, sums=None):
    """tests/_indel_worker.py's pile_rows with the runs of rule N5: the model of dcn_pileup_batch (with quals: of
    dcn_pileup_batch_qual; sums: tests/_quality_worker.py's quality sums, one array per record, or None) on a map whose
    switch is on -> (edits, n_added, info)"""
    rows = rows.copy()
    if select is not None:
        rows["record"][~np.asarray(select, bool)] = UNPLACED
    owner = np.arange(len(rows)) if row_offsets is None else np.repeat(np.arange(len(reads)), np.diff(np.asarray(row_offsets, np.int64)))
    edits, offs, cigar, info = left_align_rows(reads, records, rows, row_offsets, max_edits, max_permille)
    n_added = 0
    for r in range(len(rows)):
        if int(edits[r]) >= OVER:
            continue
        R = int(rows["record"][r])
        S, Tt = intervals(reads[owner[r]], records[R], rows[r])
        if len(Tt) == 0:
            continue  # rule P2
        runs = cigar[int(offs[r]):int(offs[r + 1])]
        ref_start, reverse = int(rows["ref_start"][r]), int(rows["reverse"][r])
        if quals is None:
            counted = S
        else:
            q = QW.qualities_of_S(quals[owner[r]], rows[r], qual_offset)
            counted = QW.masked(S, q, min_base_qual)
            if sums is not None:
                QW.add_sums(sums[R], S, q, ref_start, runs, min_base_qual)
        assert PW.add_runs(counts[R], counted, ref_start, reverse, runs) == (len(S), len(Tt))
        insertions[R] += IW.events_of_runs(S, ref_start, reverse, runs)
        deletions[R] += DW.deletion_events_of_runs(ref_start, reverse, runs)
        n_added += 1
    return edits, n_added, info


# ---- rows for the seams ----------------------------------------------------------------------------------------------
def seam_rows(dcn):
    """rows whose gaps take steps, in both records of tests/test_gpu_pileup_seams.py's pair and on both strands: what the
    subprocess cases run -> (records, reads, rows)"""
    from test_gpu_pileup_seams import Case, make_records
    records = make_records()
    c = Case(dcn, records, 2291)
    hp = records[0][1290:1390]  # ten bases, the homopolymer of 70, twenty bases
    for q, ln in enumerate((1, 2, 5, 17, 33)):
        c.put(hp[:40] + hp[40 + ln:], 0, 1290, 1390, rev=q % 2)          # a deletion inside the homopolymer
        c.put(hp[:40] + b"A" * ln + hp[40:], 0, 1290, 1390, rev=1 - q % 2)  # an insertion
    rng = np.random.default_rng(2292)
    for q in range(24):  # two letters: a gap almost always has a repeat in front of it
        R = q % 2
        a = 300 + 41 * q
        T = records[R][a:a + 90]
        S = VW.edit(rng, T, n_sub=q % 3, n_ins=1 + q % 2, n_del=1 + q % 3)
        c.put(S, R, a, a + 90, rev=(q // 2) % 2)
    c.unplaced()
    return records, c.reads, np.concatenate(c.rows)


def _run_seams(O, dcn, repeat=1):
    records, reads, rows = seam_rows(dcn)
    reads, rows = reads * repeat, np.concatenate([rows] * repeat)
    amap = VW.build_map(O, dcn, records)
    placer = dcn.Placer(amap, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    b, o = O.concat_reads(reads)
    got = placer.left_align_batch(b, o, rows, max_permille=1000)
    want = left_align_rows(reads, records, rows, max_permille=1000)
    AW.assert_same(got[:3], want[:3], rows)
    assert got[3] == want[3], (got[3], want[3])
    assert want[3]["rows_changed"] >= 10 * repeat
    plain = placer.align_batch(b, o, rows, max_permille=1000)
    AW.assert_same(plain, AW.align_rows(reads, records, rows, max_permille=1000), rows)  # the call beside it is what it was
    placer.close()
    amap.close()
    return got


def case_groups(O, dcn):
    """DCN_ALIGN_TRACE_BYTES as the test set it: the pass runs once, behind the last group's align kernel"""
    got = _run_seams(O, dcn)
    print("left_align groups " + "".join(np.ascontiguousarray(x).tobytes().hex() + ":" for x in got[:3]) + repr(sorted(got[3].items())).replace(" ", ""))


def case_trips(O, dcn):
    """DCN_GRID_CUS = 1 as the test set it: a few hundred rows, so that the kernel's work loop makes a second trip (one CU:
    32 workgroups of four waves = 128 rows a trip)"""
    assert os.environ.get("DCN_GRID_CUS") == "1"
    got = _run_seams(O, dcn, repeat=8)
    assert got[3]["rows_aligned"] >= 256
    print("left_align trips %d %d" % (got[3]["rows_aligned"], got[3]["rows_changed"]))


if __name__ == "__main__":
    import deacon_server_amd as dcn
    from oracle import oracle as O
    O.lib()
    {"groups": case_groups, "trips": case_trips}[sys.argv[1]](O, dcn)

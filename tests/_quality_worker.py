"""The model of tests/test_pileup_qual_abi.py and tests/test_gpu_pileup_qual*.py, and the worker of their subprocess cases.

THE DEFINITION OF A QUALITY-AWARE PILEUP (include/deacon_hip.h), restated over bytes.  The runs of a row come from aligning
the UNMASKED S (tests/_align_worker.py; rule Q6: qualities never change what aligns).  The counts are
tests/_pileup_worker.py's add_runs over a copy of S in which every base with q < min_base_qual has become N (rule Q3); the
sums are a second loop over the same runs, one step at a time (rule Q4); the events are tests/_insertion_worker.py's, from
the unmasked S (rule Q5).  Nothing here is shared with csrc/dcn_pileup.h: no lanes, no planes, no prefix sums.

As a program (python tests/_quality_worker.py CASE) it runs one case in a process of its own, whose environment the test
has set, and exits non-zero with a traceback when a check fails."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import _align_worker as AW  # noqa: E402
import _insertion_worker as IW  # noqa: E402
import _pileup_worker as PW  # noqa: E402
import _verify_worker as VW  # noqa: E402
from _verify_worker import OVER, UNPLACED, intervals  # noqa: E402


def quality(byte, qual_offset=33):
    """rule Q2"""
    return byte - qual_offset if byte >= qual_offset else 0


def qualities_of_S(read_quals, row, qual_offset=33):
    """rule Q2: q(S[i]) for every i.  S[i] of a reverse row is the complement of the read's base read_end - 1 - i, and its
    quality is that base's"""
    q = [quality(b, qual_offset) for b in bytes(read_quals)[int(row["read_start"]):int(row["read_end"])]]
    return q[::-1] if int(row["reverse"]) else q


def masked(S, q, min_base_qual):
    """rule Q3 as a string: every base of S below the threshold becomes N (an invalid base is N either way)"""
    assert len(S) == len(q)
    return bytes(ord("N") if x < min_base_qual else b for b, x in zip(S, q))


def add_sums(sums, S, q, ref_start, runs, min_base_qual):
    """rule Q4: one row's runs, step by step, into sums[len(record), 4]"""
    i = j = 0
    for x in runs:
        ln, op = int(x) >> 4, int(x) & 15
        if op == AW.OP_I:
            i += ln
        elif op == AW.OP_D:
            j += ln
        else:
            for _ in range(ln):
                col = PW.column(S[i])
                if col <= PW.T and q[i] >= min_base_qual:
                    sums[ref_start + j, col] += q[i]
                i += 1
                j += 1
    return i, j


def new_sums(records):
    return [np.zeros((len(r), 4), np.int64) for r in records]


def pile_pair(S, T, q, min_base_qual, reverse=0, ref_start=0):
    """one pair alone, q parallel to S -> (counts, sums, events, the runs as text), or None without an alignment"""
    d, runs = AW.align_pair(S, T)
    if d > VW.threshold(len(S), len(T)) or len(T) == 0:
        return None
    counts, sums = np.zeros((ref_start + len(T), PW.COLUMNS), np.int64), np.zeros((ref_start + len(T), 4), np.int64)
    assert PW.add_runs(counts, masked(S, q, min_base_qual), ref_start, reverse, runs) == (len(S), len(T))
    assert add_sums(sums, S, q, ref_start, runs, min_base_qual) == (len(S), len(T))
    return counts, sums, IW.events_of_runs(S, ref_start, reverse, runs), AW.cigar_text(runs)


def pile_rows(counts, sums, ledger, reads, quals, records, rows, row_offsets=None, min_base_qual=0, qual_offset=33,
              max_edits=VW.MAX_EDITS, max_permille=200, select=None):
    """the model of dcn_pileup_batch_qual: adds to counts, sums and ledger (one entry per record; sums or ledger None: not
    kept) -> (edits, n_added).  quals: one bytes per read, parallel to reads"""
    rows = rows.copy()
    if select is not None:
        rows["record"][~np.asarray(select, bool)] = UNPLACED
    owner = np.arange(len(rows)) if row_offsets is None else np.repeat(np.arange(len(reads)), np.diff(np.asarray(row_offsets, np.int64)))
    edits, offs, cigar = AW.align_rows(reads, records, rows, row_offsets, max_edits, max_permille)  # (the unmasked S)
    n_added = 0
    for r in range(len(rows)):
        if int(edits[r]) >= OVER:
            continue
        R = int(rows["record"][r])
        S, Tt = intervals(reads[owner[r]], records[R], rows[r])
        if len(Tt) == 0:
            continue
        q = qualities_of_S(quals[owner[r]], rows[r], qual_offset)
        runs = cigar[int(offs[r]):int(offs[r + 1])]
        a, rev = int(rows["ref_start"][r]), int(rows["reverse"][r])
        assert PW.add_runs(counts[R], masked(S, q, min_base_qual), a, rev, runs) == (len(S), len(Tt))
        if sums is not None:
            assert add_sums(sums[R], S, q, a, runs, min_base_qual) == (len(S), len(Tt))
        if ledger is not None:
            ledger[R] += IW.events_of_runs(S, a, rev, runs)
        n_added += 1
    return edits, n_added


def assert_sums(amap, records, sums):
    """the quality sums of a map against the model, with the first position that differs named"""
    for R, rec in enumerate(records):
        got, want = amap.pileup_fetch_qualities(R), PW.as_u32(sums[R])
        assert got.shape == want.shape == (len(rec), 4) and got.dtype == np.uint32
        if not np.array_equal(got, want):
            p = int(np.argwhere((got != want).any(axis=1))[0][0])
            raise AssertionError(("sums of record", R, "position", p, "got", got[p].tolist(), "want", want[p].tolist()))


def random_quals(rng, reads, lo=0, hi=41, qual_offset=33):
    """one quality string per read, uniform in lo .. hi"""
    return [(rng.integers(lo, hi + 1, len(r)) + qual_offset).astype(np.uint8).tobytes() for r in reads]


def variant_quals(c, s, ref_byte, call):
    """`deacon-hip call`'s ref_qual and alt_qual of a SUB line: the integer quotient of the sum and the count of the
    reference's column and of the called one; "." for a count of 0 or an invalid reference base"""
    def mean(col):
        return "." if col > PW.T or int(c[col]) == 0 else str(int(s[col]) // int(c[col]))
    return mean(PW.column(ref_byte)), mean(PW.column(ord(call)))


def concat(O, reads, quals):
    b, o = O.concat_reads(reads)
    return b, o, np.frombuffer(b"".join(quals), np.uint8)


# ---- the subprocess cases --------------------------------------------------------------------------------------------
def _run(O, dcn, records, reads, quals, rows, min_base_qual, batches=1):
    amap = VW.build_map(O, dcn, records)
    amap.pileup_enable()
    amap.pileup_keep_insertions()
    amap.pileup_keep_qualities()
    placer = dcn.Placer(amap, max_batch_bases=1 << 18, max_batch_reads=1 << 10)
    rows = IW.rows_as(dcn.filter.PLACEMENT_DTYPE, rows)
    counts, sums, ledger = PW.new_counts(records), new_sums(records), IW.new_ledger(records)
    cuts = np.linspace(0, len(reads), batches + 1).astype(int)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        b, o, q = concat(O, reads[lo:hi], quals[lo:hi])
        edits, n_added = placer.pileup_batch(b, o, rows[lo:hi], quals=q, min_base_qual=min_base_qual)
        want = pile_rows(counts, sums, ledger, reads[lo:hi], quals[lo:hi], records, rows[lo:hi], min_base_qual=min_base_qual)
        assert edits.tolist() == want[0].tolist() and n_added == want[1]
    PW.assert_counts(amap, records, counts)
    assert_sums(amap, records, sums)
    IW.assert_ledger(amap, records, counts, ledger, fills=(False,))
    text = "".join(np.ascontiguousarray(amap.pileup_fetch(R)).tobytes().hex() + ":" + np.ascontiguousarray(amap.pileup_fetch_qualities(R)).tobytes().hex() + ":"
                   for R in range(len(records)))
    placer.close()
    amap.close()
    return text


def case_groups(O, dcn):
    """DCN_ALIGN_TRACE_BYTES as the test set it: several trace groups per call, the same counters and sums"""
    records, reads, rows = IW.random_rows(5, 60)
    quals = random_quals(np.random.default_rng(50), reads)
    print("quality groups " + _run(O, dcn, records, reads, quals, rows, 20))


def case_grid(O, dcn):
    """DCN_GRID_CUS = 1 with 300 rows: the capped grid of the quality kernel takes the second trip of its work loop"""
    assert os.environ.get("DCN_GRID_CUS") == "1"
    records, reads, rows = IW.random_rows(6, 300)
    assert int((AW.align_rows(reads, records, rows)[0] < OVER).sum()) > 128  # (one trip of that grid: 32 workgroups of four waves)
    quals = random_quals(np.random.default_rng(60), reads)
    print("quality grid " + _run(O, dcn, records, reads, quals, rows, 20))


if __name__ == "__main__":
    import deacon_server_amd as dcn
    from oracle import oracle as O
    O.lib()
    {"groups": case_groups, "grid": case_grid}[sys.argv[1]](O, dcn)

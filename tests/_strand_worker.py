"""The model of tests/test_strand_abi.py and tests/test_gpu_strand*.py, and the worker of their subprocess case.

THE DEFINITION OF STRAND EVIDENCE (include/deacon_hip.h), written as it reads.  The runs of a row come from
tests/_align_worker.py's table and walk (left-aligned by tests/_left_align_worker.py where the map's switch is on);
add_planes() follows them one step at a time by rule S2 into a numpy array of four reverse counters per base of the record,
over the same masked copy of S that tests/_quality_worker.py counts (rule Q3).  base_table() and indel_table() are rules S3
and S4, score() rule S5 in Python's unbounded integers, flags() rule S6, count_reverse() the a_rev of rule S4 as a loop over
the ledgers' tuples.  Nothing here is shared with csrc/dcn_strand.h or csrc/dcn_pileup.h: no lanes, no planes, no shift by a
loop, no 64-bit bound.

As a program (python tests/_strand_worker.py CASE) it runs one case in a process of its own, whose environment the test has
set, and exits non-zero with a traceback when a check fails."""
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
import _left_align_worker as LW  # noqa: E402
import _pileup_worker as PW  # noqa: E402
import _quality_worker as QW  # noqa: E402
import _verify_worker as VW  # noqa: E402
from _verify_worker import OVER, intervals  # noqa: E402

STRAND_BIAS, STRAND_ONE_SIDED = 1, 2
DEFAULTS = dict(max_sb_centi=1083, min_alt_strand=1, min_strand_depth=3)
SB_CAP = 65535


# ---- rule S2 ---------------------------------------------------------------------------------------------------------
def add_planes(planes, S, ref_start, reverse, runs):
    """one row's runs, step by step, into planes[len(record), 4]; S is the copy in which a base that counts as N is N"""
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
                if reverse and col <= PW.T:
                    planes[ref_start + j, col] += 1
                i += 1
                j += 1
    return i, j


def new_planes(records):
    return [np.zeros((len(r), 4), np.int64) for r in records]


def pile_planes(planes, reads, records, rows, row_offsets=None, max_edits=VW.MAX_EDITS, max_permille=200, quals=None, min_base_qual=0,
                qual_offset=33, left_align=False):
    """the planes' side of dcn_pileup_batch / _batch_qual on a map that keeps them (the other models add the counters, the
    sums and the ledgers of the same rows) -> n_added"""
    owner = np.arange(len(rows)) if row_offsets is None else np.repeat(np.arange(len(reads)), np.diff(np.asarray(row_offsets, np.int64)))
    edits, offs, cigar = AW.align_rows(reads, records, rows, row_offsets, max_edits, max_permille)
    n_added = 0
    for r in range(len(rows)):
        if int(edits[r]) >= OVER:
            continue
        R = int(rows["record"][r])
        S, Tt = intervals(reads[owner[r]], records[R], rows[r])
        if len(Tt) == 0:
            continue
        runs = cigar[int(offs[r]):int(offs[r + 1])]
        if left_align:
            runs = LW.left_align(S, Tt, runs)[0]
        counted = S if quals is None else QW.masked(S, QW.qualities_of_S(quals[owner[r]], rows[r], qual_offset), min_base_qual)
        assert add_planes(planes[R], counted, int(rows["ref_start"][r]), int(rows["reverse"][r]), runs) == (len(S), len(Tt))
        n_added += 1
    return n_added


def assert_planes(amap, records, planes, counts=None):
    """the strand planes of a map against the model, with the first position that differs named; with the counters given,
    rule S2's two inequalities as well"""
    for R, rec in enumerate(records):
        got, want = amap.pileup_fetch_strands(R), PW.as_u32(planes[R])
        assert got.shape == want.shape == (len(rec), 4) and got.dtype == np.uint32
        if not np.array_equal(got, want):
            p = int(np.argwhere((got != want).any(axis=1))[0][0])
            raise AssertionError(("planes of record", R, "position", p, "got", got[p].tolist(), "want", want[p].tolist()))
        if counts is not None:
            c = np.asarray(counts[R])
            assert (planes[R] <= c[:, :4]).all() and (planes[R].sum(axis=1) <= c[:, PW.REV]).all()


# ---- rules S3 - S6 ---------------------------------------------------------------------------------------------------
def base_table(n, r, ref, alt_mask):
    """rule S3: n and r are the four counters and the four reverse counters of the position"""
    f = [int(n[c]) - int(r[c]) for c in range(4)]
    assert min(f) >= 0 and 0 <= ref <= 3 and 0 < alt_mask < 16 and not alt_mask & (1 << ref)
    alt = [c for c in range(4) if alt_mask & (1 << c)]
    return f[ref], int(r[ref]), sum(f[c] for c in alt), sum(int(r[c]) for c in alt)


def indel_table(depth, rev, a_all, a_rev):
    """rule S4"""
    d = a_rev
    c = a_all - a_rev
    b = rev - d if rev >= d else 0
    fwd = depth - rev if depth >= rev else 0
    a = fwd - c if fwd >= c else 0
    return a, b, c, d


def score(table):
    """rule S5"""
    m = max(table)
    s = 0 if m < 1024 else m.bit_length() - 10
    a, b, c, d = (x >> s for x in table)
    n, r1, r2, c1, c2 = a + b + c + d, a + b, c + d, a + c, b + d
    if r1 * r2 * c1 * c2 == 0:
        return 0
    return min(SB_CAP, 100 * n * (a * d - b * c) ** 2 // (r1 * r2 * c1 * c2))


def flags(table, sb_centi, max_sb_centi=1083, min_alt_strand=1, min_strand_depth=3):
    """rule S6"""
    a, b, c, d = table
    out = 0
    if max_sb_centi > 0 and sb_centi >= max_sb_centi:
        out |= STRAND_BIAS
    if min(c, d) < min_alt_strand and a + c >= min_strand_depth and b + d >= min_strand_depth:
        out |= STRAND_ONE_SIDED
    return out


def evidence(counts, planes, query, **params):
    """one query (pos, kind, ref_code, alt_mask, count, count_reverse) over a record's counts[len, 8] and planes[len, 4] ->
    (fwd, rev, table, sb_centi, flags), as AnchorMap.strand_evidence's site"""
    pos, kind, ref, alt_mask, count, count_reverse = (int(x) for x in query)
    c = [int(x) for x in counts[pos]]
    if kind == 0:
        r = [int(x) for x in planes[pos]]
        table = base_table(c[:4], r, ref, alt_mask)
        fwd, rev = [c[x] - r[x] for x in range(4)], r
    else:
        table = indel_table(sum(c[:6]), c[PW.REV], count, count_reverse)
        fwd, rev = [0] * 4, [0] * 4
    sb = score(table)
    return fwd, rev, list(table), sb, flags(table, sb, **dict(DEFAULTS, **params))


def device_evidence(sites):
    """AnchorMap.strand_evidence's array as the model's tuples; the reserved words are 0"""
    assert not sites["reserved"].any()
    return [([int(x) for x in s["fwd"]], [int(x) for x in s["rev"]], [int(x) for x in s["table"]], int(s["sb_centi"]), int(s["flags"])) for s in sites]


def assert_evidence(amap, R, counts, planes, queries, **params):
    """AnchorMap.strand_evidence against the model, the first difference named -> the model's sites"""
    want = [evidence(counts, planes, q, **params) for q in queries]
    import deacon_server_amd as dcn
    arr = np.zeros(len(queries), dcn.STRAND_QUERY_DTYPE)
    for k, q in enumerate(queries):
        arr[k] = tuple(int(x) for x in q) + (0,)
    got = device_evidence(amap.strand_evidence(R, arr, **dict(DEFAULTS, **params)))
    if got != want:
        k = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
        raise AssertionError(("query", k, tuple(int(x) for x in queries[k]), "got", got[k:k + 1], "want", want[k:k + 1], params))
    return want


def genotype_queries(sites, ploidy=2):
    """the base queries of the model's genotype sites (tests/_genotype_worker.py: dicts with pos, gt, ref_code), by rule G3's
    order written out"""
    pairs = [(0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2), (0, 3), (1, 3), (2, 3), (3, 3)]
    out = []
    for pos, gt, ref in sites:
        alleles = set(pairs[gt]) if ploidy == 2 else {gt}
        mask = sum(1 << x for x in alleles if x != ref)
        out.append((pos, 0, ref, mask, 0, 0))
    return out


# ---- a_rev of rule S4 ------------------------------------------------------------------------------------------------
def count_reverse(insertions, deletions, site):
    """site = the model's (pos, flags, len, bases, ...) of tests/_indel_worker.py; insertions / deletions the record's events"""
    p, fl, ln, bases = site[:4]
    if fl & DW.INDEL_DELETION:
        return sum(1 for e in deletions if e == (p, ln, 1))
    front = 1 if fl & DW.INDEL_FRONT else 0
    return sum(1 for e in insertions if (e[0], 1 if e[1] else 0, e[2], e[3], e[4]) == (p, front, ln, bases, 1))


# ---- the rows of the host program (tests/cpp/strand_rule_test.cpp prints them; tests/test_strand_abi.py compares) ------
def check_rule_rows(lines):
    """lines "T a b c d max_sb min_alt min_depth -> sb flags" -> how many rows were checked against score() and flags()"""
    n = 0
    for line in lines:
        if not line.startswith("T "):
            continue
        left, right = line[2:].split("->")
        a, b, c, d, max_sb, min_alt, min_depth = (int(x) for x in left.split())
        sb, fl = (int(x) for x in right.split())
        want_sb = score((a, b, c, d))
        assert (sb, fl) == (want_sb, flags((a, b, c, d), want_sb, max_sb, min_alt, min_depth)), line
        n += 1
    return n


# ---- the subprocess case ---------------------------------------------------------------------------------------------
def case_grid(O, dcn):
    """DCN_GRID_CUS = 1 with 300 rows: the capped grid of both strand forms of the pileup kernel takes the second trip of its
    work loop (tests/_grid_trip_cases.py reaches the other kernels' the same way)"""
    assert os.environ.get("DCN_GRID_CUS") == "1"
    records, reads, rows = IW.random_rows(7, 300)
    assert int((AW.align_rows(reads, records, rows)[0] < OVER).sum()) > 128  # (one trip of that grid: 32 workgroups of four waves)
    quals = QW.random_quals(np.random.default_rng(70), reads)
    rows = IW.rows_as(dcn.filter.PLACEMENT_DTYPE, rows)
    text = ""
    for with_quals in (False, True):
        amap = VW.build_map(O, dcn, records)
        amap.pileup_enable()
        amap.pileup_keep_strands()
        placer = dcn.Placer(amap, max_batch_bases=1 << 18, max_batch_reads=1 << 10)
        counts, planes = PW.new_counts(records), new_planes(records)
        if with_quals:
            b, o, q = QW.concat(O, reads, quals)
            edits, n_added = placer.pileup_batch(b, o, rows, quals=q, min_base_qual=20)
            want = QW.pile_rows(counts, None, None, reads, quals, records, rows, min_base_qual=20)
            assert pile_planes(planes, reads, records, rows, quals=quals, min_base_qual=20) == want[1]
        else:
            b, o = O.concat_reads(reads)
            edits, n_added = placer.pileup_batch(b, o, rows)
            want = PW.pile_rows(counts, reads, records, rows)
            assert pile_planes(planes, reads, records, rows) == want[1]
        assert edits.tolist() == want[0].tolist() and n_added == want[1] > 128
        PW.assert_counts(amap, records, counts)
        assert_planes(amap, records, planes, counts)
        assert sum(int(p.sum()) for p in planes) > 1000
        text += "".join(np.ascontiguousarray(amap.pileup_fetch_strands(R)).tobytes().hex() + ":" for R in range(len(records)))
        placer.close()
        amap.close()
    print("strand grid " + text)


if __name__ == "__main__":
    import deacon_server_amd as dcn
    from oracle import oracle as O
    O.lib()
    {"grid": case_grid}[sys.argv[1]](O, dcn)

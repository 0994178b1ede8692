"""The model of tests/test_align_abi.py and tests/test_gpu_align*.py, and the worker of their subprocess cases.

THE DEFINITION OF AN ALIGNED PLACEMENT (include/deacon_hip.h), restated over bytes.  D[i][j] is the Levenshtein distance
of S[:i] and T[:j] under rule 2's equality (tests/_verify_worker.py's encode: an invalid base equals nothing); table()
builds all (m + 1) x (n + 1) cells row by row.  walk() goes from (m, n) to (0, 0) cell by cell and takes, at a cell of
cost s, the first of X (D[i-1][j-1] == s - 1), I (D[i-1][j] == s - 1), D (D[i][j-1] == s - 1), else '='; the steps
reversed, equal neighbours merged, are the runs, len << 4 | op with BAM's codes.  There is no wavefront here and no
furthest-reaching point: the model shares nothing with the kernel.

As a program (python tests/_align_worker.py CASE) it runs one case in a process of its own, whose environment the test
has set, and exits non-zero with a traceback when a check fails."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import _verify_worker as VW  # noqa: E402
from _verify_worker import OVER, UNPLACED, encode, intervals, threshold  # noqa: E402
from conftest import random_reads, revcomp  # noqa: E402

OP_I, OP_D, OP_EQ, OP_X = 1, 2, 7, 8
LETTER = {OP_I: "I", OP_D: "D", OP_EQ: "=", OP_X: "X"}
CODE = {v: k for k, v in LETTER.items()}


def table(S, T):
    """int32[(m + 1, n + 1)]: rule A2's D, row i from row i - 1"""
    s, t = encode(S, -1), encode(T, -2)
    m, n = len(s), len(t)
    idx = np.arange(n + 1, dtype=np.int32)
    D = np.empty((m + 1, n + 1), np.int32)
    D[0] = idx
    for i in range(m):
        x = np.empty(n + 1, np.int32)
        x[0] = i + 1
        x[1:] = np.minimum(D[i, :-1] + (t != s[i]), D[i, 1:] + 1)  # substitution / match, a base of S alone
        D[i + 1] = np.minimum.accumulate(x - idx) + idx            # a base of T alone
    return D


def walk(D):
    """rule A3 over the table -> the runs of rule A4, from the start of both intervals"""
    i, j = D.shape[0] - 1, D.shape[1] - 1
    steps = []
    while i > 0 or j > 0:
        s = int(D[i, j])
        if i > 0 and j > 0 and D[i - 1, j - 1] == s - 1:
            steps.append(OP_X)
            i, j = i - 1, j - 1
        elif i > 0 and D[i - 1, j] == s - 1:
            steps.append(OP_I)
            i -= 1
        elif j > 0 and D[i, j - 1] == s - 1:
            steps.append(OP_D)
            j -= 1
        else:
            assert i > 0 and j > 0 and D[i - 1, j - 1] == s
            steps.append(OP_EQ)
            i, j = i - 1, j - 1
    runs = []
    for op in reversed(steps):
        if runs and runs[-1][0] == op:
            runs[-1][1] += 1
        else:
            runs.append([op, 1])
    return [(ln << 4) | op for op, ln in runs]


def align_pair(S, T):
    """(d, runs) of two byte strings"""
    D = table(S, T)
    return int(D[-1, -1]), walk(D)


def cigar_text(runs):
    return "".join("%d%s" % (int(x) >> 4, LETTER[int(x) & 15]) for x in runs)


def parse_cigar(text):
    """"3=1X" -> runs"""
    runs, num = [], ""
    for ch in text:
        if ch.isdigit():
            num += ch
        else:
            runs.append((int(num) << 4) | CODE[ch])
            num = ""
    assert num == ""
    return runs


def check_sums(runs, m, n, d):
    """what rule A4 says of a row's runs"""
    tot = {OP_I: 0, OP_D: 0, OP_EQ: 0, OP_X: 0}
    for x in runs:
        assert (int(x) >> 4) > 0
        tot[int(x) & 15] += int(x) >> 4
    assert tot[OP_X] + tot[OP_I] + tot[OP_D] == d, (tot, d)
    assert tot[OP_EQ] + tot[OP_X] + tot[OP_I] == m and tot[OP_EQ] + tot[OP_X] + tot[OP_D] == n, (tot, m, n)
    assert len(runs) <= 2 * d + 1 and all((int(a) & 15) != (int(b) & 15) for a, b in zip(runs, runs[1:]))
    return tot


_PAIRS = {}  # (S, T) -> (d, runs): the tests ask for the same pair through several placement calls


def align_rows(reads, records, rows, row_offsets=None, max_edits=VW.MAX_EDITS, max_permille=200):
    """the model of dcn_align_batch -> (edits np.uint32[n_rows], cigar_offsets np.uint64[n_rows + 1], cigar np.uint32[]).
    The distance of every row comes from tests/_verify_worker.py's programme; the table is built for the rows within
    their threshold only, and its last cell must agree."""
    owner = np.arange(len(rows)) if row_offsets is None else np.repeat(np.arange(len(reads)), np.diff(np.asarray(row_offsets, np.int64)))
    assert len(owner) == len(rows)
    edits = VW.verify_rows(reads, records, rows, row_offsets, max_edits, max_permille)
    offs, cigar = [0], []
    for i in range(len(rows)):
        if int(edits[i]) < OVER:
            S, T = intervals(reads[owner[i]], records[int(rows["record"][i])], rows[i])
            if (S, T) not in _PAIRS:
                _PAIRS[(S, T)] = align_pair(S, T)
            d, runs = _PAIRS[(S, T)]
            assert d == int(edits[i])
            check_sums(runs, len(S), len(T), d)
            cigar += runs
        offs.append(len(cigar))
    return edits, np.array(offs, np.uint64), np.array(cigar, np.uint32)


def assert_same(got, want, rows=None):
    """(edits, cigar_offsets, cigar) twice: equal, with the first row that differs named"""
    ge, go, gc = got
    we, wo, wc = want
    for i in range(len(we)):
        g, w = gc[int(go[i]):int(go[i + 1])] if i + 1 < len(go) else None, wc[int(wo[i]):int(wo[i + 1])]
        assert int(ge[i]) == int(we[i]) and g is not None and list(g) == list(w), \
            (i, int(ge[i]), int(we[i]), cigar_text(g) if g is not None else None, cigar_text(w), None if rows is None else rows[i])
    assert np.asarray(ge).tolist() == we.tolist() and np.asarray(go).tolist() == wo.tolist() and np.asarray(gc).tolist() == wc.tolist()


# ---- subprocess cases ----------------------------------------------------------------------------------------------
def groups_batch(dcn):
    """the batch of the groups cases: rows of d = 0 .. 40 in no order, both strands, an OVER and an UNPLACED row between"""
    rng = np.random.default_rng(1421)
    records = [random_reads(rng, 1, 2500, 2500)[0], random_reads(rng, 1, 1203, 1203)[0]]
    D = dcn.filter.PLACEMENT_DTYPE
    reads, rows = [], []
    for q, d in enumerate([3, 0, 17, 40, 1, 0, 33, 8, 2, 25, 40, 5]):
        R, rev = q % 2, (q // 2) % 2
        a = 100 + 37 * q
        T = records[R][a:a + 400]
        S = VW.mutate_mixed(rng, T, d / 400.0) if q % 3 else spaced(T, d)
        reads.append(b"ACGTTGCA"[:q % 8] + (revcomp(S) if rev else S))
        rows.append(VW.make_row(D, R, rev, q % 8, q % 8 + len(S), a, a + 400))
        if q == 4:
            reads.append(random_reads(rng, 1, 400, 400)[0])
            rows.append(VW.make_row(D, 0, 0, 0, 400, 0, 400))  # unrelated: OVER
        if q == 7:
            reads.append(b"ACGT")
            rows.append(VW.make_row(D, UNPLACED, 0, 0, 0, 0, 0))
    return records, reads, np.concatenate(rows)


def spaced(T, count):
    s = bytearray(T)
    for i in range(count):
        at = (2 * i + 1) * len(T) // (2 * count)
        s[at] = ord("A") if s[at] != ord("A") else ord("C")
    return bytes(s)


def case_groups(O, dcn):
    """DCN_ALIGN_TRACE_BYTES as the test set it: the batch's results, printed as one line of hex for the test to compare
    with the default budget's, and checked against the model here"""
    records, reads, rows = groups_batch(dcn)
    amap = VW.build_map(O, dcn, records)
    placer = dcn.Placer(amap, max_batch_bases=1 << 16, max_batch_reads=1 << 10)
    b, o = O.concat_reads(reads)
    got = placer.align_batch(b, o, rows)
    assert_same(got, align_rows(reads, records, rows), rows)
    again = placer.align_batch(b, o, rows)  # (the buffers of the first call serve the second)
    assert all(np.array_equal(x, y) for x, y in zip(got, again))
    placer.close()
    amap.close()
    print("align groups " + "".join(np.ascontiguousarray(x).tobytes().hex() + ":" for x in got))


if __name__ == "__main__":
    import deacon_server_amd as dcn
    from oracle import oracle as O
    O.lib()
    {"groups": case_groups}[sys.argv[1]](O, dcn)

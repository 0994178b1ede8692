"""The model of tests/test_pileup_abi.py and tests/test_gpu_pileup*.py, and the worker of their subprocess case.

THE DEFINITION OF A PILEUP (include/deacon_hip.h), restated over bytes.  The runs of a row come from
tests/_align_worker.py's table and walk (rule A3: no wavefront); add_runs() follows them one step at a time by rule P3 into
a numpy array of one row of eight counters per base of the record; call_position() is rule P6 in Python integers.  Nothing
here is shared with csrc/dcn_pileup.h: no prefix sum over runs, no lanes, no planes.

As a program (python tests/_pileup_worker.py CASE) it runs one case in a process of its own, whose environment the test
has set, and exits non-zero with a traceback when a check fails."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import _align_worker as AW  # noqa: E402
import _verify_worker as VW  # noqa: E402
from _verify_worker import OVER, UNPLACED, intervals  # noqa: E402
from conftest import random_reads, revcomp  # noqa: E402

A, C, G, T, N, DEL, INS, REV = range(8)
COLUMNS = 8
SITE_SUB, SITE_DEL, SITE_INS, NO_CODE = 1, 2, 4, 7
_COLUMN = {ord("A"): A, ord("C"): C, ord("G"): G, ord("T"): T, ord("a"): A, ord("c"): C, ord("g"): G, ord("t"): T}


def column(byte):
    return _COLUMN.get(byte, N)


def add_runs(counts, S, ref_start, reverse, runs):
    """rule P3: one row's runs, step by step, into counts[len(record), 8]"""
    i = j = 0
    for x in runs:
        ln, op = int(x) >> 4, int(x) & 15
        if op == AW.OP_I:
            counts[ref_start + (j - 1 if j > 0 else 0), INS] += 1  # the run, whatever its length
            i += ln
            continue
        for _ in range(ln):
            p = ref_start + j
            if op == AW.OP_D:
                counts[p, DEL] += 1
            else:
                counts[p, column(S[i])] += 1
                i += 1
            if reverse:
                counts[p, REV] += 1
            j += 1
    return i, j


def pile_pair(S, T, reverse=0, ref_start=0, ref_len=None):
    """one pair alone: counts over a record of ref_len bases (default: T's), or None when the pair has no alignment under
    the default threshold"""
    d, runs = AW.align_pair(S, T)
    counts = np.zeros((len(T) if ref_len is None else ref_len, COLUMNS), np.int64)
    if d > VW.threshold(len(S), len(T)) or len(T) == 0:
        return None
    assert add_runs(counts, S, ref_start, reverse, runs) == (len(S), len(T))
    return counts


def new_counts(records):
    return [np.zeros((len(r), COLUMNS), np.int64) for r in records]


def pile_rows(counts, reads, records, rows, row_offsets=None, max_edits=VW.MAX_EDITS, max_permille=200, select=None):
    """the model of dcn_pileup_batch: adds to counts (one array per record) -> (edits, n_added).  select: a boolean per row;
    a row it leaves out is unplaced, as Placer.pileup_batch gives it"""
    rows = rows.copy()
    if select is not None:
        rows["record"][~np.asarray(select, bool)] = UNPLACED
    owner = np.arange(len(rows)) if row_offsets is None else np.repeat(np.arange(len(reads)), np.diff(np.asarray(row_offsets, np.int64)))
    edits, offs, cigar = AW.align_rows(reads, records, rows, row_offsets, max_edits, max_permille)
    n_added = 0
    for r in range(len(rows)):
        if int(edits[r]) >= OVER:
            continue
        S, Tt = intervals(reads[owner[r]], records[int(rows["record"][r])], rows[r])
        if len(Tt) == 0:
            continue  # rule P2: n = 0 adds nothing
        runs = cigar[int(offs[r]):int(offs[r + 1])]
        assert add_runs(counts[int(rows["record"][r])], S, int(rows["ref_start"][r]), int(rows["reverse"][r]), runs) == (len(S), len(Tt))
        n_added += 1
    return edits, n_added


def as_u32(counts):
    """what the device holds: the counters wrap at 2^32 (never reached here)"""
    return (np.asarray(counts) & 0xFFFFFFFF).astype(np.uint32)


def call_position(c, ref_byte, min_depth=3, min_permille=500):
    """rule P6 at one position: c = its eight counters -> (call character, site_info)"""
    c = [int(x) for x in c]
    depth = sum(c[A:DEL + 1])
    best = A
    for col in (C, G, T, DEL):
        if c[col] > c[best]:
            best = col
    deep = depth > 0 and depth >= min_depth
    called = deep and c[best] * 1000 >= depth * min_permille
    call_code = NO_CODE if not called else (4 if best == DEL else best)
    ref_col = column(ref_byte)
    ref_code = ref_col if ref_col != N else NO_CODE
    flags = 0
    if called and best != DEL and best != ref_code:
        flags |= SITE_SUB
    if called and best == DEL:
        flags |= SITE_DEL
    if deep and c[INS] * 1000 >= depth * min_permille:
        flags |= SITE_INS
    return "ACGT-"[call_code] if called else "N", flags | call_code << 8 | ref_code << 16


def call_range(counts, record, start=0, n=None, min_depth=3, min_permille=500):
    """the model of dcn_anchor_map_pileup_call -> (calls bytes, site_pos np.uint64[], site_info np.uint32[])"""
    n = len(record) - start if n is None else n
    calls, pos, info = [], [], []
    for p in range(start, start + n):
        ch, x = call_position(counts[p], bytes(record)[p], min_depth, min_permille)
        calls.append(ch)
        if x & 0xFF:
            pos.append(p)
            info.append(x)
    return "".join(calls).encode(), np.array(pos, np.uint64), np.array(info, np.uint32)


def assert_counts(amap, records, counts):
    """the whole pileup of a map against the model, with the first position that differs named"""
    for R, rec in enumerate(records):
        got, want = amap.pileup_fetch(R), as_u32(counts[R])
        assert got.shape == want.shape == (len(rec), COLUMNS) and got.dtype == np.uint32
        if not np.array_equal(got, want):
            p = int(np.argwhere((got != want).any(axis=1))[0][0])
            raise AssertionError(("record", R, "position", p, "got", got[p].tolist(), "want", want[p].tolist()))


def assert_calls(amap, records, counts, R, start=0, n=None, **kw):
    got = amap.pileup_call(R, start, n, **kw)
    want = call_range(counts[R], records[R], start, n, **kw)
    assert got[0] == want[0], ("calls", R, start, n)
    assert got[1].tolist() == want[1].tolist() and got[2].tolist() == want[2].tolist(), ("sites", R, start, n, got[1:], want[1:])
    return want


# ---- the subprocess case --------------------------------------------------------------------------------------------
def case_groups(O, dcn):
    """DCN_ALIGN_TRACE_BYTES as the test set it: the pileup of tests/_align_worker.py's groups batch, checked against the
    model here and printed as one line of hex for the test to compare with the default budget's"""
    records, reads, rows = AW.groups_batch(dcn)
    amap = VW.build_map(O, dcn, records)
    amap.pileup_enable()
    placer = dcn.Placer(amap, max_batch_bases=1 << 16, max_batch_reads=1 << 10)
    b, o = O.concat_reads(reads)
    edits, n_added = placer.pileup_batch(b, o, rows)
    counts = new_counts(records)
    want_edits, want_added = pile_rows(counts, reads, records, rows)
    assert edits.tolist() == want_edits.tolist() and n_added == want_added
    assert_counts(amap, records, counts)
    text = "".join(np.ascontiguousarray(amap.pileup_fetch(R)).tobytes().hex() + ":" for R in range(len(records)))
    placer.close()
    amap.close()
    print("pileup groups %d " % n_added + text)


if __name__ == "__main__":
    import deacon_server_amd as dcn
    from oracle import oracle as O
    O.lib()
    {"groups": case_groups}[sys.argv[1]](O, dcn)

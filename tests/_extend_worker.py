"""The model of tests/test_extend_abi.py and tests/test_gpu_extend*.py.

THE DEFINITION OF AN EXTENDED PLACEMENT (include/deacon_hip.h), restated over bytes.  X1: R' is the read, or its reverse
complement when the row says reverse; (a, b) is the read interval on R'.  X2: the right flank is U = R'[b:], V =
record[ref_end:]; the left flank is U = R'[:a] and V = record[:ref_start], both read backwards.  X3: D is the full table
of Levenshtein distances of the prefixes of U and V, one row per base of U by the plain dynamic programme of
tests/_verify_worker.py (no wavefront, no lanes, no band, no early stop: it shares nothing with the kernel).  X4: every
cell with D <= max_edits is a candidate of value i + j - penalty * D, plus end_bonus in row f.  X5: the largest value, then
the smaller D, then the larger i.  X6 and X7 put the row together.

flank_best_many() runs the table for many flanks at once, padded to the longest: a row of every table per step."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import _verify_worker as VW  # noqa: E402
from conftest import revcomp  # noqa: E402

UNPLACED = 0xFFFFFFFF
PENALTY, END_BONUS, MAX_EDITS = 6, 4, 1023  # the conventions of the layers above
EXTENSION_FIELDS = [("read_start", np.uint32), ("read_end", np.uint32), ("ref_start", np.uint64), ("ref_end", np.uint64),
                    ("left_edits", np.uint32), ("right_edits", np.uint32)]
_LOWEST = np.iinfo(np.int64).min // 4


def _chunk_best(flanks, penalty, end_bonus, max_edits):
    """rules X3-X5 for a chunk of flanks [(U, V)] -> int64[B, 3] of (i*, j*, D*)"""
    B = len(flanks)
    f = np.array([len(u) for u, _ in flanks], np.int64)
    g = np.array([len(v) for _, v in flanks], np.int64)
    M, Nn = int(f.max()), int(g.max())
    Ua, Va = np.full((B, max(M, 1)), -3, np.int16), np.full((B, max(Nn, 1)), -4, np.int16)
    for b, (u, v) in enumerate(flanks):
        Ua[b, :f[b]] = VW.encode(u, -1)
        Va[b, :g[b]] = VW.encode(v, -2)
    Va = Va[:, :Nn]
    idx = np.arange(Nn + 1, dtype=np.int32)
    in_v = idx[None, :] <= g[:, None]
    rows = np.arange(B)
    best = np.zeros((B, 3), np.int64)  # i, j, D
    best_value = np.full(B, _LOWEST, np.int64)
    D = np.tile(idx, (B, 1))  # row 0: D[0][j] = j  (int32: a distance is at most max(f, g))
    lowest = np.int32(np.iinfo(np.int32).min // 2)
    assert penalty * (M + Nn) + end_bonus < -int(lowest)
    for i in range(M + 1):
        if i > 0:
            x = np.empty((B, Nn + 1), np.int32)
            x[:, 0] = i
            x[:, 1:] = np.minimum(D[:, :-1] + (Va != Ua[:, i - 1:i]), D[:, 1:] + 1)  # substitution / match, a base of U alone
            D = np.minimum.accumulate(x - idx, axis=1) + idx                           # a base of V alone
        live = i <= f
        if not live.any():
            break
        candidate = in_v & (D <= max_edits) & live[:, None]
        value = np.where(candidate, (i + idx)[None, :] - np.int32(penalty) * D + np.where(i == f, end_bonus, 0).astype(np.int32)[:, None], lowest)
        # within a row the value and D give j, and of two cells of one value the one with the smaller D has the smaller j:
        # the first of the largest
        j = np.argmax(value, axis=1)
        v, d = value[rows, j].astype(np.int64), D[rows, j].astype(np.int64)
        v[~live] = _LOWEST
        # against the rows before: the larger value; then the smaller D; then this row, whose i is larger
        better = (v > best_value) | ((v == best_value) & live & (d <= best[:, 2]))
        best_value = np.where(better, v, best_value)
        best[better] = np.stack([np.full(B, i, np.int64), j, d], axis=1)[better]
    return best


def flank_best_many(flanks, penalty=PENALTY, end_bonus=END_BONUS, max_edits=MAX_EDITS, chunk=256):
    """[(U, V)] -> int64[len(flanks), 3]: (i*, j*, D*) of every flank.  Chunks of flanks of similar f: the tables of a chunk
    are as tall as its longest U and as wide as its longest V."""
    out = np.zeros((len(flanks), 3), np.int64)
    # (D[i][j] >= j - i >= j - f: a cell behind column f + max_edits is no candidate by rule X4, and no column of the table
    # depends on a later one, so those columns are not computed)
    flanks = [(u, v[:len(u) + max_edits]) for u, v in flanks]
    order = sorted(range(len(flanks)), key=lambda t: (len(flanks[t][0]), len(flanks[t][1])))
    at = 0
    while at < len(order):
        ids, width = [], 0
        while at < len(order) and len(ids) < chunk:
            w = max(width, len(flanks[order[at]][1]) + 1)
            if ids and (len(ids) + 1) * w > 1 << 19:
                break
            ids.append(order[at])
            width = w
            at += 1
        out[ids] = _chunk_best([flanks[t] for t in ids], penalty, end_bonus, max_edits)
    return out


def flank_best(U, V, penalty=PENALTY, end_bonus=END_BONUS, max_edits=MAX_EDITS):
    """one flank -> (i*, j*, D*)"""
    return tuple(int(x) for x in flank_best_many([(bytes(U), bytes(V))], penalty, end_bonus, max_edits)[0])


def flanks_of(read, record, row):
    """rule X2 for a placed row -> ((U_left, V_left), (U_right, V_right)), and (a, b, L)"""
    read, record = bytes(read), bytes(record)
    L, rev = len(read), int(row["reverse"])
    oriented = revcomp(read) if rev else read
    rs, re = int(row["read_start"]), int(row["read_end"])
    a, b = (L - re, L - rs) if rev else (rs, re)
    fs, fe = int(row["ref_start"]), int(row["ref_end"])
    return ((oriented[:a][::-1], record[:fs][::-1]), (oriented[b:], record[fe:])), (a, b, L)


def extend_rows(reads, records, rows, row_offsets=None, penalty=PENALTY, end_bonus=END_BONUS, max_edits=MAX_EDITS):
    """the model of dcn_extend_batch -> (rows_extended, extension), as Placer.extend_batch returns them"""
    owner = np.arange(len(rows)) if row_offsets is None else np.repeat(np.arange(len(reads)), np.diff(np.asarray(row_offsets, np.int64)))
    assert len(owner) == len(rows)
    ext = np.zeros(len(rows), np.dtype(EXTENSION_FIELDS))
    for name in ("read_start", "read_end", "ref_start", "ref_end"):
        ext[name] = rows[name]
    placed = [t for t in range(len(rows)) if int(rows["record"][t]) != UNPLACED]
    flanks = []
    for t in placed:
        (left, right), _ = flanks_of(reads[owner[t]], records[int(rows["record"][t])], rows[t])
        flanks += [left, right]
    best = flank_best_many(flanks, penalty, end_bonus, max_edits)
    for n, t in enumerate(placed):
        (il, jl, dl), (ir, jr, dr) = best[2 * n].tolist(), best[2 * n + 1].tolist()
        rev = int(rows["reverse"][t])
        ext["read_start"][t] -= ir if rev else il  # rule X6
        ext["read_end"][t] += il if rev else ir
        ext["ref_start"][t] -= jl
        ext["ref_end"][t] += jr
        ext["left_edits"][t], ext["right_edits"][t] = dl, dr
    out = np.array(rows, copy=True)
    for name in ("read_start", "read_end", "ref_start", "ref_end"):
        out[name] = ext[name]
    return out, ext


def clips(read_len, row):
    """rule X6's soft clips of a row (extended or not), in the record's direction -> (left, right)"""
    rs, re = int(row["read_start"]), int(row["read_end"])
    return (read_len - re, rs) if int(row["reverse"]) else (rs, read_len - re)

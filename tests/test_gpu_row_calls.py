"""The front end that the four row calls share (verify, align, pileup, extend): one context serves them in turn with row
counts that grow and then shrink again -- 1, 300, 2, 300, 1, 2 -- so that the items of one kind of call are staged into
buffers another call has grown, and a small call runs in buffers a large one left behind.  Every result is byte for byte
what the same call returns on a fresh context."""
import numpy as np
import pytest

import _verify_worker as VW
from conftest import random_reads, revcomp

pytestmark = pytest.mark.gpu

UNPLACED = VW.UNPLACED


def make_rows(dtype, n_rows):
    """n_rows hand-made rows over two reads of 60 bases, record[100:160] forwards and record[250:310] backwards: intervals
    that leave flanks of 3 .. 16 bases; one row unplaced when there are more than two"""
    first = (n_rows + 1) // 2
    rows = np.zeros(n_rows, dtype)
    for q in range(n_rows):
        a, b = 10 + q % 7, 50 - q % 5 + q % 3
        if q < first:
            rows[q:q + 1] = VW.make_row(dtype, 0, 0, a, b, 100 + a, 100 + b)
        else:
            rows[q:q + 1] = VW.make_row(dtype, 0, 1, a, b, 310 - b, 310 - a)
    if n_rows > 2:
        rows["record"][7 % n_rows] = UNPLACED
    return rows, np.array([0, first, n_rows], np.uint64)


def run(kind, placer, amap, b, o, rows, ro):
    """one call -> its results as a tuple of byte strings"""
    if kind == "verify":
        out = (placer.verify_batch(b, o, rows, row_offsets=ro),)
    elif kind == "align":
        out = placer.align_batch(b, o, rows, row_offsets=ro)
    elif kind == "extend":
        out = placer.extend_batch(b, o, rows, row_offsets=ro)
    else:
        amap.pileup_reset()
        edits, n_added = placer.pileup_batch(b, o, rows, row_offsets=ro)
        out = (edits, np.array([n_added]), amap.pileup_fetch(0))
    return tuple(np.ascontiguousarray(x).tobytes() for x in out)


def test_row_calls_share_one_context(dcn, oracle):
    rng = np.random.default_rng(1701)
    record = random_reads(rng, 1, 400, 400)[0]
    amap = VW.build_map(oracle, dcn, [record])
    amap.pileup_enable()
    read0 = bytearray(record[100:160])
    for at in (4, 30):  # an edit in the left flank of every row and one inside every interval
        read0[at] = b"ACGT"[(b"ACGT".find(bytes([read0[at]])) + 1) % 4]
    reads = [bytes(read0), revcomp(record[250:310])]
    b, o = oracle.concat_reads(reads)
    shared = dcn.Placer(amap, max_batch_bases=1 << 16, max_batch_reads=1 << 8)
    sequence = [("verify", 1), ("extend", 300), ("align", 2), ("verify", 300), ("extend", 1), ("pileup", 2)]
    for kind, n_rows in sequence:
        rows, ro = make_rows(dcn.filter.PLACEMENT_DTYPE, n_rows)
        got = run(kind, shared, amap, b, o, rows, ro)
        fresh = dcn.Placer(amap, max_batch_bases=1 << 16, max_batch_reads=1 << 8)
        want = run(kind, fresh, amap, b, o, rows, ro)
        fresh.close()
        assert got == want, (kind, n_rows)
        # (the calls do something: the model's distances, flanks that are carried to the read's ends, counts in the pileup)
        if kind in ("verify", "align", "pileup"):
            assert np.frombuffer(got[0], np.uint32).tolist() == VW.verify_rows(reads, [record], rows, row_offsets=ro).tolist()
        if kind == "extend":
            xrows = np.frombuffer(got[0], rows.dtype)
            placed = rows["record"] != UNPLACED
            assert (xrows["read_start"][placed] == 0).all() and (xrows["read_end"][placed] == 60).all()
        if kind == "pileup":
            assert np.frombuffer(got[1], np.int64)[0] == 2 and np.frombuffer(got[2], np.uint32).sum() > 0
    shared.close()
    amap.close()

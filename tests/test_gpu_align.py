"""dcn_align_batch on the rows the three placement calls return, against the model of tests/_align_worker.py (a full table
and a walk by rule A3: no wavefront): reads cut from three 20 kbp random records -- error-free, with 5 % mixed edits, on
both strands, chimeras, unplaced reads, reads with N and lower case -- at (k, w) = (31, 15), (31, 1), (33, 15).  The
DCN_ERR_CAPACITY protocol, the two new argument errors, and one context serving split, verify, align, locate, align."""
import ctypes as C

import numpy as np
import pytest

import _align_worker as AW
import _verify_worker as VW
from conftest import random_reads, revcomp

pytestmark = pytest.mark.gpu

CASES = [(31, 15), (31, 1), (33, 15)]
OVER, UNPLACED = VW.OVER, VW.UNPLACED


def make_records():
    recs = random_reads(np.random.default_rng(1431), 3, 20_000, 20_000)
    low = bytearray(recs[2])
    low[5000:5400] = bytes(low[5000:5400]).lower()
    low[9000:9003] = b"NNN"
    return [recs[0], recs[1], bytes(low)]


def make_reads(records):
    rng = np.random.default_rng(1432)

    def cut(lo, hi):
        while True:  # (not across the record's NNN)
            R, ln = int(rng.integers(0, 3)), int(rng.integers(lo, hi + 1))
            at = int(rng.integers(0, 20_000 - ln))
            if not (R == 2 and at < 9010 and at + ln > 8990):
                return records[R][at:at + ln]

    reads = []
    for _ in range(12):
        reads.append(cut(100, 300))                                   # error-free: one run of '='
        reads.append(revcomp(cut(100, 300)))
        reads.append(VW.mutate_mixed(rng, cut(200, 500), 0.05))       # 5 % mixed edits
        reads.append(revcomp(VW.mutate_mixed(rng, cut(200, 500), 0.05)))
    for _ in range(4):
        reads.append(cut(150, 300) + revcomp(cut(150, 300)))          # chimeras
        reads.append(VW.mutate_mixed(rng, cut(200, 300), 0.03) + cut(100, 200) + cut(100, 200))
        s = bytearray(cut(200, 400))
        s[100:103] = b"NNN"
        reads.append(bytes(s))                                        # N in the read
        reads.append(cut(150, 300).lower())
    reads += [records[2][4900:5500], revcomp(records[2][8900:9100]), records[2][8950:9050].lower()]  # lower case and N in the record
    reads += random_reads(rng, 5, 50, 300) + [b"", b"ACGT", records[0][:30]]                          # unplaced
    reads.append(VW.mutate_mixed(rng, records[1][2000:4500], 0.08))                                   # a long read
    if len(reads) % 2:
        reads.append(records[0][700:900])
    return reads


@pytest.fixture(scope="module")
def built(dcn, oracle):
    records = make_records()
    reads = make_reads(records)
    out = {}
    for k, w in CASES:
        amap = VW.build_map(oracle, dcn, records, k, w)
        placer = dcn.Placer(amap, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
        out[(k, w)] = (amap, placer)
    yield records, reads, oracle.concat_reads(reads), out
    for amap, placer in out.values():
        placer.close()
        amap.close()


@pytest.mark.parametrize("k,w", CASES)
def test_rows_of_the_three_placement_calls(built, dcn, k, w):
    records, reads, (b, o), maps = built
    amap, placer = maps[(k, w)]
    # dcn_place_batch: stride 48, row r belongs to read r
    rows = placer.place_batch(b, o)
    got = placer.align_batch(b, o, rows)
    want = AW.align_rows(reads, records, rows)
    AW.assert_same(got, want, rows)
    assert got[0].tolist() == placer.verify_batch(b, o, rows).tolist()  # edits is exactly dcn_verify_batch's
    placed = rows["record"] != UNPLACED
    assert placed.sum() > 60 and (~placed).sum() >= 5
    n_ops = np.diff(got[1].astype(np.int64))
    assert (n_ops[(got[0] >= OVER)] == 0).all() and (n_ops[got[0] == 0] == 1).all() and (n_ops[(got[0] > 0) & (got[0] < OVER)] >= 2).all()
    assert (got[0][:48:4][placed[:48:4]] == 0).all() and ((got[0][2:48:4] > 0) & (got[0][2:48:4] < OVER)).sum() > 5
    kinds = {int(x) & 15 for x in got[2]}
    assert kinds == {AW.OP_I, AW.OP_D, AW.OP_EQ, AW.OP_X}
    assert dcn.cigar_string(got[2][int(got[1][0]):int(got[1][1])]) == AW.cigar_text(want[2][int(want[1][0]):int(want[1][1])])
    # dcn_place_split_batch: stride 64, CSR
    po, srows, _ = placer.place_split_batch(b, o, max_placements=4)
    sgot = placer.align_batch(b, o, srows, row_offsets=po)
    AW.assert_same(sgot, AW.align_rows(reads, records, srows, row_offsets=po), srows)
    assert sgot[0].tolist() == placer.verify_batch(b, o, srows, row_offsets=po).tolist()
    assert (np.diff(po.astype(np.int64)) >= 2).sum() >= 4
    # dcn_place_pair_batch: stride 80, one row per read
    prows, _ = placer.place_pair_batch(b, o)
    AW.assert_same(placer.align_batch(b, o, prows), AW.align_rows(reads, records, prows), prows)
    # a tighter threshold: the rows it leaves have the runs they had, the others none
    tight = placer.align_batch(b, o, rows, max_edits=10, max_permille=30)
    AW.assert_same(tight, AW.align_rows(reads, records, rows, max_edits=10, max_permille=30), rows)
    assert (tight[0] == OVER).sum() > (got[0] == OVER).sum()


def raw_align(dcn, placer, b, o, rows, ro, capacity, cigar_null=False, offsets_null=False):
    """dcn_align_batch itself -> (rc, edits, cigar_offsets, cigar): the buffers as the call left them"""
    N = dcn._native
    p = N.VerifyParams(1023, 200, rows.dtype.itemsize, 0)
    edits = np.full(len(rows), 0xABABABAB, np.uint32)
    offs = np.full(len(rows) + 1, 0xABABABABABABABAB, np.uint64)
    cigar = np.full(max(capacity, 1), 0xABABABAB, np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = N.lib().dcn_align_batch(placer._h, placer.anchor_map._h, ptr(b), ptr(o), len(o) - 1, C.byref(p), ptr(ro), ptr(rows), len(rows),
                                 ptr(edits), None if offsets_null else ptr(offs), None if cigar_null else ptr(cigar), capacity)
    return rc, edits, offs, cigar


def test_capacity_protocol(built, dcn):
    """capacity 0 with NULL, one short, exact: edits and cigar_offsets complete, cigar untouched until the runs fit"""
    records, reads, (b, o), maps = built
    _, placer = maps[(31, 15)]
    N = dcn._native
    po, srows, _ = placer.place_split_batch(b, o, max_placements=4)
    po = np.ascontiguousarray(po, np.uint64)
    want = AW.align_rows(reads, records, srows, row_offsets=po)
    total = int(want[1][-1])
    assert total > 200
    rc, edits, offs, _ = raw_align(dcn, placer, b, o, srows, po, 0, cigar_null=True)
    assert rc == N.DCN_ERR_CAPACITY and str(total).encode() in N.lib().dcn_last_error()
    assert edits.tolist() == want[0].tolist() and offs.tolist() == want[1].tolist()
    rc, edits, offs, cigar = raw_align(dcn, placer, b, o, srows, po, total - 1)
    assert rc == N.DCN_ERR_CAPACITY and edits.tolist() == want[0].tolist() and offs.tolist() == want[1].tolist()
    assert (cigar == 0xABABABAB).all()  # not written
    rc, edits, offs, cigar = raw_align(dcn, placer, b, o, srows, po, total)
    assert rc == 0 and edits.tolist() == want[0].tolist() and offs.tolist() == want[1].tolist() and cigar.tolist() == want[2].tolist()
    rc, _, _, cigar = raw_align(dcn, placer, b, o, srows, po, total + 5)
    assert rc == 0 and cigar[:total].tolist() == want[2].tolist() and (cigar[total:] == 0xABABABAB).all()
    # the Python mirror: one call with an estimate, a second with the size reported; a given capacity raises
    AW.assert_same(placer.align_batch(b, o, srows, row_offsets=po), want, srows)
    AW.assert_same(placer.align_batch(b, o, srows, row_offsets=po, capacity=total), want, srows)
    with pytest.raises(dcn.DeaconHipError) as e:
        placer.align_batch(b, o, srows, row_offsets=po, capacity=total - 1)
    assert e.value.code == N.DCN_ERR_CAPACITY
    # the two argument errors of this call alone
    rc, *_ = raw_align(dcn, placer, b, o, srows, po, total, offsets_null=True)
    assert rc == N.DCN_ERR_ARG and b"cigar_offsets is NULL" in N.lib().dcn_last_error()
    rc, *_ = raw_align(dcn, placer, b, o, srows, po, total, cigar_null=True)
    assert rc == N.DCN_ERR_ARG and b"cigar is NULL" in N.lib().dcn_last_error()
    # a bad row is named as dcn_verify_batch names it
    bad = srows.copy()
    bad["ref_end"][3] = 20_001
    with pytest.raises(dcn.DeaconHipError) as e:
        placer.align_batch(b, o, bad, row_offsets=po)
    assert e.value.code == N.DCN_ERR_ARG and "row 3: ref_end 20001 is past the record's 20000 bases" in e.value.message
    with pytest.raises(dcn.DeaconHipError) as e2:
        placer.verify_batch(b, o, bad, row_offsets=po)
    assert e2.value.message == e.value.message


def test_one_context_serves_every_call(built, dcn):
    """split, verify, align, locate and align again on one context; the counters stay; profiling sees pack and finish"""
    records, reads, (b, o), maps = built
    amap, placer = maps[(31, 15)]
    po, srows, _ = placer.place_split_batch(b, o)
    edits = placer.verify_batch(b, o, srows, row_offsets=po)
    first = placer.align_batch(b, o, srows, row_offsets=po)
    assert first[0].tolist() == edits.tolist()
    few = reads[:40]
    fb, fo = dcn.concat_reads(few)
    N = dcn._native
    lp = N.LocateParams(2 * 15 - 1, 1, 0xFFFFFFFF, 0, 0)
    seg_off = np.zeros(len(few) + 1, np.uint64)
    rc = N.lib().dcn_locate_batch(placer._h, amap._h, fb.ctypes.data_as(C.c_void_p), fo.ctypes.data_as(C.c_void_p), len(few), C.byref(lp),
                                  seg_off.ctypes.data_as(C.c_void_p), None, 0)
    assert rc in (0, N.DCN_ERR_CAPACITY) and int(seg_off[-1]) > 0
    again = placer.align_batch(b, o, srows, row_offsets=po)
    assert all(np.array_equal(x, y) for x, y in zip(first, again))
    assert placer.verify_batch(b, o, srows, row_offsets=po).tolist() == edits.tolist()
    before = placer.stats()
    placer.align_batch(b, o, srows, row_offsets=po)
    assert placer.stats() == before  # the six counters are untouched
    placer.set_profiling(True)
    placer.align_batch(b, o, srows, row_offsets=po, capacity=int(first[1][-1]))
    ms, n = placer.profile()
    placer.set_profiling(False)
    assert n == 1 and ms["pack"] > 0 and ms["finish"] > 0

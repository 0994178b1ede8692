"""dcn_verify_batch on the rows the three placement calls return, against the model of tests/_verify_worker.py: reads cut from
three 20 kbp random records -- error-free (edits 0), with 5 % mixed edits, on both strands, chimeras, unplaced reads, reads
with N and lower case -- at (k, w) = (31, 15), (31, 1), (33, 15).  Kept bases: fetch round-trips records and ranges, the
store does not depend on how the records were spread over add calls, and a map that keeps bases places exactly as one that
does not."""
import numpy as np
import pytest

import _verify_worker as VW
from conftest import random_reads, revcomp

pytestmark = pytest.mark.gpu

CASES = [(31, 15), (31, 1), (33, 15)]
OVER, UNPLACED = VW.OVER, VW.UNPLACED


def make_records():
    recs = random_reads(np.random.default_rng(1321), 3, 20_000, 20_000)
    low = bytearray(recs[2])
    low[5000:5400] = bytes(low[5000:5400]).lower()
    low[9000:9003] = b"NNN"
    return [recs[0], recs[1], bytes(low)]


def make_reads(records):
    rng = np.random.default_rng(1322)

    def cut(lo, hi):
        while True:  # (not across the record's NNN: a cut would carry them, and N equals nothing)
            R, ln = int(rng.integers(0, 3)), int(rng.integers(lo, hi + 1))
            at = int(rng.integers(0, 20_000 - ln))
            if not (R == 2 and at < 9010 and at + ln > 8990):
                return records[R][at:at + ln]

    reads = []
    for _ in range(30):
        reads.append(cut(100, 400))                                   # error-free: edits 0
        reads.append(revcomp(cut(100, 400)))
        reads.append(VW.mutate_mixed(rng, cut(200, 600), 0.05))       # 5 % mixed edits
        reads.append(revcomp(VW.mutate_mixed(rng, cut(200, 600), 0.05)))
    for _ in range(8):
        reads.append(cut(150, 300) + revcomp(cut(150, 300)))          # chimeras
        reads.append(VW.mutate_mixed(rng, cut(200, 300), 0.03) + cut(100, 200) + cut(100, 200))
        s = bytearray(cut(200, 400))
        s[100:103] = b"NNN"
        reads.append(bytes(s))                                        # N in the read
        reads.append(cut(150, 300).lower())
    reads += [records[2][4900:5500], revcomp(records[2][8900:9100]), records[2][8950:9050].lower()]  # lower case and N in the record
    reads += random_reads(rng, 10, 50, 300) + [b"", b"ACGT", records[0][:30]]                         # unplaced
    reads.append(VW.mutate_mixed(rng, records[1][2000:6000], 0.08))                                   # a long read
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


def compare(got, want, rows, what):
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (what, [(int(i), int(got[i]), int(want[i]), rows[i]) for i in bad[:5]])


@pytest.mark.parametrize("k,w", CASES)
def test_rows_of_the_three_placement_calls(built, k, w):
    records, reads, (b, o), maps = built
    amap, placer = maps[(k, w)]
    # dcn_place_batch: stride 48, row r belongs to read r
    rows = placer.place_batch(b, o)
    got = placer.verify_batch(b, o, rows)
    want = VW.verify_rows(reads, records, rows)
    compare(got, want, rows, ("place", k, w))
    placed = rows["record"] != UNPLACED
    assert placed.sum() > 150 and (~placed).sum() >= 10 and (got[~placed] == UNPLACED).all()
    assert (got[:120:4][placed[:120:4]] == 0).all() and (got[1:120:4][placed[1:120:4]] == 0).all()  # the error-free cuts, both strands
    noisy = got[2:120:4][placed[2:120:4]]
    assert ((noisy > 0) & (noisy != OVER)).sum() > 10  # 5 % of 200 .. 600 bases, under the threshold of 20 %
    # dcn_place_split_batch: stride 64, CSR
    po, srows, _ = placer.place_split_batch(b, o, max_placements=4)
    got = placer.verify_batch(b, o, srows, row_offsets=po)
    compare(got, VW.verify_rows(reads, records, srows, row_offsets=po), srows, ("split", k, w))
    assert (np.diff(po.astype(np.int64)) >= 2).sum() >= 8 and not (got == UNPLACED).any()
    rank0 = srows["rank"] == 0
    assert got[rank0].tolist() == want[placed].tolist()  # round 0 is dcn_place_batch's placement
    # dcn_place_pair_batch: stride 80, one row per read
    prows, _ = placer.place_pair_batch(b, o)
    got = placer.verify_batch(b, o, prows)
    compare(got, VW.verify_rows(reads, records, prows), prows, ("pair", k, w))
    # a tighter threshold: the same distances, more of them OVER
    tight = placer.verify_batch(b, o, rows, max_edits=10, max_permille=30)
    compare(tight, VW.verify_rows(reads, records, rows, max_edits=10, max_permille=30), rows, ("tight", k, w))
    assert (tight == OVER).sum() > (want == OVER).sum()


def test_fetch_round_trips(built):
    records, _, _, maps = built
    amap, _ = maps[(31, 15)]
    rng = np.random.default_rng(1323)
    for R, rec in enumerate(records):
        assert amap.fetch(R, 0, len(rec)) == VW.fetched_text(rec)
        for _ in range(20):
            a = int(rng.integers(0, len(rec)))
            n = int(rng.integers(0, min(len(rec) - a, 300) + 1))
            assert amap.fetch(R, a, n) == VW.fetched_text(rec[a:a + n])
    assert amap.fetch(2, 8998, 7)[2:5] == b"NNN" and amap.fetch(2, 8998, 7) == VW.fetched_text(records[2][8998:9005])
    assert amap.fetch(2, 5000, 400) == records[2][5000:5400].upper()


def test_fetch_errors(built, dcn):
    records, _, _, maps = built
    amap, _ = maps[(31, 15)]
    for args, word in (((3, 0, 1), "record 3 of 3 added"), ((0, 20_000, 1), "past the record's 20000 bases"),
                       ((0, 19_999, 2), "past the record's 20000 bases"), ((1, 20_001, 0), "past the record's 20000 bases")):
        with pytest.raises(dcn.DeaconHipError) as e:
            amap.fetch(*args)
        assert e.value.code == dcn._native.DCN_ERR_ARG and word in e.value.message, e.value.message


def test_one_add_call_or_several(built, dcn, oracle):
    """the records spread over three add calls: the same fetches and the same edits, and the same placements as a map that
    keeps no bases, field for field"""
    records, reads, (b, o), maps = built
    amap, placer = maps[(31, 15)]
    spread = VW.build_map(oracle, dcn, records, calls=[1, 1, 1])
    plain = VW.build_map(oracle, dcn, records, keep_bases=False)
    p2 = dcn.Placer(spread, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    p3 = dcn.Placer(plain, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    try:
        for R, rec in enumerate(records):
            assert spread.fetch(R, 0, len(rec)) == amap.fetch(R, 0, len(rec))
        rows = placer.place_batch(b, o)
        assert rows.tobytes() == p2.place_batch(b, o).tobytes() == p3.place_batch(b, o).tobytes()
        po, srows, counts = placer.place_split_batch(b, o)
        for other in (p2, p3):
            po2, srows2, counts2 = other.place_split_batch(b, o)
            assert po.tolist() == po2.tolist() and srows.tobytes() == srows2.tobytes() and counts.tolist() == counts2.tolist()
        assert placer.place_pair_batch(b, o)[0].tobytes() == p3.place_pair_batch(b, o)[0].tobytes()
        assert placer.verify_batch(b, o, srows, row_offsets=po).tolist() == p2.verify_batch(b, o, srows, row_offsets=po).tolist()
        assert spread.info() == amap.info() == plain.info()
        # a map that keeps no bases: no fetch, no verify
        with pytest.raises(dcn.DeaconHipError) as e:
            p3.verify_batch(b, o, rows)
        assert e.value.code == dcn._native.DCN_ERR_ARG and "keeps no bases" in e.value.message
        with pytest.raises(dcn.DeaconHipError) as e:
            plain.fetch(0, 0, 10)
        assert e.value.code == dcn._native.DCN_ERR_ARG and "keeps no bases" in e.value.message
        # keep_bases after an add
        assert dcn._native.lib().dcn_anchor_map_keep_bases(plain._h) == dcn._native.DCN_ERR_ARG
        assert b"before the first dcn_anchor_map_add" in dcn._native.lib().dcn_last_error()
        assert dcn._native.lib().dcn_anchor_map_keep_bases(amap._h) == 0  # idempotent on a map that keeps them
        idx = dcn.Index.from_keys(np.arange(1, 50, dtype=np.uint64), 31, 15)
        assert dcn._native.lib().dcn_anchor_map_keep_bases(idx._h) == dcn._native.DCN_ERR_ARG  # not a map
        idx.close()
        # a clone is a plain index: the store stays behind
        clone = amap.clone(0)
        assert dcn._native.lib().dcn_anchor_map_fetch(clone._h, 0, 0, 1, None) == dcn._native.DCN_ERR_ARG
        clone.close()
    finally:
        p2.close()
        p3.close()
        spread.close()
        plain.close()


def test_one_context_serves_every_call(built, dcn):
    """place, split, verify, locate and verify again on one context: the verify call stages and packs its own batch"""
    records, reads, (b, o), maps = built
    amap, placer = maps[(31, 15)]
    rows = placer.place_batch(b, o)
    po, srows, _ = placer.place_split_batch(b, o)
    first = placer.verify_batch(b, o, srows, row_offsets=po)
    few = reads[:40]
    fb, fo = dcn.concat_reads(few)
    import ctypes as C
    N = dcn._native
    lp = N.LocateParams(2 * 15 - 1, 1, 0xFFFFFFFF, 0, 0)
    seg_off = np.zeros(len(few) + 1, np.uint64)
    rc = N.lib().dcn_locate_batch(placer._h, amap._h, fb.ctypes.data_as(C.c_void_p), fo.ctypes.data_as(C.c_void_p), len(few), C.byref(lp),
                                  seg_off.ctypes.data_as(C.c_void_p), None, 0)
    assert rc in (0, N.DCN_ERR_CAPACITY) and int(seg_off[-1]) > 0  # (the count alone: the batch in the context is now another)
    again = placer.verify_batch(b, o, srows, row_offsets=po)
    assert first.tolist() == again.tolist()
    assert placer.verify_batch(b, o, rows).tolist() == VW.verify_rows(reads, records, rows).tolist()
    before = placer.stats()
    placer.verify_batch(b, o, rows)
    assert placer.stats() == before  # the six counters are untouched
    placer.set_profiling(True)
    placer.verify_batch(b, o, rows)
    ms, n = placer.profile()
    placer.set_profiling(False)
    assert n == 1 and ms["pack"] > 0 and ms["finish"] > 0

"""The seams of the anchor and placement kernels, with hits placed base by base: w = 1, so every position of a read is a
minimizer and a cut of n bases from a record has n - k + 1 anchor hits on one diagonal.  Everything is compared with the
model of tests/_place_worker.py exactly; where the construction fixes the outcome it is asserted as well.

Not covered here (DESIGN.md section 17 says so too): a diagonal above 2^32 (it needs a record of 2^32 bases), key 0's
word (reaching it needs an XXH3 preimage of 0), and batches past 2^32 bases.

On cell sharing: by the definition, cell j collects the diagonals of [(j-1)W, (j+1)W), so two groups of hits whose
diagonals differ by less than W always share a cell, groups that differ by exactly W share one as well (x and x + W both
lie in the cell that starts at x - x % W), groups 2W apart never do, and between the two it depends on x % W."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _place_worker as PW
from _place_worker import AnchorModel, assert_map, assert_placements, place
from conftest import random_reads, revcomp

pytestmark = pytest.mark.gpu

K = 31
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_place_worker.py")
BANDS = (1, 2, 31, 256)


@pytest.fixture(scope="module")
def ref(oracle, dcn):
    """two random records of 5,000 and 300 bases at w = 1: (records, model, map)"""
    rng = np.random.default_rng(931)
    records = random_reads(rng, 1, 5000, 5000) + random_reads(rng, 1, 300, 300)
    model, amap = PW.build_map(oracle, dcn, records, K, 1)
    assert model.info() == {"records": 2, "keys": 5000 - K + 1 + 300 - K + 1, "anchors": 5240, "repeats": 0}
    assert_map(amap, model)
    yield records, model, amap
    amap.close()


def check(oracle, dcn, ref, reads, **kw):
    records, model, amap = ref
    got = place(dcn, amap, reads, oracle, **kw)
    want = model.place_all(reads, W=kw.get("band_bases", 256), min_votes=kw.get("min_votes", 2))
    assert_placements(got, want, tuple(kw.items()))
    return got


@pytest.mark.parametrize("W", BANDS)
def test_band_edges(oracle, dcn, ref, W):
    """cuts whose diagonal is j*W - 1, j*W and j*W + 1, on both strands (D = a + len forward, a + len - k reverse); every
    hit of a cut has that diagonal, so its cells j and j + 1 tie and the smaller wins, with the same extents"""
    rec = ref[0][0]
    reads, want = [], []
    for ln in (K, 64, 80):
        for j in (1, 7):
            for d in (-1, 0, 1):
                for rev in (0, 1):
                    D = max(j * W, 512) // W * W + d
                    a = D - ln + (K if rev else 0)
                    s = rec[a:a + ln]
                    reads.append(revcomp(s) if rev else s)
                    want.append((0, rev, ln - K + 1, a, a + ln))
    got = check(oracle, dcn, ref, reads, band_bases=W, min_votes=1)
    assert [(int(g["record"]), int(g["reverse"]), int(g["votes"]), int(g["ref_start"]), int(g["ref_end"])) for g in got] == want
    assert (got["read_start"] == 0).all() and (got["votes"] == got["n_anchors"]).all() and (got["votes"] == got["n_positions"]).all()


@pytest.mark.parametrize("W", BANDS)
def test_cell_sharing(oracle, dcn, ref, W):
    """two cuts of 60 bases with one base inserted between them; the second cut starts `gap` bases further on the record
    than the read goes on, so the two groups of 30 hits have diagonals gap apart"""
    rec = ref[0][0]
    reads, gaps = [], []
    for a in (1000, 1000 + W // 2, 1000 + W - 1):
        for gap in (0, W - 1, W, 2 * W - 1, 2 * W, 3 * W + 1):
            b = a + 61 + gap
            reads.append(rec[a:a + 60] + b"N" + rec[b:b + 60])
            gaps.append(gap)
    got = check(oracle, dcn, ref, reads, band_bases=W, min_votes=1)
    assert (got["n_anchors"] == 60).all()
    for g, gap in zip(got, gaps):
        if gap <= W:
            assert g["votes"] == 60 and (g["read_start"], g["read_end"]) == (0, 121), (W, gap)
        if gap >= 2 * W:
            assert g["votes"] == 30 and g["read_end"] - g["read_start"] == 60, (W, gap)


def test_whole_record_and_min_votes(oracle, dcn, ref):
    """a read that is the whole record, on both strands (the lane path and, for the long record, the workgroup path);
    min_votes at votes - 1, votes and votes + 1"""
    records = ref[0]
    reads = [records[1], revcomp(records[1]), records[0], revcomp(records[0])]
    got = check(oracle, dcn, ref, reads)
    assert got["record"].tolist() == [1, 1, 0, 0] and got["reverse"].tolist() == [0, 1, 0, 1]
    assert got["ref_start"].tolist() == [0] * 4 and got["ref_end"].tolist() == [300, 300, 5000, 5000]
    assert got["read_end"].tolist() == [300, 300, 5000, 5000] and got["votes"].tolist() == [270, 270, 4970, 4970]
    read = [records[0][2000:2060]]  # 30 votes
    for votes, placed in ((29, True), (30, True), (31, False)):
        got = check(oracle, dcn, ref, read, min_votes=votes)
        assert (got["record"][0] == 0) == placed and got["n_anchors"][0] == 30 and got["votes"][0] == (30 if placed else 0)


def test_bitmap_words(oracle, dcn, ref):
    """reads that start at every offset mod 32 of the batch stream, and neighbours that share a bitmap word: reads of k
    bases have one position each, at their first base, beside reads of k + 1 and k - 1 bases and reads that hit nothing"""
    rec = ref[0][0]
    rng = np.random.default_rng(932)
    reads = []
    for i in range(300):
        ln = (K, K + 1, K - 1, K, 33, K, 41)[i % 7]
        a = int(rng.integers(0, 4900))
        s = rec[a:a + ln]
        reads.append(random_reads(rng, 1, ln, ln)[0] if i % 11 == 4 else (revcomp(s) if i % 3 == 0 else s))
    starts = np.cumsum([0] + [len(r) for r in reads[:-1]])
    assert set((starts % 32).tolist()) == set(range(32))
    got = check(oracle, dcn, ref, reads, band_bases=31, min_votes=1)
    assert int((got["votes"] == 1).sum()) > 100 and int((got["n_positions"] == 0).sum()) > 30


def test_anchor_protocol_under_contention(oracle, dcn):
    """a record of one 64-base unit repeated 500 times: every key occurs at 499 or 500 positions and is a repeat; the same
    unit once (with the unit's first k - 1 bases behind it, so that it has the same 64 keys): every key is an anchor"""
    unit = random_reads(np.random.default_rng(933), 1, 64, 64)[0]
    many, once = unit * 500, unit + unit[:K - 1]
    keys = oracle.Index.build([once], k=K, w=1).keys()
    assert len(keys) == 64
    idx = dcn.Index.from_keys(keys, K, 1)
    for record, want in ((many, {"records": 1, "keys": 64, "anchors": 0, "repeats": 64}),
                         (once, {"records": 1, "keys": 64, "anchors": 64, "repeats": 0})):
        amap = dcn.AnchorMap(idx)
        amap.add_records([record])
        assert amap.info() == want
        assert_map(amap, AnchorModel(oracle, K, 1, keys).add([record]))
        got = place(dcn, amap, [unit + unit], oracle, min_votes=1)
        assert got["n_positions"][0] == 98 and got["n_anchors"][0] == (0 if record is many else 98)
        amap.close()
    idx.close()


def run_worker(case, **env):
    p = subprocess.run([sys.executable, WORKER, case], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout


def test_tile_seams():
    out = run_worker("seams", DCN_TILE_WINDOWS="16")
    assert "place seams w=15" in out and "place seams w=1:" in out


def test_path_switch():
    assert "place switch ok" in run_worker("switch", DCN_PLACE_LANE_BASES="100")


def test_partitions():
    assert "place partitions ok" in run_worker("partitions", DCN_PLACE_LDS_CELLS="16", DCN_PLACE_LANE_BASES="0")


def test_displaced_slots():
    assert "place displaced ok" in run_worker("displaced", DCN_TABLE_SLOTS_PER_KEY="2")

"""The model of tests/test_place_split_abi.py and tests/test_gpu_place_split*.py, and the worker of their subprocess
cases.  Anchors, hits and cells are tests/_place_worker.py's (AnchorModel.cells); place_split() restates the five rules
of "THE DEFINITION OF A SPLIT PLACEMENT" (include/deacon_hip.h) over them:

  rounds     round t takes the best cell over the hits no earlier round took (most votes, then the smallest (R, o, j));
             its hits leave; rounds end when no hit is left or after round t = max_placements
  reported   the rounds t < max_placements with votes >= min_votes
  rival      the most votes of any other computed round whose read interval [min q, max q + k) intersects this one's
  mapq       0 when rival >= votes, else 60 * (votes - rival) // votes

As a program (python tests/_place_split_worker.py CASE) it runs one case in a process of its own, whose environment the
test has set, and exits non-zero with a traceback when a check fails."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import _place_worker as PW  # noqa: E402
from _place_worker import (AnchorModel, build_map, chimera, cut, displaced_map, make_genomes, make_records,  # noqa: E402,F401
                           parity_reads, partitions_of, stitched, switch_reads)
from conftest import mutate, random_reads, revcomp  # noqa: E402

SPLIT_FIELDS = PW.FIELDS + ("rank", "n_placed", "rival_votes", "mapq")


def rounds_of(model, read, W=256, prefix=0, max_placements=4):
    """([(cell, [(q, P)])] of the computed rounds, n_anchors, n_positions)"""
    cells, n_anchors, n_pos = model.cells(read, W, prefix)
    rounds = []
    for _ in range(max_placements + 1):
        cells = {c: hits for c, hits in cells.items() if hits}
        if not cells:
            break
        cell, hits = min(cells.items(), key=lambda c: (-len(c[1]), c[0]))
        rounds.append((cell, hits))
        gone = {q for q, _ in hits}  # (a position is one hit: it leaves both of its cells)
        cells = {c: [h for h in hs if h[0] not in gone] for c, hs in cells.items()}
    return rounds, n_anchors, n_pos


def place_split(model, read, W=256, min_votes=2, prefix=0, max_placements=4):
    """(rows in the order of SPLIT_FIELDS, (n_anchors, n_positions)) of one read"""
    k = model.k
    rounds, n_anchors, n_pos = rounds_of(model, read, W, prefix, max_placements)
    votes = [len(hits) for _, hits in rounds]
    assert all(a >= b for a, b in zip(votes, votes[1:]))  # rule 1: votes never rise
    spans = [(min(q for q, _ in hits), max(q for q, _ in hits) + k) for _, hits in rounds]
    n_placed = sum(1 for t, v in enumerate(votes) if t < max_placements and v >= min_votes)
    rows = []
    for t in range(n_placed):
        (R, o, _), hits = rounds[t]
        Ps = [P for _, P in hits]
        rival = max([votes[u] for u in range(len(rounds))
                     if u != t and max(spans[t][0], spans[u][0]) < min(spans[t][1], spans[u][1])], default=0)
        mapq = 0 if rival >= votes[t] else 60 * (votes[t] - rival) // votes[t]
        rows.append((R, o, votes[t], n_anchors, n_pos, spans[t][0], spans[t][1], min(Ps), max(Ps) + k, t, n_placed, rival, mapq))
    return rows, (n_anchors, n_pos)


def place_split_all(model, reads, **kw):
    """(offsets, rows, read_counts) of a batch"""
    offsets, rows, counts = [0], [], []
    for r in reads:
        rr, c = place_split(model, r, **kw)
        rows += rr
        counts.append(c)
        offsets.append(len(rows))
    return offsets, rows, counts


def split(dcn, amap, reads, O, max_placements=4, capacity=None, **kw):
    b, o = O.concat_reads(reads)
    p = dcn.Placer(amap, max_batch_bases=1 << 20, max_batch_reads=1 << 12, **kw)
    try:
        return p.place_split_batch(b, o, max_placements=max_placements, capacity=capacity)
    finally:
        p.close()


def assert_split(got, want, what=()):
    """(place_offsets, rows, read_counts) of Placer.place_split_batch against place_split_all"""
    po, rows, counts = got
    w_off, w_rows, w_counts = want
    assert po.tolist() == w_off, tuple(what) + ("offsets", [(i, a, b) for i, (a, b) in enumerate(zip(po.tolist(), w_off)) if a != b][:4])
    assert counts.tolist() == [list(c) for c in w_counts], tuple(what) + ("read_counts",)
    assert len(rows) == len(w_rows) and not rows["reserved"].any()
    g = np.stack([rows[f].astype(np.int64) for f in SPLIT_FIELDS], axis=1) if len(rows) else np.zeros((0, len(SPLIT_FIELDS)), np.int64)
    w = np.array(w_rows, np.int64).reshape(len(w_rows), len(SPLIT_FIELDS))
    if not np.array_equal(g, w):
        bad = np.flatnonzero((g != w).any(axis=1))
        raise AssertionError(tuple(what) + (len(bad), [(int(i), g[i].tolist(), w[i].tolist()) for i in bad[:4]]))


def check_split(dcn, O, model, amap, reads, what=(), max_placements=4, **kw):
    got = split(dcn, amap, reads, O, max_placements=max_placements, **kw)
    want = place_split_all(model, reads, W=kw.get("band_bases", 256), min_votes=kw.get("min_votes", 2),
                           prefix=kw.get("prefix_length", 0), max_placements=max_placements)
    assert_split(got, want, tuple(what) + (max_placements,) + tuple(kw.items()))
    return got


# ---- inputs --------------------------------------------------------------------------------------------------------
def split_reads(model, records, W=256):
    """chimeras of two and three parts across records and strands, parts that overlap on the read, 5 % substitutions,
    the stretch held twice and the stretch two records share, and reads that are not placed"""
    rng = np.random.default_rng(951)
    reads = []
    for _ in range(40):
        a, b, c = (cut(rng, records, 60, 220) for _ in range(3))
        reads.append(a + b)
        reads.append(a + revcomp(b))
        reads.append(revcomp(a) + b + c)
        reads.append(mutate(rng, a + revcomp(b) + c, 0.05))
        reads.append(a + b[:int(rng.integers(1, 30))] + c)  # a middle part too short to have a hit of its own
        # parts that overlap on the read: b replaces as many bases of a record as it has, so the stretches before and
        # behind it lie on one diagonal and their cell's interval spans b's
        R, at = int(rng.integers(0, 3)), int(rng.integers(0, 15000))
        reads.append(records[R][at:at + 90] + b + records[R][at + 90 + len(b):at + 200 + len(b)])
        reads.append(revcomp(records[R][at:at + 150] + revcomp(b) + records[R][at + 150 + len(b):at + 210 + len(b)]))
    for _ in range(10):  # parts a few bands apart on one record: several cells of one (record, strand)
        R = int(rng.integers(0, 3))
        at = int(rng.integers(0, 15000))
        reads.append(records[R][at:at + 120] + records[R][at + 700:at + 800] + records[R][at + 2000:at + 2090])
        reads.append(revcomp(records[R][at:at + 120] + records[R][at + 300:at + 400]))
    reads += [records[3][:1700], records[3][300:900], records[4][600:1100], revcomp(records[5][250:650]),
              records[4][650:1050] + records[5][200:700]]
    reads.append(records[0][100:2100] + records[2][7000:9500] + revcomp(records[1][50:1900]))  # the workgroup path
    reads.append(records[0][100:700] + records[2][7000:7400] + records[1][50:600] + records[0][9000:9300] + records[2][100:900])
    reads.append(chimera(model, records, W))
    reads += random_reads(rng, 10, 50, 300)
    reads += [b"", records[2][:30], b"ACGT", b"\n", records[0][500:700] + b"\n",
              records[1][3000:3100] + b"N" * 5 + records[1][3105:3200], b"N" * 80]
    return reads


# ---- subprocess cases ----------------------------------------------------------------------------------------------
def case_seams(O, dcn):
    """tiles of 16 windows: every read of 31 bases or more is cut into several tiles"""
    assert os.environ.get("DCN_TILE_WINDOWS") == "16"
    records = make_records(make_genomes())
    for w in (15, 1):
        model, amap = build_map(O, dcn, records, 31, w)
        reads = split_reads(model, records) + parity_reads(model, records)[:200]
        po, _, _ = check_split(dcn, O, model, amap, reads, ("seams", w))
        assert int((np.diff(po.astype(np.int64)) >= 2).sum()) > 100
        amap.close()
    print("place split seams ok")


def case_switch(O, dcn):
    """the same reads with DCN_PLACE_LANE_BASES = 100 (most take the workgroup path) agree with the model, which is what
    the default switch is checked against by the parity test: equal results on both sides"""
    lane = int(os.environ["DCN_PLACE_LANE_BASES"])
    records = make_records(make_genomes())
    for w in (1, 15):
        model, amap = build_map(O, dcn, records, 31, w)
        reads = switch_reads(records, lane) + split_reads(model, records)
        reads += [records[1][3000:3000 + lane - 30] + records[0][40:70], records[1][3000:3000 + lane - 29] + records[0][40:70]]
        for W in (1, 256):
            for n in (1, 8):
                check_split(dcn, O, model, amap, reads, ("switch", w), max_placements=n, band_bases=W)
        amap.close()
    print("place split switch ok")


def case_partitions(O, dcn):
    """DCN_PLACE_LDS_CELLS = 16 and DCN_PLACE_LANE_BASES = 0: every read takes the workgroup path and a stitched read
    has far more cells than the set has slots.  The partition of a cell is replayed (partitions_of): reads[0] is searched
    for a stitching whose ROUND-1 winner lies in the last partition of the count that round 0 arrived at (the count
    carries over; since the hits of a round are a subset of the round before, no later round can need more partitions
    than an earlier one, so a count that doubles in a later round only does not exist -- reads[1] is the nearest thing:
    round 0 needs 16 partitions or more, and its later rounds, with fewer cells, run at that count)"""
    assert os.environ.get("DCN_PLACE_LDS_CELLS") == "16" and os.environ.get("DCN_PLACE_LANE_BASES") == "0"
    records = make_records(make_genomes())
    model, amap = build_map(O, dcn, records, 31, 1)
    found = None
    for seed in range(400):
        read = stitched(np.random.default_rng(2000 + seed), records, 60)
        rounds = rounds_of(model, read, 1, 0, 4)[0]
        parts, where = partitions_of(model.cells(read, 1)[0], 16)
        if parts >= 8 and len(rounds) > 1 and where[rounds[1][0]] == parts - 1:
            found = read
            break
    assert found is not None
    rng = np.random.default_rng(952)
    reads = [found, stitched(rng, records, 200),
             stitched(rng, records, 30) + records[1][4000:4050] + stitched(rng, records, 30) + records[0][8000:8050],
             records[0][100:160], b"", records[1][:30]] + split_reads(model, records)
    assert partitions_of(model.cells(reads[1], 1)[0], 16)[0] >= 16
    for W in (1, 64):
        for n in (2, 8):
            check_split(dcn, O, model, amap, reads, ("partitions",), max_placements=n, band_bases=W)
    amap.close()
    print("place split partitions ok")


def case_displaced(O, dcn):
    """a map whose anchors sit in displaced slots and behind the wrap of the last group (displaced_map): every record as a
    read on both strands, and pairs of records stitched into reads of two placements of one vote each"""
    assert os.environ.get("DCN_TABLE_SLOTS_PER_KEY") == "2"
    k, w, G, S, keys, records, model, amap, absent = displaced_map(O, dcn)
    reads = records + [revcomp(r) for r in records] + absent
    reads += [records[i] + b"N" + revcomp(records[i + 1]) for i in range(1, len(records) - 2, 2)]
    po, rows, _ = check_split(dcn, O, model, amap, reads, ("displaced",), min_votes=1)
    assert int((np.diff(po.astype(np.int64)) == 2).sum()) >= 10
    amap.close()
    print("place split displaced ok")


if __name__ == "__main__":
    import deacon_server_amd as dcn
    from oracle import oracle as O
    O.lib()
    {"seams": case_seams, "switch": case_switch, "partitions": case_partitions, "displaced": case_displaced}[sys.argv[1]](O, dcn)

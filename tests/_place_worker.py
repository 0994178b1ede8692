"""The model of tests/test_place_abi.py and tests/test_gpu_place*.py, and the worker of their subprocess cases.

Model (the statements of include/deacon_hip.h as short functions over oracle.minimizer_hashes_and_positions and plain
dicts).  AnchorModel holds, per key of a key set, nothing (unseen), the one (record, position) that has its hash, or
REPEAT.  place() votes: a read's distinct positions whose hash is an anchor are its anchor hits; the orientation of a
hit is '+' when the read's k-mer and the record's k-mer are the same text (upper-cased), else '-'; D = P - q + len or
P + q; the hit votes for cells (R, o, D // W) and (R, o, D // W + 1); the best cell has the most votes, ties to the
smallest (R, o, j) with '+' before '-'.  Integers only.

As a program (python tests/_place_worker.py CASE) it runs one case in a process of its own, whose environment the test
has set (DCN_TILE_WINDOWS, DCN_PLACE_LANE_BASES, DCN_PLACE_LDS_CELLS, DCN_TABLE_SLOTS_PER_KEY), and exits non-zero with a
traceback when a check fails."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
from conftest import mutate, random_reads, revcomp  # noqa: E402

REPEAT = "repeat"
UNPLACED = 0xFFFFFFFF
FIELDS = ("record", "reverse", "votes", "n_anchors", "n_positions", "read_start", "read_end", "ref_start", "ref_end")


def occurrences(O, seq, k, w, prefix=0):
    """[(hash, position)] of the distinct positions of a sequence, ascending by position"""
    h, p = O.minimizer_hashes_and_positions(seq, k, w, prefix)
    if not len(p):
        return []
    up, first = np.unique(p, return_index=True)  # a position the list repeats counts once
    return list(zip(np.asarray(h, np.uint64)[first].tolist(), up.tolist()))


class AnchorModel:
    def __init__(self, O, k, w, keys):
        self.O, self.k, self.w = O, k, w
        self.keys = set(keys.tolist() if isinstance(keys, np.ndarray) else keys)
        self.state = {}  # key -> (record, position) | REPEAT
        self.records = []

    def add(self, records):
        for rec in records:
            R = len(self.records)
            self.records.append(bytes(rec))
            for h, P in occurrences(self.O, rec, self.k, self.w):
                if h not in self.keys:
                    continue
                old = self.state.get(h)
                if old is None:
                    self.state[h] = (R, P)
                elif old != (R, P):
                    self.state[h] = REPEAT
        return self

    def anchors(self):
        return {h: v for h, v in self.state.items() if v != REPEAT}

    def info(self):
        a = len(self.anchors())
        return {"records": len(self.records), "keys": len(self.keys), "anchors": a, "repeats": len(self.state) - a}

    def cells(self, read, W=256, prefix=0):
        """({(R, o, j): [(q, P)]}, n_anchors, n_positions) of one read"""
        k, ln = self.k, len(read)
        occ = occurrences(self.O, read, k, self.w, prefix)
        cells, n_anchors = {}, 0
        text = bytes(read).upper()
        for h, q in occ:
            at = self.state.get(h)
            if at is None or at == REPEAT:
                continue
            n_anchors += 1
            R, P = at
            same = text[q:q + k] == self.records[R][P:P + k].upper()
            o = 0 if same else 1
            D = P - q + ln if same else P + q
            assert D >= 0
            for j in (D // W, D // W + 1):
                cells.setdefault((R, o, j), []).append((q, P))
        return cells, n_anchors, len(occ)

    def place(self, read, W=256, min_votes=2, prefix=0):
        """the placement of one read as a tuple in the order of FIELDS"""
        cells, n_anchors, n_pos = self.cells(read, W, prefix)
        if cells:
            (R, o, j), hits = min(cells.items(), key=lambda c: (-len(c[1]), c[0]))
            if len(hits) >= min_votes:
                qs, Ps = [q for q, _ in hits], [P for _, P in hits]
                return (R, o, len(hits), n_anchors, n_pos, min(qs), max(qs) + self.k, min(Ps), max(Ps) + self.k)
        return (UNPLACED, 0, 0, n_anchors, n_pos, 0, 0, 0, 0)

    def place_all(self, reads, **kw):
        return [self.place(r, **kw) for r in reads]


def assert_placements(got, want, what=()):
    """the structured array of Placer.place_batch against AnchorModel.place_all"""
    assert len(got) == len(want), ("n",) + tuple(what)
    assert not got["reserved"].any()
    g = np.stack([got[f].astype(np.int64) for f in FIELDS], axis=1) if len(got) else np.zeros((0, len(FIELDS)), np.int64)
    w = np.array(want, np.int64).reshape(len(want), len(FIELDS))
    if not np.array_equal(g, w):
        bad = np.flatnonzero((g != w).any(axis=1))
        raise AssertionError(tuple(what) + (len(bad), [(int(i), g[i].tolist(), w[i].tolist()) for i in bad[:4]]))


def assert_map(amap, model, what=()):
    """info() and anchors() of an AnchorMap against the model"""
    assert amap.info() == model.info(), tuple(what) + (amap.info(), model.info())
    keys, rec, pos = amap.anchors()
    got = {int(h): (int(r), int(p)) for h, r, p in zip(keys, rec, pos)}
    assert len(got) == len(keys) and got == model.anchors(), tuple(what) + ("anchors",)


# ---- inputs --------------------------------------------------------------------------------------------------------
def make_genomes():
    return random_reads(np.random.default_rng(911), 3, 20_000, 20_000)


def make_records(genomes):
    """the three genomes, a record that holds a 200-base stretch twice (its keys there are repeats), and two records
    that share a stretch of 300 bases (repeats across records)"""
    rng = np.random.default_rng(912)
    a, b, c, d = random_reads(rng, 4, 1500, 1500)
    twice = a[:600] + a[200:400] + a[600:]
    shared = random_reads(rng, 1, 300, 300)[0]
    return list(genomes) + [twice, b[:700] + shared + b[700:], c[:300] + shared + c[300:]]


def cut(rng, records, lo, hi, R=None):
    R = int(rng.integers(0, len(records))) if R is None else R
    ln = int(rng.integers(lo, hi + 1))
    at = int(rng.integers(0, len(records[R]) - ln + 1))
    return records[R][at:at + ln]


def chimera(model, records, W, first=1, second=0):
    """a read of two error-free halves, the first from record `first` and the second from the smaller record `second`,
    whose best cells tie in votes: the second half grows base by base until the model's cells say so"""
    head = records[first][5000:5150]
    for ln in range(60, 600):
        read = head + records[second][9000:9000 + ln]
        cells = model.cells(read, W)[0]
        top = {R: max([len(v) for (r, _, _), v in cells.items() if r == R], default=0) for R in (first, second)}
        if top[first] == top[second] >= 2 and max(len(v) for v in cells.values()) == top[first]:
            return read
    raise AssertionError("no tie found")


def parity_reads(model, records, W=256):
    rng = np.random.default_rng(913)
    reads = []
    for _ in range(150):
        reads.append(cut(rng, records, 40, 400))
        reads.append(revcomp(cut(rng, records, 40, 400)))
        reads.append(mutate(rng, cut(rng, records, 80, 400), 0.05))
        reads.append(revcomp(mutate(rng, cut(rng, records, 80, 400), 0.05)))
    for _ in range(40):
        s = cut(rng, records, 200, 400)
        i, j = sorted(rng.integers(20, len(s) - 20, 2).tolist())
        reads.append(s[:i] + b"G" + s[i:j] + s[j + 1:])  # an inserted and a deleted base
        s = bytearray(cut(rng, records, 200, 400))
        at = int(rng.integers(0, len(s) - 12))
        s[at:at + int(rng.integers(1, 12))] = b"N" * 11
        reads.append(bytes(s[:len(s)]))
        reads.append(cut(rng, records, 100, 300).lower())
        low = bytearray(cut(rng, records, 100, 300))
        low[30:90] = bytes(low[30:90]).lower()
        reads.append(bytes(low))
    reads += [records[0][500:700] + b"\n", revcomp(records[1][100:140]) + b"\n", records[2][:30], b"", b"ACGT", b"\n",
              records[3][:1700], records[4][600:1100], revcomp(records[5][250:650])]
    for ln, R in ((3000, 0), (5200, 1), (9000, 2)):  # reads of the workgroup path
        reads.append(cut(rng, records, ln, ln, R))
        reads.append(revcomp(mutate(rng, cut(rng, records, ln, ln, R), 0.03)))
    reads.append(records[0][100:2100] + records[2][7000:9500])  # a long chimera
    reads.append(chimera(model, records, W))
    reads += random_reads(rng, 20, 50, 300)
    return reads


def build_map(O, dcn, records, k, w, keys=None):
    """(model, AnchorMap) over the records' own keys (or `keys`), every record added in one call"""
    if keys is None:
        keys = O.Index.build(records, k=k, w=w).keys()
    model = AnchorModel(O, k, w, keys).add(records)
    idx = dcn.Index.from_keys(np.asarray(sorted(model.keys), np.uint64), k, w)
    amap = dcn.AnchorMap(idx)
    idx.close()
    amap.add_records(records)
    return model, amap


def place(dcn, amap, reads, O, **kw):
    b, o = O.concat_reads(reads)
    p = dcn.Placer(amap, max_batch_bases=1 << 20, max_batch_reads=1 << 12, **kw)
    try:
        return p.place_batch(b, o)
    finally:
        p.close()


# ---- subprocess cases ----------------------------------------------------------------------------------------------
def case_seams(O, dcn):
    """the parity batch with tiles of 16 windows (every read of 31 bases or more is cut into several tiles, each seam a
    carry window), at w = 15 and at w = 1: a position emitted on both sides of a seam is one vote, and in add one
    occurrence, not a repeat"""
    assert os.environ.get("DCN_TILE_WINDOWS") == "16"
    records = make_records(make_genomes())
    for w in (15, 1):
        model, amap = build_map(O, dcn, records, 31, w)
        assert_map(amap, model, ("seams", w))
        reads = parity_reads(model, records)
        got = place(dcn, amap, reads, O)
        assert_placements(got, model.place_all(reads), ("seams", w))
        assert int((got["record"] != UNPLACED).sum()) > 500
        amap.close()
        print(f"place seams w={w}: {model.info()}")


def switch_reads(records, lane):
    """reads of lane - 1, lane and lane + 1 bases on both strands, between short ones"""
    reads = []
    for ln in (lane - 1, lane, lane + 1):
        reads += [records[0][40:120], records[1][3000:3000 + ln], revcomp(records[2][777:777 + ln]), records[1][50:90]]
    return reads


def case_switch(O, dcn):
    """both sides of the path switch with DCN_PLACE_LANE_BASES = 100: the lane path and the workgroup path agree with
    the model, at w = 1 (about 70 hits a read) and w = 15"""
    lane = int(os.environ["DCN_PLACE_LANE_BASES"])
    records = make_records(make_genomes())
    for w in (1, 15):
        model, amap = build_map(O, dcn, records, 31, w)
        reads = switch_reads(records, lane) + parity_reads(model, records)
        for W in (1, 256):
            assert_placements(place(dcn, amap, reads, O, band_bases=W), model.place_all(reads, W=W), ("switch", w, W))
        amap.close()
    print("place switch ok")


def stitched(rng, records, n, R=None):
    """a read stitched from n 40-base cuts of scattered places"""
    return b"".join(cut(rng, records, 40, 40, R) for _ in range(n))


_M64 = (1 << 64) - 1


def plc_mix(x):
    """place.hip's mix of a cell key"""
    x ^= x >> 33
    x = x * 0xFF51AFD7ED558CCD & _M64
    x ^= x >> 33
    x = x * 0xC4CEB9FE1A85EC53 & _M64
    return x ^ (x >> 33)


def partitions_of(cells, slots):
    """what place_big_kernel does with a read's cells and an LDS set of `slots` slots: the set is keyed by (record, j) --
    the two orientations share a slot -- and the partition count doubles until no partition holds more distinct keys than
    the set has slots.  -> (partition count, {cell: its partition})"""
    keys = {c: ((c[0] + 1) << 33) | c[2] for c in cells}
    parts = 1
    while True:
        load = {}
        for key in set(keys.values()):
            load[plc_mix(key) & (parts - 1)] = load.get(plc_mix(key) & (parts - 1), 0) + 1
        if max(load.values(), default=0) <= slots:
            return parts, {c: plc_mix(key) & (parts - 1) for c, key in keys.items()}
        parts *= 2


def case_partitions(O, dcn):
    """DCN_PLACE_LDS_CELLS = 16 and DCN_PLACE_LANE_BASES = 0: every read takes the workgroup path, and a read stitched
    from scattered 40-base cuts has far more distinct cells than the set has slots (w = 1: ten hits per cut, two cells
    each).  Which partition a cell falls into is place.hip's mix of its key, replayed here (partitions_of), and the two
    cases the construction is for are asserted, not hoped for: in reads[0] at W = 1 the winning cell lies in the LAST
    of 16 partitions; in reads[3] two cuts of 50 bases tie at 20 votes in cells of different partitions, and the smaller
    cell wins whichever partition is swept first"""
    assert os.environ.get("DCN_PLACE_LDS_CELLS") == "16" and os.environ.get("DCN_PLACE_LANE_BASES") == "0"
    rng = np.random.default_rng(915)
    records = make_records(make_genomes())
    model, amap = build_map(O, dcn, records, 31, 1)
    reads = [stitched(rng, records, 60), stitched(rng, records, 200),
             stitched(rng, records, 80) + records[2][15000:15080],
             stitched(rng, records, 30) + records[1][4000:4050] + stitched(rng, records, 30) + records[0][8000:8050] +
             stitched(rng, records, 10),
             records[0][100:160], b"", records[1][:30]] + parity_reads(model, records)[:200]
    for W in (1, 64):
        want = model.place_all(reads, W=W)
        if W == 1:
            # the long last cut wins; of the two cuts of 50 bases that tie, the one on the smaller record
            assert want[2][:3] == (2, 0, 50) and want[3][:3] == (0, 0, 20) and want[3][7] == 8000
            # reads[0]: the winner is met only in the last partition
            cells = model.cells(reads[0], W)[0]
            parts, where = partitions_of(cells, 16)
            best = min(cells.items(), key=lambda c: (-len(c[1]), c[0]))[0]
            assert len({(c[0], c[2]) for c in cells}) > 6 * 16 and parts == 16 and where[best] == parts - 1, (parts, where[best])
            # reads[3]: cells of equal (top) votes in more than one partition
            cells = model.cells(reads[3], W)[0]
            parts, where = partitions_of(cells, 16)
            top = max(len(v) for v in cells.values())
            tied = {where[c] for c, v in cells.items() if len(v) == top}
            assert top == 20 and parts >= 8 and len(tied) >= 3, (parts, sorted(tied))
        assert_placements(place(dcn, amap, reads, O, band_bases=W), want, ("partitions", W))
    amap.close()
    print("place partitions ok")


def displaced_map(O, dcn):
    """A map over a table of G groups built under DCN_TABLE_SLOTS_PER_KEY = 2, in which the chains of the last group wrap
    to group 0 and every key on them is an anchor with a record of its own.  Keys and records come from the pool of
    single-window reads of tests/test_gpu_classify_seams.py (k + w - 1 bases, one minimizer each).  Groups G - 1, 0 and 1
    each are the home of 3 * S + 2 keys of the map (S slots a group): whichever S of them the build leaves in group
    G - 1, at least 2 * S + 2 keys homed there sit in group 0 or later, behind the keys homed in groups 0 and 1.  The same
    is done at G - 5 and at a few groups inside the table.  One record is added twice (a repeat on a wrapped chain), two
    reads homed at G - 1 are in no record's key set (their lookups walk the wrapped chain and find nothing), and random
    keys fill the table to half.
    -> (k, w, G, S, keys, records, model, map, extra reads)"""
    from test_classify_replicas import group_of
    from test_gpu_classify_seams import W as WIN
    from test_gpu_classify_seams import Pool, group_slots
    k, S = 31, group_slots()
    G = 2048 // S
    per = 3 * S + 2
    pool = Pool(O, k, 24_000, 7)
    homes = [G - 1, 0, 1, G - 5, G - 4] + list(range(40, G - 40, 97))
    records, keys = [], set()
    for g in homes:
        for r, h in pool.take(per, lambda hs, g=g: group_of(hs, G) == np.uint64(g)):
            records.append(r)
            keys.add(h)
    absent = [r for r, _ in pool.take(2, lambda hs: group_of(hs, G) == np.uint64(G - 1))]
    records.append(records[0])  # the first key homed at G - 1 occurs in two records: a repeat
    rng = np.random.default_rng(916)
    while len(keys) < 980:
        keys.add(int(rng.integers(1, 2**63)))
    keys = np.array(sorted(keys), np.uint64)
    model = AnchorModel(O, k, WIN, keys).add(records)
    idx = dcn.Index.from_keys(keys, k, WIN)
    assert idx.table_bytes == G * S * 8, (idx.table_bytes, G, S)  # the table the construction was made for
    amap = dcn.AnchorMap(idx)
    idx.close()
    amap.add_records(records)
    return k, WIN, G, S, keys, records, model, amap, absent


def case_displaced(O, dcn):
    """anchors(), info() and the placements of a map whose anchors sit in second slots, in displaced groups and in
    group 0 and later after the last group (displaced_map), and the ordinary map of the parity records over a half-full
    table"""
    assert os.environ.get("DCN_TABLE_SLOTS_PER_KEY") == "2"
    from test_classify_replicas import group_of
    k, w, G, S, keys, records, model, amap, absent = displaced_map(O, dcn)
    # the construction reached the wrap: more keys homed in the last group than two groups hold, all but the repeat of
    # them anchors, and groups 0 and 1 full of their own
    home = group_of(keys, G)
    anchors = model.anchors()
    last = [int(h) for h in keys[home == np.uint64(G - 1)].tolist()]
    assert len(last) >= 3 * S + 2 and sum(h in anchors for h in last) >= 3 * S + 1
    assert sum(model.state.get(h) == REPEAT for h in last) == 1
    for g in (0, 1):
        assert int((home == np.uint64(g)).sum()) >= 3 * S + 2
    assert model.info()["repeats"] == 1 and model.info()["anchors"] == len(records) - 2
    assert_map(amap, model, ("displaced", "wrap"))
    got_keys, got_rec, _ = amap.anchors()
    at = dict(zip(got_keys.tolist(), got_rec.tolist()))
    assert all(at[h] == anchors[h][0] for h in last if h in anchors)
    # every record as a read, on both strands, and the two reads whose key the map does not hold
    reads = records + [revcomp(r) for r in records] + absent
    want = model.place_all(reads, min_votes=1)
    got = place(dcn, amap, reads, O, min_votes=1)
    assert_placements(got, want, ("displaced", "wrap"))
    n = len(records)
    assert got["record"][1:n - 1].tolist() == list(range(1, n - 1)) and (got["votes"][1:n - 1] == 1).all()
    assert got["record"][n + 1:2 * n - 1].tolist() == list(range(1, n - 1)) and (got["reverse"][n + 1:2 * n - 1] == 1).all()
    assert got["record"][[0, n - 1, 2 * n, 2 * n + 1]].tolist() == [UNPLACED] * 4  # the repeat, and the absent keys
    amap.close()
    records = make_records(make_genomes())
    model, amap = build_map(O, dcn, records, 31, 1)
    assert_map(amap, model, ("displaced",))
    reads = parity_reads(model, records)
    assert_placements(place(dcn, amap, reads, O), model.place_all(reads), ("displaced",))
    amap.close()
    print("place displaced ok", model.info())


if __name__ == "__main__":
    import deacon_server_amd as dcn
    from oracle import oracle as O
    O.lib()
    {"seams": case_seams, "switch": case_switch, "partitions": case_partitions, "displaced": case_displaced}[sys.argv[1]](O, dcn)

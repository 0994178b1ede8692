"""The model of tests/test_place_pair_abi.py and tests/test_gpu_place_pair*.py, and the worker of their subprocess cases.
Rounds are tests/_place_split_worker.py's (rounds_of); place_pair() restates "THE DEFINITION OF A PAIRED PLACEMENT"
(include/deacon_hip.h) over them:

  candidates  a mate's computed rounds t < max_placements, whatever their votes
  concordant  same record, opposite orientations ('+' round F, '-' round V), F.ref_start < V.ref_end,
              T = max(ref_end) - min(ref_start) <= max_insert, max(votes) >= min_votes
  chosen      the concordant combination with the most votes_a + votes_b, then the smallest a, then the smallest b: the
              pair is PROPER and reports rounds a, b; else each mate reports round 0 with votes >= min_votes, or nothing
  pv(t)       votes_t + the most votes of a candidate of the other mate concordant with t (0 for t = max_placements)
  rival       the largest pv(u) over the same mate's other computed rounds whose read interval intersects t's
  mapq        0 when rival >= pv(t), else 60 * (pv(t) - rival) // pv(t)

As a program (python tests/_place_pair_worker.py CASE) it runs one case in a process of its own, whose environment the
test has set, and exits non-zero with a traceback when a check fails."""
import os
import sys
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import _place_split_worker as SW  # noqa: E402
from _place_split_worker import build_map, make_genomes, make_records, rounds_of  # noqa: E402,F401
from conftest import mutate, random_reads, revcomp  # noqa: E402

PAIR_FIELDS = SW.SPLIT_FIELDS + ("flags", "pair_votes", "tlen")
F = {f: i for i, f in enumerate(PAIR_FIELDS)}
PROPER, RESCUED, MATE_PLACED = 1, 2, 4
UNPLACED = 0xFFFFFFFF
HIST_BINS = 256

Round = namedtuple("Round", "R o votes q0 q1 p0 p1")  # read interval [q0, q1), reference extent [p0, p1)


def mate_rounds(model, read, W=256, prefix=0, N=4):
    """([Round] of the computed rounds 0 .. N, n_anchors, n_positions)"""
    k = model.k
    rounds, n_anchors, n_pos = rounds_of(model, read, W, prefix, N)
    out = []
    for (R, o, _), hits in rounds:
        qs, Ps = [q for q, _ in hits], [P for _, P in hits]
        out.append(Round(R, o, len(hits), min(qs), max(qs) + k, min(Ps), max(Ps) + k))
    return out, n_anchors, n_pos


def template(x, y, I, min_votes):
    """T of two rounds when they are concordant (rule 2), else None"""
    if x.R != y.R or x.o == y.o or max(x.votes, y.votes) < min_votes:
        return None
    fwd, rev = (x, y) if x.o == 0 else (y, x)
    if not fwd.p0 < rev.p1:
        return None
    T = max(fwd.p1, rev.p1) - min(fwd.p0, rev.p0)
    return T if T <= I else None


def place_pair(model, read1, read2, W=256, min_votes=2, prefix=0, max_placements=4, max_insert=1000):
    """(row of mate 1, row of mate 2, T or None) in the order of PAIR_FIELDS"""
    N, I = max_placements, max_insert
    mates = [mate_rounds(model, r, W, prefix, N) for r in (read1, read2)]
    rs = [m[0] for m in mates]
    cand = [r[:N] for r in rs]
    combos = [(-(x.votes + y.votes), a, b) for a, x in enumerate(cand[0]) for b, y in enumerate(cand[1])
              if template(x, y, I, min_votes) is not None]
    chosen = min(combos)[1:] if combos else None

    def pv(m, t):
        me = rs[m][t]
        if t >= N:
            return me.votes
        return me.votes + max([y.votes for y in cand[1 - m] if template(me, y, I, min_votes) is not None], default=0)

    T = template(cand[0][chosen[0]], cand[1][chosen[1]], I, min_votes) if chosen else None
    reported = []
    for m in (0, 1):
        if chosen:
            reported.append(chosen[m])
        else:
            reported.append(0 if rs[m] and rs[m][0].votes >= min_votes else None)
    rows = []
    for m in (0, 1):
        _, n_anchors, n_pos = mates[m]
        t = reported[m]
        if t is None:
            rows.append((UNPLACED, 0, 0, n_anchors, n_pos) + (0,) * (len(PAIR_FIELDS) - 5))
            continue
        me = rs[m][t]
        n_placed = sum(1 for u, x in enumerate(rs[m]) if u < N and x.votes >= min_votes)
        rival = max([pv(m, u) for u, x in enumerate(rs[m]) if u != t and max(me.q0, x.q0) < min(me.q1, x.q1)], default=0)
        mine = pv(m, t)
        mapq = 0 if rival >= mine else 60 * (mine - rival) // mine
        flags, tlen = 0, 0
        if chosen:
            flags = PROPER | MATE_PLACED | (RESCUED if me.votes < min_votes else 0)
            other = rs[1 - m][reported[1 - m]]
            first = me.p0 < other.p0 or (me.p0 == other.p0 and m == 0)
            tlen = T if first else -T
        elif reported[1 - m] is not None:
            flags = MATE_PLACED
        rows.append((me.R, me.o, me.votes, n_anchors, n_pos, me.q0, me.q1, me.p0, me.p1, t, n_placed, rival, mapq, flags, mine, tlen))
    return rows[0], rows[1], T


def place_pair_all(model, reads, hist_bin_bases=8, **kw):
    """(rows of the interleaved batch, the 256-bin histogram); a pair that the batch repeats is computed once"""
    assert len(reads) % 2 == 0
    rows, hist, memo = [], [0] * HIST_BINS, {}
    for u in range(len(reads) // 2):
        key = (reads[2 * u], reads[2 * u + 1])
        if key not in memo:
            memo[key] = place_pair(model, key[0], key[1], **kw)
        a, b, T = memo[key]
        rows += [a, b]
        if T is not None:
            hist[min(T // hist_bin_bases, HIST_BINS - 1)] += 1
    return rows, hist


def assert_pairs(got, want, what=()):
    """(rows, hist) of Placer.place_pair_batch against place_pair_all; hist None on either side is not compared"""
    rows, hist = got
    w_rows, w_hist = want
    assert len(rows) == len(w_rows) and rows.dtype.itemsize == 80 and not rows["reserved"].any(), tuple(what)
    g = np.stack([rows[f].astype(np.int64) for f in PAIR_FIELDS], axis=1) if len(rows) else np.zeros((0, len(PAIR_FIELDS)), np.int64)
    w = np.array(w_rows, np.int64).reshape(len(w_rows), len(PAIR_FIELDS))
    if not np.array_equal(g, w):
        bad = np.flatnonzero((g != w).any(axis=1))
        raise AssertionError(tuple(what) + (len(bad), [(int(i), g[i].tolist(), w[i].tolist()) for i in bad[:4]]))
    if hist is not None and w_hist is not None:
        assert hist.tolist() == list(w_hist), tuple(what) + ("hist",)


def model_kw(kw):
    """the model's names of Placer / place_pair_batch keywords"""
    out = {"W": kw.get("band_bases", 256), "min_votes": kw.get("min_votes", 2), "prefix": kw.get("prefix_length", 0)}
    for name in ("max_placements", "max_insert", "hist_bin_bases"):
        if name in kw:
            out[name] = kw[name]
    return out


def check_pairs(dcn, O, model, amap, reads, what=(), **kw):
    """a Placer of its own over `amap`: place_pair_batch against the model; -> (rows, hist, the model's rows)"""
    ctx = {n: kw[n] for n in ("band_bases", "min_votes", "prefix_length") if n in kw}
    call = {n: kw[n] for n in ("max_placements", "max_insert", "hist_bin_bases") if n in kw}
    b, o = O.concat_reads(reads)
    p = dcn.Placer(amap, max_batch_bases=1 << 20, max_batch_reads=1 << 12, **ctx)
    try:
        got = p.place_pair_batch(b, o, **call)
    finally:
        p.close()
    want = place_pair_all(model, reads, **model_kw(kw))
    assert_pairs(got, want, tuple(what) + tuple(kw.items()))
    return got[0], got[1], want[0]


# ---- inputs --------------------------------------------------------------------------------------------------------
def mates_of(frag, L1, L2, flip=False):
    """an FR pair of a fragment: mate 1 its first L1 bases, mate 2 the reverse complement of its last L2; flip: as given
    the other way round (mate 1 on the reverse strand)"""
    a, b = frag[:L1], revcomp(frag[len(frag) - L2:])
    return (b, a) if flip else (a, b)


def fragment(rng, records, lo, hi, R=None):
    R = int(rng.integers(0, 3)) if R is None else R
    ln = int(rng.integers(lo, hi + 1))
    at = int(rng.integers(0, len(records[R]) - ln + 1))
    return R, at, records[R][at:at + ln]


def mosaic(records, at, seg=45, A=0, B=1):
    """a read of four segments that alternate between record A and record B at the same offset from `at`: two cells on
    overlapping stretches of the read (at w = 1 with 2 * (seg - k + 1) votes each)"""
    a, b = records[A][at:at + 4 * seg], records[B][at:at + 4 * seg]
    return a[:seg] + b[seg:2 * seg] + a[2 * seg:3 * seg] + b[3 * seg:]


def pair_reads(model, records, I=1000):
    """[(kind, mate 1, mate 2)]: every kind of pair the parity test names.  kinds_hold() asserts on the model that each
    kind is what its name says"""
    rng = np.random.default_rng(971)
    k, w = model.k, model.w
    one = k + w - 1  # a mate of one window: one position
    out = []
    for i in range(30):
        _, _, f = fragment(rng, records, 250, 600)
        L1, L2 = int(rng.integers(80, 151)), int(rng.integers(80, 151))
        out.append(("fr", *mates_of(f, L1, L2)))
        out.append(("rf_given", *mates_of(f, L1, L2, flip=True)))
        m1, m2 = mates_of(f, 150, 150, flip=bool(i % 2))
        out.append(("subst", mutate(rng, m1, 0.05), mutate(rng, m2, 0.05)))
    for i in range(8):
        _, _, f = fragment(rng, records, 300, 600, R=0)
        _, _, g = fragment(rng, records, 300, 600, R=1 + i % 2)
        out.append(("records", f[:120], revcomp(g[-120:])))
        out.append(("same_strand", f[:120], f[-120:]))
        out.append(("outie", revcomp(f[:120]), f[-120:]))
        _, _, long_ = fragment(rng, records, I + 1, I + 400)
        out.append(("long", *mates_of(long_, 120, 120, flip=bool(i % 2))))
        _, _, f = fragment(rng, records, 300, 600)
        out.append(("one_hit_inside", *mates_of(f, 130, one, flip=bool(i % 2))))
        out.append(("one_hit_outside", *mates_of(long_, 130, one, flip=bool(i % 2))))
        out.append(("both_one_hit", *mates_of(f, one, one)))
        out.append(("none", f[:140], random_reads(rng, 1, 100, 150)[0]))
        # a chimeric mate: its stronger part lies elsewhere, its weaker part is the one the partner supports
        _, _, x = fragment(rng, records, 140, 140)
        out.append(("chimeric", x + f[:90], revcomp(f[-120:])))
    _, _, f = fragment(rng, records, 400, 400, R=2)
    out += [("edge", b"", revcomp(f[-100:])), ("edge", f[:100], b"N" * 90), ("edge", f[:20], revcomp(f[-100:])),
            ("edge", f[:100] + b"\n", revcomp(f[-100:]) + b"\n"), ("edge", b"\n", b""), ("edge", b"ACGT", f[:100]),
            ("edge", f[:60] + b"N" * 3 + f[63:140], revcomp(f[-100:]))]
    # two equal-vote cells on one stretch of mate 1 (a mosaic of records 0 and 1); the partner supports the first (record
    # 0, which wins the tie alone) or the second (record 1: the rank-1 round is reported)
    found = 0
    for at in range(2000, 18000, 137):
        m1 = mosaic(records, at)
        rs = mate_rounds(model, m1)[0]
        if len(rs) < 2 or rs[0].votes != rs[1].votes or rs[0].votes < 2 or {rs[0].R, rs[1].R} != {0, 1}:
            continue
        if not max(rs[0].q0, rs[1].q0) < min(rs[0].q1, rs[1].q1):
            continue
        for R in (0, 1):
            out.append(("tie_%d" % R, m1, revcomp(records[R][at + 300:at + 420])))
        found += 1
        if found == 3:
            break
    return out


def kinds_hold(model, pairs, I=1000, **kw):
    """asserts, on the model alone, that the batch holds at least one pair of each kind and that each is what its name
    says.  -> the model's rows"""
    reads = [m for _, a, b in pairs for m in (a, b)]
    rows, _ = place_pair_all(model, reads, max_insert=I, **kw)
    seen = {}
    for u, (kind, m1, m2) in enumerate(pairs):
        a, b = rows[2 * u], rows[2 * u + 1]
        proper = bool(a[F["flags"]] & PROPER)
        assert proper == bool(b[F["flags"]] & PROPER)
        ok = None
        if kind in ("fr", "rf_given"):
            ok = proper and a[F["reverse"]] == (1 if kind == "rf_given" else 0) and b[F["reverse"]] == 1 - a[F["reverse"]]
            ok = ok and a[F["pair_votes"]] == b[F["pair_votes"]] == a[F["votes"]] + b[F["votes"]] and a[F["tlen"]] == -b[F["tlen"]] != 0
        elif kind == "subst":
            ok = True  # (whatever the substitutions leave: counted below)
        elif kind in ("records", "same_strand", "outie", "long"):
            ok = not proper and a[F["record"]] != UNPLACED and b[F["record"]] != UNPLACED
            ok = ok and a[F["flags"]] == b[F["flags"]] == MATE_PLACED and a[F["tlen"]] == 0
            if kind == "records":
                ok = ok and a[F["record"]] != b[F["record"]]
            elif kind == "same_strand":
                ok = ok and a[F["record"]] == b[F["record"]] and a[F["reverse"]] == b[F["reverse"]]
            elif kind == "outie":
                ok = ok and a[F["record"]] == b[F["record"]] and a[F["reverse"]] == 1 and b[F["reverse"]] == 0
            else:
                ok = ok and a[F["record"]] == b[F["record"]] and a[F["reverse"]] != b[F["reverse"]]
        elif kind == "one_hit_inside":
            short = a if a[F["n_anchors"]] == 1 else b
            ok = proper and short[F["votes"]] == 1 and short[F["flags"]] == PROPER | RESCUED | MATE_PLACED and short[F["n_placed"]] == 0
        elif kind == "one_hit_outside":
            short, full = (a, b) if a[F["n_anchors"]] == 1 else (b, a)
            ok = not proper and short[F["n_anchors"]] == 1 and short[F["record"]] == UNPLACED and full[F["record"]] != UNPLACED
            ok = ok and full[F["flags"]] == 0 and short[F["flags"]] == 0
        elif kind == "both_one_hit":
            ok = not proper and a[F["n_anchors"]] == b[F["n_anchors"]] == 1 and a[F["record"]] == b[F["record"]] == UNPLACED
        elif kind == "none":
            ok = not proper and b[F["n_anchors"]] == 0 and b[F["record"]] == UNPLACED and a[F["record"]] != UNPLACED
        elif kind == "chimeric":
            ok = proper and a[F["rank"]] == 1 and b[F["rank"]] == 0
        elif kind == "edge":
            ok = True
        elif kind.startswith("tie_"):
            R = int(kind[-1])
            alone = SW.place_split(model, m1, max_placements=kw.get("max_placements", 4))[0][0]
            ok = proper and alone[12] == 0 and alone[11] == alone[2]  # (alone: the rival is as strong, mapq 0)
            ok = ok and a[F["record"]] == R and a[F["rank"]] == R and a[F["mapq"]] == 60 * b[F["votes"]] // (a[F["votes"]] + b[F["votes"]]) > 0
            ok = ok and a[F["rival_votes"]] == a[F["votes"]]
        if ok:
            seen[kind] = seen.get(kind, 0) + 1
    return rows, seen


ALL_KINDS = ("fr", "rf_given", "subst", "records", "same_strand", "outie", "long", "one_hit_inside", "one_hit_outside",
             "both_one_hit", "none", "chimeric", "edge", "tie_0", "tie_1")


# ---- seams: w = 1 over a restricted key set, hits placed base by base ------------------------------------------------
class Seams:
    """A model and a map at k = 31, w = 1 whose keys are the k-mers at chosen positions of the records only: a read cut
    from a record has a hit exactly where a chosen k-mer lies inside it, so votes, extents and intervals are set base
    by base.  positions: {record: [position]}.  The model is built on the CPU; attach() makes the map."""

    def __init__(self, O, records, positions, k=31):
        self.O, self.k, self.records = O, k, records
        keys = set()
        for R, ps in positions.items():
            for P in ps:
                h, pos = O.minimizer_hashes_and_positions(records[R][P:P + k], k, 1, 0)
                assert len(h) == 1 and int(pos[0]) == 0
                keys.add(int(h[0]))
        self.keys = np.array(sorted(keys), np.uint64)
        self.model = SW.AnchorModel(O, k, 1, self.keys).add(records)
        assert self.model.info()["repeats"] == 0 and self.model.info()["anchors"] == len(keys) == sum(len(set(p)) for p in positions.values())
        self.amap = None

    def attach(self, dcn):
        idx = dcn.Index.from_keys(self.keys, self.k, 1)
        self.amap = dcn.AnchorMap(idx)
        idx.close()
        self.amap.add_records(self.records)
        return self

    def close(self):
        if self.amap is not None:
            self.amap.close()


# ---- subprocess cases ----------------------------------------------------------------------------------------------
def parity_batch(O, dcn, k, w):
    records = make_records(make_genomes())
    model, amap = build_map(O, dcn, records, k, w)
    pairs = pair_reads(model, records)
    reads = [m for _, a, b in pairs for m in (a, b)]
    return records, model, amap, pairs, reads


def case_seams(O, dcn):
    """tiles of 16 windows: every mate of 31 bases or more is cut into several tiles"""
    assert os.environ.get("DCN_TILE_WINDOWS") == "16"
    for w in (15, 1):
        _, model, amap, pairs, reads = parity_batch(O, dcn, 31, w)
        rows, _, _ = check_pairs(dcn, O, model, amap, reads, ("tiles", w))
        assert int((rows["flags"] & PROPER).astype(bool).sum()) > 100
        amap.close()
    print("place pair tiles ok")


def case_switch(O, dcn):
    """DCN_PLACE_LANE_BASES = 100: one mate on the workgroup path and one on the lane path, in both orders, and both on
    either"""
    assert os.environ.get("DCN_PLACE_LANE_BASES") == "100"
    records = make_records(make_genomes())
    rng = np.random.default_rng(972)
    for w in (1, 15):
        model, amap = build_map(O, dcn, records, 31, w)
        reads = []
        for i in range(60):
            _, _, f = fragment(rng, records, 400, 700)
            L1, L2 = [(90, 180), (180, 90), (100, 101), (101, 100), (250, 250), (80, 80)][i % 6]
            reads += list(mates_of(f, L1, L2, flip=bool(i % 4 >= 2)))
        lens = [(len(reads[2 * u]) > 100, len(reads[2 * u + 1]) > 100) for u in range(len(reads) // 2)]
        assert {(True, False), (False, True), (True, True), (False, False)} <= set(lens)
        for n in (1, 4):
            rows, _, _ = check_pairs(dcn, O, model, amap, reads, ("switch", w), max_placements=n)
            assert int((rows["flags"] & PROPER).astype(bool).sum()) >= 100
        amap.close()
    print("place pair switch ok")


def case_partitions(O, dcn):
    """DCN_PLACE_LDS_CELLS = 16 with DCN_PLACE_LANE_BASES = 200: mate 1 is stitched from scattered cuts (far more cells
    than the set has slots: the partitioned count) and ends in the fragment's head; mate 2 takes the lane path"""
    assert os.environ.get("DCN_PLACE_LDS_CELLS") == "16" and os.environ.get("DCN_PLACE_LANE_BASES") == "200"
    records = make_records(make_genomes())
    rng = np.random.default_rng(973)
    model, amap = build_map(O, dcn, records, 31, 1)
    reads = []
    for i in range(12):
        _, _, f = fragment(rng, records, 400, 700)
        m1 = SW.stitched(rng, records, 30) + f[:100 + 10 * i]
        reads += [m1, revcomp(f[-120:])] if i % 2 == 0 else [revcomp(f[-120:]), m1]
    assert SW.partitions_of(model.cells(reads[0], 256)[0], 16)[0] >= 2
    for n in (2, 8):
        rows, _, want = check_pairs(dcn, O, model, amap, reads, ("partitions",), max_placements=n)
        # (a scattered cut now and then falls into the band of the fragment's head and stretches its extent past the limit)
        assert int((rows["flags"] & PROPER).astype(bool).sum()) >= 16
    amap.close()
    print("place pair partitions ok")


if __name__ == "__main__":
    import deacon_server_amd as dcn
    from oracle import oracle as O
    O.lib()
    {"seams": case_seams, "switch": case_switch, "partitions": case_partitions}[sys.argv[1]](O, dcn)

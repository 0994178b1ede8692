"""No case of tests/_filter_seam_cases.py is vacuous: from the layout model and the oracle alone, every case reaches the line
of scan.hip or plan.hip it is built for.  CPU only.  A builder that cannot reach its shape fails here; nothing skips or
shrinks itself when the GPU tests run."""
import collections

import numpy as np
import pytest

import _filter_seam_cases as F
from _filter_seam_cases import LOCAL_ITEMS, RCAP, WAVE
from test_gpu_classify_seams import required

GEOMS = pytest.mark.parametrize("k,w", F.GEOMETRIES, ids=["k%dw%d" % g for g in F.GEOMETRIES])


def test_the_constants_are_the_sources():
    """the figures the issue names, as the sources state them today: a changed constant fails here"""
    assert (F.WAVE, F.LCAP, F.RCAP, LOCAL_ITEMS) == (64, 40, 256, 192)
    assert F.fixed_ws() == [1, 11, 15]
    assert [F.flush_above(w) for w in (15, 11, 9)] == [25, 29, 32]
    assert (F.LDS_SET_MAX, F.LDS_WALK_MAX_TILES, F.FAST_EXTRA, F.TILE_WINDOWS, F.SHORT_LMAX) == (1400, 1024, 4, 256, 152)
    assert F.early_out_max_items(2, 0.01) == 249 and F.early_out_max_items(2, 0.2) == 12


@GEOMS
def test_every_case_fits_the_layout_model(k, w):
    """at most 256 reads (one planning workgroup), every read one tile of at most flush_above entries unless the case says
    otherwise, and the two models agree on every unit"""
    W = F.world(k, w)
    for c in W.cases:
        reads, uid = c.batch()
        assert uid.tolist() == sorted(uid.tolist()) and uid[-1] == len(c.units) - 1
        L = W.layout(c.name)
        assert len(L.tiles) == len(reads), c.name  # one tile per read
        b, o = W.O.concat_reads(reads)
        oidx = W.O.Index(W.key_array(), k, w)
        for abs_t, rel_t, deplete in c.thresholds:
            want = W.O.filter_batch(oidx, b, o, uid, abs_t, rel_t, 0, deplete)
            plain = F.expected(W.O, c, W.keys, abs_t, rel_t, deplete)
            assert [x.tolist() for x in want] == [list(x) for x in plain], c.name
        if c.name != "A6":
            assert not any(L.flushes(i) for i in range(L.n_waves)), c.name


@GEOMS
def test_a1_reaches_the_ring_limit(k, w):
    """scan.hip flush(): `sh.items[uslot] <= (uint32_t)(DCN_RCAP - DCN_WAVE)`"""
    W = F.world(k, w)
    c, L = W.by_name["A1"], W.layout("A1")
    for name, n_items, in_wave in (("191", 191, True), ("192", 192, True), ("193", 193, False), ("192bad", 192, True)):
        u = c.mark[name]
        items = L.items(u)
        assert len(items) == n_items and L.local(u) and L.in_wave(u) is in_wave, name
        assert L.lanes_of(u)[0][1] == 0, "the unit starts its wave"
        hits = L.hits(u, W.keys)
        assert len(hits) == len([h for h in items if h is not None]), "every valid item is a hit"
        assert len(set(hits)) < len(hits), "duplicates inside"
    assert L.items(c.mark["192bad"]).count(None) == 5  # items != total


@GEOMS
def test_a1_and_a2_thresholds_sit_on_the_rounding(k, w):
    """dcn_required_hits: rel * total is x.5 exactly; distinct hits are required - 1 and required, raw hits more"""
    W = F.world(k, w)
    c, L = W.by_name["A1t"], W.layout("A1t")
    for n_items, in_wave in ((191, True), (193, False)):
        for less in (1, 0):
            u = c.mark["%d-%d" % (n_items, less)]
            hits = L.hits(u, W.keys)
            total = len([h for h in L.items(u) if h is not None])
            assert total == n_items and (0.5 * total) % 1 == 0.5 and L.in_wave(u) is in_wave
            assert len(set(hits)) == required(1, 0.5, total) - less and len(hits) > len(set(hits))
    c, L = W.by_name["A2t"], W.layout("A2t")
    for less in (1, 0):
        u = c.mark["63-%d" % less]
        hits = L.hits(u, W.keys)
        assert len(L.items(u)) == 63 and L.in_wave(u) and len(set(hits)) == 32 - less and len(hits) > len(set(hits))


@GEOMS
def test_a2_repeats_at_every_distance(k, w):
    """scan.hip: `for (uint32_t d0 = 0; __any(d0 < run); d0 += 4)`: distances on both sides of a step of four, of a round of
    64 items (sh.hraw carried over) and the longest the ring serves"""
    W = F.world(k, w)
    c, L = W.by_name["A2"], W.layout("A2")
    u, v = c.mark["dup"], c.mark["control"]
    hits = L.hits(u, W.keys)
    assert L.in_wave(u) and L.in_wave(v) and len(hits) == LOCAL_ITEMS == len(L.hits(v, W.keys))
    d = F.distances(hits)
    assert sorted(d) == sorted(F.A2_DISTANCES) and all(d[x] == F.A2_RANKS[x] for x in d)
    assert len(set(hits)) == LOCAL_ITEMS - len(F.A2_DISTANCES)
    assert F.distances(L.hits(v, W.keys)) == {}
    # the copy at distance 63, 64, 65 and 191 is handled in a later round than the first: every item is a hit, so hit rank = flat item
    assert [h for _, h in L.flat(L.waves_of(u)[0])] == hits
    assert all((d[x] + x) // WAVE > d[x] // WAVE for x in (63, 64, 65, 191))


@GEOMS
def test_a3_neighbours_meet_in_the_ring(k, w):
    """scan.hip: `d0 + 3 < run` and `(x - d0 - 4) & (DCN_RCAP - 1)`"""
    W = F.world(k, w)
    c, L = W.by_name["A3"], W.layout("A3")
    ring = L.ring(0, W.keys)
    units = [u for u, _ in ring]
    A, B, C, D = (c.mark[x] for x in "ABCD")
    assert all(L.in_wave(u) for u in (A, B, C, D))
    a_last = max(i for i, u in enumerate(units) if u == A)
    assert units[a_last + 1] == B and ring[a_last][1] == ring[a_last + 1][1], "A's last hit is B's first"
    assert L.hits(A, W.keys).count(ring[a_last][1]) == 1 and L.hits(B, W.keys).count(ring[a_last][1]) == 1
    c_last = max(i for i, u in enumerate(units) if u == C)
    d_hits = L.hits(D, W.keys)
    assert units[c_last + 1] == D and d_hits[3] == ring[c_last][1] == d_hits[7] and d_hits.index(ring[c_last][1]) == 3
    # (a walk one slot too far from D's hit of rank 3 reads slot c_last, which holds the same hash)
    ring = L.ring(1, W.keys)
    assert len(ring) > RCAP and len({u for u, _ in ring}) == 5
    R0, R4 = c.mark["R0"], c.mark["R4"]
    first4 = min(i for i, (u, _) in enumerate(ring) if u == R4)
    assert first4 == RCAP and ring[first4 - RCAP] == (R0, ring[first4][1]), "R4's first hit is the hash 256 slots earlier"
    r4 = L.hits(R4, W.keys)
    assert len(set(r4)) < len(r4) and r4.count(r4[0]) == 1


@GEOMS
def test_a4_round_geometry(k, w):
    """scan.hip: `run_head = lok && (below == 0 || prev_us != o_uslot[u])`"""
    W = F.world(k, w)
    c, L = W.by_name["A4"], W.layout("A4")
    flat = L.flat(0)
    assert len(flat) == 3 * WAVE
    u0, u1 = c.mark["lane0"], c.mark["lane63"]
    assert [u for u, _ in flat[:64]] == [u0] * 64 and [u for u, _ in flat[64:128]] == [u1] * 64  # boundaries at 63|64, 127|128
    hit = [i for i, (u, h) in enumerate(flat) if h in W.keys]
    assert [i for i in hit if i < 128] == [0, 127], "the only hits of rounds 0 and 1: lane 0 and lane 63"
    in_round2 = [u for u, h in flat[128:] if h in W.keys]
    assert len(set(in_round2)) == 3 and all(L.in_wave(u) for u in set(in_round2))
    e = c.mark["echo"]
    flat = L.flat(1)
    assert [u for u, _ in flat[:128]] == [e] * 128 and [h for _, h in flat[:64]] == [h for _, h in flat[64:128]]
    assert all(h in W.keys for _, h in flat[:128]) and L.in_wave(e)  # round 1: 64 hit lanes, every one a duplicate


@GEOMS
def test_a6_one_lane_flushes_the_wave(k, w):
    """scan.hip: `if (__any(cnt > DCN_LCAP - STEP)) flush(IntTag<1>{}, false)`, `if (!final_flush) go_global = true`"""
    W = F.world(k, w)
    c, L = W.by_name["A6"], W.layout("A6")
    low = c.mark["low"]
    (wave, lane), = L.lanes_of(low)
    assert (wave, lane) == (0, 10) and L.tiles[10].entries > F.flush_above(w) and len(L.tiles) == WAVE
    assert L.flushes(0) and not any(L.in_wave(u) for u in range(len(c.units)))
    assert all(t.entries <= F.flush_above(w) for i, t in enumerate(L.tiles) if i != 10)
    twin, L2 = W.by_name["A6c"], W.layout("A6c")
    assert [u for i, u in enumerate(c.units) if i != low] == twin.units
    assert not L2.flushes(0) and all(L2.in_wave(u) for u in range(len(twin.units)))
    for lay, case in ((L, c), (L2, twin)):  # planted hits, and in EVERY clean unit the same hash as a hit twice: after the
        for u in range(len(case.units)):    # flush the distinct pass sees them, without it the ring
            hits = lay.hits(u, W.keys)
            assert (u == low and lay is L) or (len(hits) >= 4 and len(set(hits)) < len(hits)), u
    assert len(twin.units) == 22 and sum(len(u) for u in twin.units) == WAVE - 1


def test_c2_raw_hits_sit_on_the_set_limit():
    """plan.hip: `Hset > DCN_LDS_SET_MAX`"""
    W = F.world(31, 15)
    for H in (F.LDS_SET_MAX - 1, F.LDS_SET_MAX, F.LDS_SET_MAX + 1):
        c, L = W.by_name["C2-%d" % H], W.layout("C2-%d" % H)
        hits = L.hits(0, W.keys)
        assert len(hits) == H and len(set(hits)) == H - 64
        assert L.waves_of(0) == [0, 1] and not L.in_wave(0) and len(L.where(0)) <= F.LDS_WALK_MAX_TILES
        assert all(len(L.hits(0, W.keys, wv)) > 0 for wv in (0, 1))  # a run in each wave


def test_c3_units_sit_on_enough():
    """plan.hip: `if ((uint64_t)H < req)`, `Hset = H < enough ? H : enough`, `distinct < enough`"""
    W = F.world(31, 15)
    for name, total in (("C3-2", 200), ("C3-33", 200), ("C3-300", 5000)):
        c, L = W.by_name[name], W.layout(name)
        req = c.req
        assert all(required(a, r, total) == req for a, r, _ in c.thresholds)
        u = c.mark["below"]
        hits = L.hits(u, W.keys)
        assert len(L.items(u)) == total and len(set(hits)) == req - 1 and len(hits) >= max(req, 2 * (req - 1)) and not L.in_wave(u)
        if total == 5000:
            assert len(hits) > F.LDS_SET_MAX and req - 1 <= F.LDS_SET_MAX  # served by the LDS set through Hset
            u = W.by_name[name + "-early"].mark["early"]
            L2 = W.layout(name + "-early")
            first_run = L2.hits(u, W.keys, 0)
            req2 = W.by_name[name + "-early"].req
            assert req2 == 33 and len(set(first_run[:F.ENOUGH_STRIDE])) >= req2 and len(first_run) == 1280
            assert len(L2.hits(u, W.keys)) == 5000
            continue
        u = c.mark["last"]
        hits = L.hits(u, W.keys)
        assert len(set(hits)) == req and hits.count(hits[-1]) == 1 and L.items(u)[-1] == hits[-1]
        u = c.mark["few"]
        assert len(L.hits(u, W.keys)) == req - 1
        u = c.mark["exact"]
        assert len(L.hits(u, W.keys)) == req == len(set(L.hits(u, W.keys))) and not L.in_wave(u)  # H == required: `H < req`, not `<=`


def _fast_model(L, keys, need):
    """the early-out block of scan_body on wave 0 of a layout: per lane (nh after the own-list rounds, rem) and R1"""
    tiles = L.wave(0)
    R1 = min(F.fast_r1(need), max(len(t.items) for t in tiles))
    units = collections.OrderedDict()
    for lane, t in enumerate(tiles):
        units.setdefault(t.unit, []).append(lane)
    nh, rem = {}, {}
    for u, lanes in units.items():
        seen = []
        for j in range(R1):
            for lane in lanes:
                it = tiles[lane].items
                if j < len(it) and len(seen) < need and it[j] in keys and it[j] not in seen:
                    seen.append(it[j])
        for lane in lanes:
            nh[lane] = len(seen)
            rem[lane] = len(tiles[lane].items) - R1 if len(seen) < need and len(tiles[lane].items) > R1 else 0
    return R1, nh, rem


@pytest.mark.parametrize("need", (1, 2, 3, 4))
def test_b1_b2_reach_the_early_out_edges(need):
    """scan.hip, FAST block: note_hit's seen0..2, `R1`, the flattened rest"""
    c, _ = F.b_world(need)
    O = F._oracle()
    L = F.Layout(O, c)
    keys = c.keys
    most = F.early_out_max_items(need, 0.01)
    assert len(L.tiles) == WAVE and not L.flushes(0)
    for u in range(len(c.units)):  # `own` holds for every lane: the wave takes the early-out
        assert len(L.where(u)) <= 2 and L.local(u) and len(L.items(u)) <= most
    R1, nh, rem = _fast_model(L, keys, need)
    assert R1 == need + F.FAST_EXTRA
    start = np.concatenate([[0], np.cumsum([rem[i] for i in range(WAVE)])])
    keep = F.expected(O, c, keys, need, 0.01, False)[0]
    for rep in range(6):
        for kind in ("none", "near", "far"):
            u = c.mark["%s%d" % (kind, rep)]
            (_, lane), = L.lanes_of(u)
            items = L.tiles[lane].items
            hits = L.hits(u, keys)
            assert len(set(items[:F.B_SAME])) == 1
            if need > 1 or kind == "near":
                assert hits[:min(need, F.B_SAME)] == [items[0]] * min(need, F.B_SAME), "the first `need` hits are one hash"
            assert keep[u] is (kind != "none") and len(set(hits)) == need - (kind == "none")
            if kind == "near":
                assert max(items.index(h) for h in set(hits)) < R1 and nh[lane] == need
            if kind == "far":
                at = items.index(hits[-1])
                assert at == F.B_FAR_RANK >= R1 and nh[lane] == need - 1 and rem[lane] > 0
                e = int(start[lane]) + at - R1
                assert e % WAVE != lane, "another lane probes it and hands it back"
        for kind, kept in (("rc_below", False), ("rc_at", True), ("mate2", True)):
            u = c.mark["%s%d" % (kind, rep)]
            (_, a), (_, b) = L.lanes_of(u)
            assert b == a + 1 and keep[u] is kept
            if kind == "mate2":
                assert not set(L.tiles[a].items) & keys and len(set(L.tiles[b].items) & keys) == need
            else:
                assert sorted(L.tiles[a].items) == sorted(L.tiles[b].items)  # the reverse complement: the same hashes
                assert len(set(L.hits(u, keys))) == need - (kind == "rc_below") and len(L.hits(u, keys)) == 2 * len(set(L.hits(u, keys)))


def test_b3_one_lane_takes_the_early_out_from_its_wave():
    """scan.hip: `cnt_unit <= a.early_out_max_items`, `if (__all(own))`"""
    (c, twin), most = F.b3_world()
    O = F._oracle()
    L, L2 = F.Layout(O, c), F.Layout(O, twin)
    assert most == 12 and len(L.tiles) == 3 * WAVE
    cut = c.mark["cut"]
    assert L.lanes_of(cut) == [(0, 63), (1, 0)] and not L.local(cut)
    last = c.mark["last"]
    assert L.lanes_of(last) == [(2, 63)] and len(L.items(last)) == most + 1 and len(L2.items(last)) == most
    for lay in (L, L2):
        for t in lay.wave(2)[:-1]:
            assert len(t.items) <= most and lay.local(t.unit)
    assert c.units[:-1] == twin.units[:-1]
    assert not any(L.flushes(i) for i in range(3))


@GEOMS
def test_a5_tiles_lie_where_the_case_says(k, w):
    """scan.hip: `first >= wave_first && first + count <= wave_first + DCN_WAVE`"""
    c, L = F.a5_world(k, w)
    assert (c.k, c.w) == (k, w) and F.TINY + 1 <= F.flush_above(w)
    keys = c.keys
    assert len(L.tiles) == 193 and not any(L.flushes(i) for i in range(L.n_waves))
    lanes = {name: L.lanes_of(u) for name, u in c.mark.items()}
    assert lanes["first"][0] == (0, 0) and lanes["ends63"][-1] == (0, 63) and L.in_wave(c.mark["ends63"]) and L.in_wave(c.mark["first"])
    assert lanes["lane0"][0] == (1, 0) and L.in_wave(c.mark["lane0"])
    u = c.mark["crosses"]
    assert lanes["crosses"][-2:] == [(1, 63), (2, 0)] and not L.local(u)
    assert L.hits(u, keys, 1) and L.hits(u, keys, 2), "a run in each wave"
    p = c.mark["pair"]
    assert lanes["pair"] == [(2, 63), (3, 0)]
    a, b = L.hits(p, keys, 2), L.hits(p, keys, 3)
    assert a and sorted(a) == sorted(b) and len(set(a)) == len(a), "every hash hit once on either side of the boundary"
    for name in ("first", "lane0", "crosses"):
        h = L.hits(c.mark[name], keys)
        assert len(set(h)) < len(h), name  # the repeated segment gave duplicates
    assert all(len(L.items(c.mark[n])) <= LOCAL_ITEMS for n in ("first", "ends63", "lane0"))


def test_c4_reads_sit_on_the_tile_limit():
    """plan.hip: `count > DCN_LDS_WALK_MAX_TILES`"""
    c, L = F.c4_world()
    for u, n_tiles in ((0, F.LDS_WALK_MAX_TILES), (1, F.LDS_WALK_MAX_TILES + 1)):
        where = L.where(u)
        assert len(where) == n_tiles
        first = where[0][0]
        slices = [(t - first) // 64 for t, x in where for h in x.items if h in c.keys]
        hits = L.hits(u, c.keys)
        assert len(hits) == 5 and len(set(hits)) == 4 and len(set(slices)) >= 4
        twice = [h for h in set(hits) if hits.count(h) == 2][0]
        a, b = [(t - first) // 64 for t, x in where for h in x.items if h == twice]
        assert a != b, "the two copies lie in different 64-tile slices"
        assert (n_tiles + 63) // 64 == (16 if u == 0 else 17)


def test_c1_units_have_their_copies():
    """plan.hip: the LDS pass's 256-entry passes, `old == h[q]`, g_zero"""
    units, keys, names = F.c1_units()
    by = dict(zip(names, units))
    assert 0 not in keys.tolist()
    ks = set(keys.tolist())
    for H in F.C1_H:
        a = by["all-%d" % H]
        assert len(a) == H and all(x in ks for x in a.tolist())
        if H >= 2:
            assert a[1] == a[0]
        if H > 260:
            assert a[256] == a[250] and a[259] == a[253]  # a copy on either side of entry 256
        if H >= 8:
            assert a[-1] == a[-5]
        b = by["third-%d" % H].tolist()
        if H >= 3:
            assert 0.2 < sum(x not in ks for x in b) / H < 0.45
    assert [int((by["zero-%d" % n] == 0).sum()) for n in (0, 1, 3)] == [0, 1, 3]
    assert sum(n.startswith("small") for n in names) == 300 and max(len(u) for u in units) == 2900


@GEOMS
def test_no_case_overflows_a_run_unasked(k, w):
    """scan.hip: `a.status->run_overflow = 1`.  A rerun at one slot per window would pass and leave the context at another
    record geometry: no case raises it at the default DCN_REC_SHIFT"""
    W = F.world(k, w)
    assert F.REC_SHIFT == 2 and all(F.runs_fit(W.layout(c.name), W.keys, F.REC_SHIFT) for c in W.cases)


def test_c5_sweeps_what_it_says():
    """C5's plan: every case of the (31, 15) world, A6 among them, and the B batches, over one index.  No hash of one case is a
    key of another (the plain statement under the union equals the one under the case's own keys); no run overflows at
    DCN_REC_SHIFT = 3 except the batch kept for that; and under its own threshold every lane of B-n is `own`, so a
    decisions-only call of it returns from the scan's early-out and a counting call follows on the same context."""
    W = F.world(31, 15)
    O = W.O
    plan, keys = W.stale_plan()
    names = [c.name for c, _ in plan]
    assert names == [c.name for c in W.cases] + ["B-1", "B-2", "B-3", "B-4", "B3", "B3twin"] and "A6" in names and len(names) == 21
    own = {name: ks for name, _, ks, _ in F.b_plan()}
    for c, thr in plan:
        L = F.Layout(O, c)
        assert F.runs_fit(L, keys, 3), c.name
        for t in thr:
            assert F.expected(O, c, keys, *t) == F.expected(O, c, own.get(c.name, W.keys), *t), c.name
        if c.name.startswith("B-"):
            need = thr[0][0]
            assert len(L.tiles) == WAVE and not L.flushes(0)
            assert all(len(L.where(u)) <= 2 and L.local(u) and len(L.items(u)) <= F.early_out_max_items(need, 0.01)
                       for u in range(len(c.units)))
    over, okeys = W.overflow_case()
    L = F.Layout(O, over)
    assert okeys <= keys and L.flushes(0) and not F.runs_fit(L, keys, 3) and len(L.hits(0, keys)) > 8 * len(set(L.hits(0, keys)))
    assert not set(L.items(0)) & set(W.layout("A6").items(W.by_name["A6"].mark["low"])), "A6's periodic read stays without a hit"


@GEOMS
def test_a7_keys_crowd_their_home_groups(k, w):
    """dcn_probe.h through scan.hip: `while (r < 0) { grp[u] = (grp[u] + 1) & a.table.group_mask; ... }`"""
    from test_classify_replicas import group_of
    from test_gpu_classify_seams import group_slots
    single, fours, G, quads = F.a7_world(k, w)
    S = group_slots()
    assert G == 64 == F.table_groups(len(single.keys), F.A7_SLOTS_PER_KEY) and len(single.keys) == (S + 1) * len(quads)
    homes = []
    for q in quads:
        hs = np.array([e.items[0] for e in q], np.uint64)
        home = set(group_of(hs, G).tolist())
        assert len(home) == 1 and len(q) == S + 2
        homes.append(home.pop())
        assert [int(h) in single.keys for h in hs] == [True] * (S + 1) + [False], "one key more than a group holds, one absent"
    assert len(set(homes)) == len(homes)
    O = F._oracle()
    L1, L4 = F.Layout(O, single), F.Layout(O, fours)
    assert all(len(L1.where(u)) == 1 for u in range(len(single.units))) and len(L1.tiles) <= WAVE  # every unit its own lane: `own`
    assert all(len(L4.hits(u, fours.keys)) == S + 2 and len(set(L4.hits(u, fours.keys))) == S + 1 for u in range(len(fours.units)))
    assert sum(L4.in_wave(u) for u in range(len(fours.units))) == len(fours.units) - 1  # (the unit in lanes 60..64 is exported)


def test_a8_batches_take_the_short_path_and_reach_its_edges():
    """scan.hip: scan_short, `if (sh.lok[uslot] || (SHORT && !enrol))`; ctx.hip: `short_fused = ... !v.d_unit_id ...`"""
    world = F.a8_world()
    O = F._oracle()
    for name, (es, keys) in world.items():
        assert all(len(e.read) <= F.SHORT_LMAX and F.windows_of(len(e.read), 31, 15) <= F.TILE_WINDOWS for e in es)
        assert all(analyse_again == e.items for e in es for analyse_again in [F.analyse(O, e.read, 31, 15)])
    dups, keys = world["dups"]
    found = set()
    for e in dups:
        assert None not in e.items and set(e.items) <= keys and len(e.items) <= F.flush_above(15)
        found |= set(F.distances(list(e.items)))
    assert set(F.A8_DISTANCES) | {8} <= found and len(dups) == WAVE
    for name, n in (("flush64", 64), ("flush65", 65)):
        es, keys = world[name]
        assert len(es) == n and len(es[10].items) > F.flush_above(15) and not set(es[10].items) & keys
        others = [e for i, e in enumerate(es[:WAVE]) if i != 10]
        twice = [e for e in others if len([h for h in e.items if h in keys]) > len({h for h in e.items if h in keys})]
        assert len(twice) >= 15, "reads that go to the work list with the same hash as a hit twice"
        assert all(len(e.items) <= F.flush_above(15) for e in others)
        with_hits = [e for e in others if set(e.items) & keys]
        assert len(with_hits) > 30 and len(others) - len(with_hits) > 15, "both kinds share the flushed wave"
        # a read's run holds its hits: run_cap = (offset + windows + l - 1 >> shift) - (offset >> shift) >= (len >> shift) - 1
        assert all(len([h for h in e.items if h in keys]) <= (len(e.read) >> F.REC_SHIFT) - 1 for e in with_hits)


def test_c4_one_hash_on_both_sides_of_a_slice():
    """plan.hip pass A: `t0 += 64`"""
    c, L = F.c4_boundary_world()
    assert len(L.tiles) == F.LDS_WALK_MAX_TILES
    hits = [(t // 64, h) for t, x in enumerate(L.tiles) for h in x.items if h in c.keys]
    in7, in8 = [h for s, h in hits if s == 7], [h for s, h in hits if s == 8]
    assert in7 and in8 and in7[-1] == in8[0], "the last hit of slice 7 is the first hit of slice 8"
    assert set(in7) == set(in8) and len(set(in7)) == 1  # the other two keys lie in other slices
    assert len({h for _, h in hits}) == 3 and len(hits) >= 4 and len({s for s, _ in hits}) >= 4

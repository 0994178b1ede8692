"""The filter's distinct-hit count at the seams of scan.hip and plan.hip: the in-wave ring's limit, its compare walk and
its wrap, round and unit boundaries, locality across waves, the mid-scan flush, the early-out of decisions-only mode, and
the distinct pass at its set limit, its tile limit and its stop at `enough`.  The batches are written item by item in
tests/_filter_seam_cases.py; tests/test_filter_seam_cases.py proves on the CPU that each reaches its edge.  Every batch goes
through counting mode and through counts=False (check_batch), and is compared with two models: the oracle's filter_batch /
should_keep_hashes, and the plain statement total = valid minimizers, hits = |set(hashes) & keys|.  Every comparison is exact.

Geometries: every scan case runs at (31, 15), (41, 15) (K128), (31, 11) (the other fixed W) and (21, 9) (generic w, STEP 8);
A1 to A7 run at all four and none is dropped: units of short reads, reads of a chosen number of 16-window tiles and
single-window reads with a chosen home group reach every shape at any k and w.  A8 is the short path, which exists for
w = 15 and k <= 32 only.  B and C are asked for without a geometry and run at (31, 15)."""
import numpy as np
import pytest

import _filter_seam_cases as F
from test_gpu_parity import check_batch

pytestmark = pytest.mark.gpu

SCAN_CASES = ("A1", "A1t", "A2", "A2t", "A3", "A4", "A6", "A6c")
GEOM_IDS = ["k%dw%d" % g for g in F.GEOMETRIES]


def make_proc(dcn, gidx):
    return dcn.FilterProcessor(gidx, max_batch_bases=1 << 20, max_batch_reads=1 << 10)


def index_pair(oracle, dcn, keys, k, w):
    keys = np.array(sorted(keys), np.uint64)
    gidx = dcn.Index.from_keys(keys, k, w)
    assert gidx.n_keys == len(keys)
    return oracle.Index(keys, k, w), gidx


def run_case(oracle, proc, oidx, case, keys, thresholds=None):
    """the case under each of its thresholds, against both models -> [(keep, hits, total)]"""
    reads, uid = case.batch()
    out = []
    for abs_t, rel_t, deplete in thresholds or case.thresholds:
        proc.abs_threshold, proc.rel_threshold, proc.deplete = abs_t, rel_t, deplete
        b, o = oracle.concat_reads(reads)
        got = proc.filter_batch(b, o, uid)
        keep, hits, total = F.expected(oracle, case, keys, abs_t, rel_t, deplete)
        for u in range(len(case.units)):  # (total, hits, keep) of the first unit that differs from the plain statement
            assert (int(got[2][u]), int(got[1][u]), bool(got[0][u])) == (total[u], hits[u], keep[u]), (case.name, "unit", u)
        only = proc.filter_batch(b, o, uid, counts=False).tolist()
        assert only == keep, (case.name, "decisions only", "unit", [u for u in range(len(keep)) if only[u] != keep[u]][0])
        got = check_batch(oracle, proc, oidx, reads, uid)
        out.append([x.tolist() for x in got])
    return out


@pytest.fixture(scope="module")
def ctx(oracle, dcn):
    """(world, oracle index, processor) per geometry, made on first use"""
    made = {}

    def get(k, w):
        if (k, w) not in made:
            W = F.world(k, w)
            oidx, gidx = index_pair(oracle, dcn, W.keys, k, w)
            made[(k, w)] = (W, oidx, make_proc(dcn, gidx), gidx)
        return made[(k, w)]
    return get


# ---- A: the scan kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCAN_CASES)
@pytest.mark.parametrize("k,w", F.GEOMETRIES, ids=GEOM_IDS)
def test_scan_seams(oracle, ctx, k, w, name):
    W, oidx, proc, _ = ctx(k, w)
    run_case(oracle, proc, oidx, W.by_name[name], W.keys)


@pytest.mark.parametrize("k,w", F.GEOMETRIES, ids=GEOM_IDS)
def test_a_flushing_lane_leaves_its_neighbours_their_counts(oracle, ctx, k, w):
    """A6: hits and totals of the 63 clean reads are the same with and without the low-complexity read in their wave"""
    W, oidx, proc, _ = ctx(k, w)
    with_it, without = W.by_name["A6"], W.by_name["A6c"]
    low = with_it.mark["low"]
    a = run_case(oracle, proc, oidx, with_it, W.keys)
    b = run_case(oracle, proc, oidx, without, W.keys)
    for x, y in zip(a, b):
        assert [v[:low] + v[low + 1:] for v in x] == y


@pytest.mark.parametrize("k,w", F.GEOMETRIES, ids=GEOM_IDS)
def test_locality_with_tiny_tiles(oracle, dcn, monkeypatch, k, w):
    """A5, at the context's own record geometry and at DCN_REC_SHIFT 0 and 2"""
    c, _ = F.a5_world(k, w)
    oidx, gidx = index_pair(oracle, dcn, c.keys, c.k, c.w)
    monkeypatch.setenv("DCN_TILE_WINDOWS", c.env["DCN_TILE_WINDOWS"])
    for shift in (None, "0", "2"):
        if shift is not None:
            monkeypatch.setenv("DCN_REC_SHIFT", shift)
        run_case(oracle, make_proc(dcn, gidx), oidx, c, c.keys)


def test_the_tile_count_edge(oracle, dcn, monkeypatch):
    """C4: 1024 tiles (pass A's walk) and 1025 (the global set), at the three record geometries"""
    c, _ = F.c4_world()
    oidx, gidx = index_pair(oracle, dcn, c.keys, c.k, c.w)
    monkeypatch.setenv("DCN_TILE_WINDOWS", c.env["DCN_TILE_WINDOWS"])
    for shift in (None, "0", "2"):
        if shift is not None:
            monkeypatch.setenv("DCN_REC_SHIFT", shift)
        proc = dcn.FilterProcessor(gidx, max_batch_bases=1 << 20, max_batch_reads=1 << 10)
        run_case(oracle, proc, oidx, c, c.keys, THRESHOLDS_C4)


def test_one_hash_on_both_sides_of_a_slice(oracle, dcn, monkeypatch):
    """C4: the same hash as the last hit of one 64-tile slice and the first of the next"""
    c, _ = F.c4_boundary_world()
    oidx, gidx = index_pair(oracle, dcn, c.keys, c.k, c.w)
    monkeypatch.setenv("DCN_TILE_WINDOWS", c.env["DCN_TILE_WINDOWS"])
    run_case(oracle, make_proc(dcn, gidx), oidx, c, c.keys, ((3, 0.0, False), (4, 0.0, False)))


THRESHOLDS_C4 = ((2, 0.0, False), (4, 0.0, False), (5, 0.0, True))  # 4 distinct hits: below, at and above


@pytest.mark.parametrize("k,w", F.GEOMETRIES, ids=GEOM_IDS)
def test_the_table_walk(oracle, dcn, monkeypatch, k, w):
    """A7: keys displaced from a full home group and absent hashes behind one, through phase B and through probe_item.  The
    built table has the group count the case's home groups were computed for."""
    from test_gpu_classify_seams import group_slots
    single, fours, G, _ = F.a7_world(k, w)
    monkeypatch.setenv("DCN_TABLE_SLOTS_PER_KEY", single.env["DCN_TABLE_SLOTS_PER_KEY"])
    oidx, gidx = index_pair(oracle, dcn, single.keys, k, w)
    assert gidx.table_bytes == G * group_slots() * 8
    proc = make_proc(dcn, gidx)
    for c in (single, fours):
        run_case(oracle, proc, oidx, c, single.keys)


@pytest.mark.parametrize("name", ("dups", "flush64", "flush65"))
def test_the_short_path(oracle, dcn, name):
    """A8: device batches without unit ids; last_batch_short() says that the scan kernel packed them itself"""
    from test_gpu_short_fused import DeviceBatch
    es, keys = F.a8_world()[name]
    oidx, gidx = index_pair(oracle, dcn, keys, 31, 15)
    proc = make_proc(dcn, gidx)
    c = F.Case(name, 31, 15, "A8")
    for e in es:
        c.add([e], keys=())
    for abs_t, rel_t, deplete in F.THRESHOLDS:
        proc.abs_threshold, proc.rel_threshold, proc.deplete = abs_t, rel_t, deplete
        batch = DeviceBatch(oracle, [e.read for e in es])
        batch.enqueue(proc)
        proc.synchronize()
        assert proc.last_batch_short() is True
        batch.check(oracle, oidx, proc)
        keep, hits, total = batch.results()
        want = F.expected(oracle, c, keys, abs_t, rel_t, deplete)
        for u in range(len(es)):
            assert (int(total[u]), int(hits[u]), bool(keep[u])) == (want[2][u], want[1][u], want[0][u]), (name, "read", u)


# ---- B: decisions-only mode ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("need", (1, 2, 3, 4))
def test_early_out(oracle, dcn, need):
    """B1 and B2: check_batch compares counts=False with the oracle's decisions; keep and deplete"""
    c, _ = F.b_world(need)
    oidx, gidx = index_pair(oracle, dcn, c.keys, c.k, c.w)
    run_case(oracle, make_proc(dcn, gidx), oidx, c, c.keys, ((need, 0.01, False), (need, 0.01, True)))


def test_one_long_list_takes_the_early_out_from_its_wave(oracle, dcn):
    """B3: the 63 reads beside the read of 13 items are decided as beside the read of 12, where the early-out runs"""
    (c, twin), _ = F.b3_world()
    oidx, gidx = index_pair(oracle, dcn, c.keys | twin.keys, c.k, c.w)
    proc = make_proc(dcn, gidx)
    a = run_case(oracle, proc, oidx, c, c.keys | twin.keys)
    b = run_case(oracle, proc, oidx, twin, c.keys | twin.keys)
    for x, y in zip(a, b):  # (run_case has compared the decisions-only calls of both with the plain statement)
        assert [v[:-1] for v in x] == [v[:-1] for v in y]


_B4 = """
import json
import numpy as np
import conftest  # (torch first)
import deacon_server_amd as dcn
import _filter_seam_cases as F
from oracle import oracle as O
O.lib()
out = {}
for name, case, keys, thr in F.b_plan():
    gidx = dcn.Index.from_keys(np.array(sorted(keys), np.uint64), 31, 15)
    proc = dcn.FilterProcessor(gidx, max_batch_bases=1 << 20, max_batch_reads=1 << 10)
    reads, uid = case.batch()
    b, o = O.concat_reads(reads)
    for t in thr:
        proc.abs_threshold, proc.rel_threshold, proc.deplete = t
        out["%s %s" % (name, list(t))] = proc.filter_batch(b, o, uid, counts=False).tolist()
print("RESULT " + json.dumps(out))
"""


def test_decisions_without_the_early_out(oracle):
    """B4: the switch is read once per process (ctx.hip, enqueue_batch: `static const bool no_early_out`), so the control is a
    process of its own: the decisions of the B batches with the early-out and `enough` switched off equal the plain
    statement, as they do with both switched on (test_early_out, test_one_long_list_...).  The variable's name is taken from
    that line of ctx.hip (F.NO_EARLY_OUT_ENV), so a renamed or misspelt switch fails instead of passing with the early-out on."""
    import json
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([here, os.path.dirname(here)]))
    env[F.NO_EARLY_OUT_ENV] = "1"
    r = subprocess.run([sys.executable, "-c", _B4], env=env, cwd=here, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][0][7:])
    n = 0
    for name, case, keys, thr in F.b_plan():
        for t in thr:
            assert got["%s %s" % (name, list(t))] == F.expected(oracle, case, keys, *t)[0], (name, t)
            n += 1
    assert n == len(got) == 12


# ---- C: the distinct pass -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_zero", (False, True))
def test_exact_hashes(oracle, dcn, with_zero):
    """C1: should_keep_hashes, one run per unit, with and without key 0 in the index"""
    units, keys, _ = F.c1_units()
    if with_zero:
        keys = np.concatenate([[np.uint64(0)], keys])
    oidx, gidx = oracle.Index(keys, 31, 15), dcn.Index.from_keys(keys, 31, 15)
    proc = make_proc(dcn, gidx)
    off = np.concatenate([[0], np.cumsum([len(u) for u in units])]).astype(np.uint64)
    flat = np.concatenate(units)
    for abs_t, rel_t, deplete in ((2, 0.01, False), (1, 0.5, False), (1, 0.5, True), (3, 0.9, False)):
        proc.abs_threshold, proc.rel_threshold, proc.deplete = abs_t, rel_t, deplete
        got = proc.should_keep_hashes(flat, off)
        want = oracle.should_keep_hashes(oidx, flat, off, abs_t, rel_t, deplete)
        plain = F.c1_expected(units, keys, with_zero, abs_t, rel_t, deplete)
        for g, w_, p in zip(got, want, plain):
            assert g.tolist() == w_.tolist() == list(p)


C_CASES = ["C2-%d" % H for H in (F.LDS_SET_MAX - 1, F.LDS_SET_MAX, F.LDS_SET_MAX + 1)] + ["C3-2", "C3-33", "C3-300", "C3-300-early"]


@pytest.mark.parametrize("name", C_CASES)
def test_distinct_pass_through_the_scan(oracle, ctx, name):
    """C2 and C3: raw hit counts on either side of DCN_LDS_SET_MAX; `enough` in decisions-only mode"""
    W, oidx, proc, _ = ctx(31, 15)
    run_case(oracle, proc, oidx, W.by_name[name], W.keys)


@pytest.mark.parametrize("shift", ("0", "2"))
def test_the_set_limit_at_other_record_geometries(oracle, dcn, ctx, monkeypatch, shift):
    """C2 at DCN_REC_SHIFT 0 and 2"""
    W, oidx, _, gidx = ctx(31, 15)
    monkeypatch.setenv("DCN_REC_SHIFT", shift)
    proc = make_proc(dcn, gidx)
    for name in C_CASES[:3]:
        run_case(oracle, proc, oidx, W.by_name[name], W.keys)


def _both_modes(proc, case, thr):
    reads, uid = case.batch()
    b, o = F._oracle().concat_reads(reads)
    proc.abs_threshold, proc.rel_threshold, proc.deplete = thr
    return b, o, uid


def test_nothing_stale(oracle, dcn, monkeypatch):
    """C5: one context runs the batches of World(31, 15).stale_plan() -- A1 to A4 and A6 with their threshold batches, C2, C3
    and B1 to B3, each B batch under its own abs_threshold, so that decisions-only calls that return from the scan's early-out
    alternate with counting calls -- forwards, backwards and, after a batch whose run overflowed, shuffled.  The overflow:
    DCN_REC_SHIFT = 3 and a low-complexity unit whose one hash is a key; the rerun is seen as
    test_a_run_overflow_is_not_counted_twice sees it, DCN_ERR_CAPACITY at synchronize, then the same batch again.  Every
    batch's results equal its first results.  (A5, A7, C4: other contexts, made under their hooks; A8, C1: other entry points.)"""
    from test_gpu_short_fused import DeviceBatch
    W = F.world(31, 15)
    over, _ = W.overflow_case()
    cases, keys = W.stale_plan()
    oidx, gidx = index_pair(oracle, dcn, keys, 31, 15)
    monkeypatch.setenv("DCN_REC_SHIFT", "3")
    monkeypatch.setenv("DCN_QUIET", "1")
    proc = make_proc(dcn, gidx)
    plan = [(c, thr[i % len(thr)]) for i, (c, thr) in enumerate(cases)]

    def sweep(order):
        out = {}
        for i in order:
            c, thr = plan[i]
            b, o, uid = _both_modes(proc, c, thr)
            if i % 2:
                out[i, "keep"] = proc.filter_batch(b, o, uid, counts=False).tolist()
                out[i] = [x.tolist() for x in proc.filter_batch(b, o, uid)]
            else:
                out[i] = [x.tolist() for x in proc.filter_batch(b, o, uid)]
                out[i, "keep"] = proc.filter_batch(b, o, uid, counts=False).tolist()
        return out
    n = len(plan)
    first = sweep(range(n))
    for i, (c, thr) in enumerate(plan):
        keep, hits, total = F.expected(oracle, c, keys, *thr)
        assert first[i] == [keep, hits, total] and first[i, "keep"] == keep, c.name
    assert sweep(range(n - 1, -1, -1)) == first
    proc.abs_threshold, proc.rel_threshold, proc.deplete = 2, 0.01, False
    reads, uid = over.batch()
    batch = DeviceBatch(oracle, reads, uid)
    s0 = proc.stats()
    batch.enqueue(proc)
    with pytest.raises(dcn.DeaconHipError) as e:
        proc.synchronize()
    assert e.value.code == dcn._native.DCN_ERR_CAPACITY and proc.stats() == s0
    batch.enqueue(proc)
    proc.synchronize()
    keep, hits, total = batch.results()
    want = F.expected(oracle, over, keys, 2, 0.01, False)
    assert [keep.astype(bool).tolist(), hits.tolist(), total.tolist()] == [list(x) for x in want]
    order = list(np.random.default_rng(5).permutation(n))
    assert sweep(order) == first

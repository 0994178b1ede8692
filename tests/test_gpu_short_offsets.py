"""Short device batches scanned straight from the offsets (scan.hip, scan_short: read r is lane r % 64 of workgroup r // 64; no
plan pass) and counted by the scan kernel itself (the finish kernel visits only the units handed to the distinct pass), against
the CPU oracle: keep, hits, total and the six counters, bit-exact.  Every test asserts through last_batch_short() that its
batches took that path.  The batches and what they contain: tests/_short_offsets_cases.py."""
import numpy as np
import pytest

import _short_fused_cases as SC
import _short_offsets_cases as OC
from test_gpu_short_fused import DeviceBatch, make_proc, run_one

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def world(oracle, dcn):
    g = SC.genome()
    oidx = oracle.Index.build([g], k=SC.K, w=SC.W)
    gidx = dcn.Index.from_keys(oidx.keys(), SC.K, SC.W)
    return g, oidx, gidx


@pytest.fixture(scope="module")
def counters(world):
    return OC.counters_batch(world[0])


def add_stats(a, b):
    return {n: a[n] + b[n] for n in a}


# 1. lanes without a window at the wave's edges
@pytest.mark.parametrize("n", OC.EDGE_SIZES)
def test_lanes_without_a_window_at_the_edges(oracle, dcn, world, n):
    g, oidx, gidx = world
    run_one(oracle, dcn, oidx, gidx, OC.edge_batch(g, n), True)


def test_a_whole_wave_without_a_window(oracle, dcn, world):
    g, oidx, gidx = world
    run_one(oracle, dcn, oidx, gidx, OC.idle_wave_batch(g), True)


def test_a_batch_of_empty_reads(oracle, dcn, world):
    g, oidx, gidx = world
    run_one(oracle, dcn, oidx, gidx, OC.empty_batch(), True)


# 2. counters
@pytest.mark.parametrize("abs_t,rel_t,deplete", SC.THRESHOLDS)
def test_counters(oracle, dcn, world, counters, abs_t, rel_t, deplete):
    g, oidx, gidx = world
    run_one(oracle, dcn, oidx, gidx, counters, True, abs_threshold=abs_t, rel_threshold=rel_t, deplete=deplete)


# 3. a run overflow must not count twice
def test_a_run_overflow_is_not_counted_twice(oracle, dcn, world):
    g = world[0]
    oidx = oracle.Index.build([OC.overflow_genome(g)], k=SC.K, w=SC.W)
    gidx = dcn.Index.from_keys(oidx.keys(), SC.K, SC.W)
    proc = make_proc(dcn, gidx)
    before = DeviceBatch(oracle, OC.edge_batch(g, 129))
    before.enqueue(proc)
    proc.synchronize()
    assert proc.last_batch_short() is True
    s0 = proc.stats()
    assert s0 == SC.expected_stats(before.reads, before.check(oracle, oidx, proc)[0])
    batch = DeviceBatch(oracle, OC.overflow_batch(g))
    batch.enqueue(proc)
    with pytest.raises(dcn.DeaconHipError) as e:
        proc.synchronize()
    assert e.value.code == dcn._native.DCN_ERR_CAPACITY
    assert proc.stats() == s0, "the overflowed attempt was counted"
    batch.enqueue(proc)
    proc.synchronize()
    assert proc.last_batch_short() is True
    want = batch.check(oracle, oidx, proc)
    s1 = add_stats(s0, SC.expected_stats(batch.reads, want[0]))
    assert proc.stats() == s1, "the batch was not counted exactly once"
    after = DeviceBatch(oracle, OC.edge_batch(g, 128))
    after.enqueue(proc)
    proc.synchronize()
    assert proc.last_batch_short() is True
    assert proc.stats() == add_stats(s1, SC.expected_stats(after.reads, after.check(oracle, oidx, proc)[0]))


# 4. no stale counts or tiles
def test_no_stale_counts_or_tiles(oracle, dcn, world):
    g, oidx, gidx = world
    plan = OC.stale_plan(g)
    proc = make_proc(dcn, gidx)
    batches = [DeviceBatch(oracle, r) for r, _ in plan]
    for b in batches:  # no synchronize in between
        b.enqueue(proc)
    proc.synchronize()
    assert proc.last_batch_short() is True
    stats = {n: 0 for n in proc.stats()}
    for b in batches:
        stats = add_stats(stats, SC.expected_stats(b.reads, b.check(oracle, oidx, proc)[0]))
    assert proc.stats() == stats
    for (r, short), b in zip(plan, batches):  # each batch alone: the path it takes
        b.enqueue(proc)
        proc.synchronize()
        assert proc.last_batch_short() is short
        stats = add_stats(stats, SC.expected_stats(b.reads, b.check(oracle, oidx, proc)[0]))
    assert proc.stats() == stats
    # decreasing offsets: the error of the classic path, and nothing counted
    bad = DeviceBatch(oracle, plan[0][0][:300])
    o = bad.o.copy()
    o[100], o[101] = o[101], o[100]
    bad.d_o = torch.from_numpy(o.view(np.int64)).to(bad.d_b.device)
    torch.cuda.synchronize()
    bad.enqueue(proc)
    with pytest.raises(dcn.DeaconHipError) as e:
        proc.synchronize()
    assert e.value.code == dcn._native.DCN_ERR_ARG
    assert proc.last_batch_short() is False
    assert proc.stats() == stats
    good = DeviceBatch(oracle, plan[1][0])
    good.enqueue(proc)
    proc.synchronize()
    assert proc.last_batch_short() is True
    assert proc.stats() == add_stats(stats, SC.expected_stats(good.reads, good.check(oracle, oidx, proc)[0]))


# 5. the same bits with the path switched off
def test_bit_identity_with_the_switch(oracle, dcn, world, counters, monkeypatch):
    g, oidx, gidx = world
    for reads in [OC.edge_batch(g, n) for n in OC.EDGE_SIZES] + [OC.idle_wave_batch(g), OC.empty_batch(), counters]:
        out = {}
        for off in (True, False):
            if off:
                monkeypatch.setenv("DCN_NO_SHORT_FUSED", "1")
            else:
                monkeypatch.delenv("DCN_NO_SHORT_FUSED", raising=False)
            proc = make_proc(dcn, gidx)
            batch = DeviceBatch(oracle, reads)
            batch.enqueue(proc)
            proc.synchronize()
            assert proc.last_batch_short() is (not off)
            out[off] = (batch.results(), proc.stats())
        for x, y in zip(out[True][0], out[False][0]):
            assert x.tobytes() == y.tobytes()
        assert out[True][1] == out[False][1]

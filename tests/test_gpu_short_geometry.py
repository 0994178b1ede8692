"""The short path of the scan kernel (scan.hip, scan_short) and the W = 15 instantiation of scan_body at every kind of k
they serve, against the CPU oracle: keep, hits, total and the six counters, bit-exact.  Every test asserts through
last_batch_short() which path its batches took.  The bytes around the stream in device memory hold the genome that continues
the batch's first and last read: a kernel that took them for bases would report hits the oracle does not have.  The batches
and what they contain: tests/_short_geometry_cases.py."""
import pytest

import _short_fused_cases as SC
import _short_geometry_cases as GC
from test_gpu_short_fused import DeviceBatch, make_proc, run_one

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_worlds = {}


def world_of(oracle, dcn, k):
    """(genome, oracle index, device index, k_batch) of one k, built once"""
    if k not in _worlds:
        g, src = GC.world(k)
        oidx = oracle.Index.build(list(src), k=k, w=GC.W)
        gidx = dcn.Index.from_keys(oidx.keys(), k, GC.W)
        _worlds[k] = (g, oidx, gidx, GC.k_batch(g, k) if k in GC.KS else None)
    return _worlds[k]


def add_stats(a, b):
    return {n: a[n] + b[n] for n in a}


def one_slot_per_window(monkeypatch, k):
    """k = 1, 3: a read's hits outgrow a run of one slot per four bases (the context reads the variable at creation)"""
    if k in GC.ONE_SLOT_PER_WINDOW:
        monkeypatch.setenv("DCN_REC_SHIFT", "0")


# 1. every k on the short path
@pytest.mark.parametrize("k", GC.KS)
def test_every_k_on_the_short_path(oracle, dcn, monkeypatch, k):
    g, oidx, gidx, reads = world_of(oracle, dcn, k)
    one_slot_per_window(monkeypatch, k)
    for shift in (0, 9):
        for abs_t, rel_t, deplete in GC.THRESHOLDS:
            run_one(oracle, dcn, oidx, gidx, reads, True, shift=shift, outside=GC.outside(k, shift), abs_threshold=abs_t,
                    rel_threshold=rel_t, deplete=deplete)


# 2. the classic kernel of the same window size, and the same bits from both
@pytest.mark.parametrize("k", GC.KS)
def test_every_k_on_the_classic_w15_kernel(oracle, dcn, monkeypatch, k):
    g, oidx, gidx, reads = world_of(oracle, dcn, k)
    one_slot_per_window(monkeypatch, k)
    out = {}
    for off in (True, False):
        if off:
            monkeypatch.setenv("DCN_NO_SHORT_FUSED", "1")
        else:
            monkeypatch.delenv("DCN_NO_SHORT_FUSED", raising=False)
        batch, proc = run_one(oracle, dcn, oidx, gidx, reads, not off, shift=9, outside=GC.outside(k, 9))
        assert proc.last_batch_short() is (not off)
        out[off] = (batch.results(), proc.stats())
    for x, y in zip(out[True][0], out[False][0]):
        assert x.tobytes() == y.tobytes()
    assert out[True][1] == out[False][1]


# 3. the host API: always the classic path
@pytest.mark.parametrize("k", GC.KS)
def test_every_k_through_the_host_api(oracle, dcn, k):
    g, oidx, gidx, reads = world_of(oracle, dcn, k)
    b, o = oracle.concat_reads(reads)
    # (the default thresholds, under which every k keeps some reads and drops others; k = 1 and 3 outgrow their runs of the
    # record array here, and the host API runs such a batch again by itself)
    proc = make_proc(dcn, gidx)
    keep, hits, total = proc.filter_batch(b, o)
    want = oracle.filter_batch(oidx, b, o, threads=4)
    assert total.tolist() == want[2].tolist(), "total minimizers differ"
    assert hits.tolist() == want[1].tolist(), "distinct hit counts differ"
    assert keep.tolist() == want[0].tolist(), "keep decisions differ"
    assert want[0].any() and not want[0].all()
    assert proc.stats() == SC.expected_stats(reads, want[0])
    assert proc.last_batch_short() is False


# 4. k = 1 at one slot per four bases: the overflow is reported once and the batch counted once
def test_k1_overflow_is_reported_once_and_counted_once(oracle, dcn, monkeypatch):
    monkeypatch.delenv("DCN_REC_SHIFT", raising=False)
    g, oidx, gidx, reads = world_of(oracle, dcn, 1)
    proc = make_proc(dcn, gidx)
    s0 = proc.stats()
    assert not any(s0.values())
    batch = DeviceBatch(oracle, reads, shift=9, outside=GC.outside(1, 9))
    batch.enqueue(proc)
    with pytest.raises(dcn.DeaconHipError) as e:
        proc.synchronize()
    assert e.value.code == dcn._native.DCN_ERR_CAPACITY
    assert proc.stats() == s0, "the overflowed attempt was counted"
    batch.enqueue(proc)
    proc.synchronize()
    assert proc.last_batch_short() is True
    s1 = SC.expected_stats(batch.reads, batch.check(oracle, oidx, proc)[0])
    assert proc.stats() == s1, "the batch was not counted exactly once"
    after = DeviceBatch(oracle, reads[64:193])
    assert len(after.reads) == 129
    after.enqueue(proc)
    proc.synchronize()
    assert proc.last_batch_short() is True
    assert proc.stats() == add_stats(s1, SC.expected_stats(after.reads, after.check(oracle, oidx, proc)[0]))


# 5. the staging area: a full wave of longest reads, its first base at every position inside a 16-byte chunk
@pytest.mark.parametrize("j", range(16))
def test_full_waves_of_longest_reads(oracle, dcn, j):
    for k in (SC.K, 5) if j in (0, 7, 15) else (SC.K,):
        g, oidx, gidx, _ = world_of(oracle, dcn, k)
        reads = GC.full_wave_batch(g, j, k)
        for shift in (0, 15):
            run_one(oracle, dcn, oidx, gidx, reads, True, shift=shift, outside=GC.outside(k, shift))


# 6. the two fallbacks: a decisions-only call and tiles below the longest short read
def test_decisions_only_and_small_tiles_take_the_classic_path(oracle, dcn, monkeypatch):
    g, oidx, gidx, reads = world_of(oracle, dcn, 13)
    proc = make_proc(dcn, gidx, abs_threshold=2)
    only = DeviceBatch(oracle, reads, counts=False)
    only.enqueue(proc)
    proc.synchronize()
    assert proc.last_batch_short() is False
    want = only.check(oracle, oidx, proc)
    assert proc.stats() == SC.expected_stats(reads, want[0])
    counting = DeviceBatch(oracle, reads)  # the same processor, a counting call
    counting.enqueue(proc)
    proc.synchronize()
    assert proc.last_batch_short() is True
    counting.check(oracle, oidx, proc)
    assert proc.stats() == add_stats(SC.expected_stats(reads, want[0]), SC.expected_stats(reads, want[0]))
    monkeypatch.setenv("DCN_TILE_WINDOWS", "128")
    run_one(oracle, dcn, oidx, gidx, reads, False)
    monkeypatch.delenv("DCN_TILE_WINDOWS")
    run_one(oracle, dcn, oidx, gidx, reads, True)


# 7. no stale state between the paths at a k with a hit in most minimizers
def test_paths_alternate_on_one_context_at_small_k(oracle, dcn):
    k = 5
    g, oidx, gidx, _ = world_of(oracle, dcn, k)
    plan = GC.alternate_plan(g, k)
    proc = make_proc(dcn, gidx)
    batches = [DeviceBatch(oracle, r, u) for r, u, _ in plan]
    for b in batches:  # no synchronize in between
        b.enqueue(proc)
    proc.synchronize()
    assert proc.last_batch_short() is True
    wants = [b.check(oracle, oidx, proc) for b in batches]
    s1 = proc.stats()
    assert s1 == {n: sum(SC.expected_stats(r, w[0], u)[n] for (r, u, _), w in zip(plan, wants)) for n in s1}
    for (r, u, short), b in zip(plan, batches):  # each batch alone: the path it takes
        b.enqueue(proc)
        proc.synchronize()
        assert proc.last_batch_short() is short
        b.check(oracle, oidx, proc)
    s2 = proc.stats()
    assert {n: s2[n] - s1[n] for n in s1} == s1

"""Device batches of short unpaired reads, which the scan kernel packs itself (scan.hip, scan_short) behind the shape
kernel's verdict (plan.hip), against the CPU oracle: keep, hits, total and the six counters, bit-exact.  Every test that
expects that path asserts through FilterProcessor.last_batch_short() that the batch took it, every test that expects the
classic path that it did not.  The batches and what they contain: tests/_short_fused_cases.py.

The short path has no planning blocks: the plan kernel returns at once for a batch the shape kernel declared short, and read
r is lane r % 64 of workgroup r // 64 of the scan kernel, whatever the batch's size.  The batches here have a few thousand
reads.  The cases module still speaks of planning blocks of 256 reads: that is how the classic path lays out the same
batches when test 6 switches the short path off (blocks of 2,048 reads from 2^19 reads on, which only bench.py's oracle
checks of the 10 M-read headline batch reach).  last_batch_short() reports batches of the device-pointer API, which is what
every test here uses."""
import numpy as np
import pytest

import _short_fused_cases as SC
from conftest import random_reads

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def world(oracle, dcn):
    g = SC.genome()
    oidx = oracle.Index.build([g], k=SC.K, w=SC.W)
    gidx = dcn.Index.from_keys(oidx.keys(), SC.K, SC.W)
    return g, oidx, gidx


@pytest.fixture(scope="module")
def seam(world):
    return SC.seam_batch(world[0])


@pytest.fixture(scope="module")
def newline(world):
    return SC.newline_batch(world[0])


def make_proc(dcn, gidx, **kw):
    return dcn.FilterProcessor(gidx, max_batch_bases=1 << 21, max_batch_reads=1 << 13, **kw)


class DeviceBatch:
    """a batch in device memory, its bases `shift` bytes into their allocation.  outside = (front, back): what the `shift`
    bytes in front of the stream and the 64 bytes behind it hold instead of zeros"""

    def __init__(self, oracle, reads, unit_id=None, shift=0, counts=True, outside=None):
        self.reads, self.unit_id = reads, unit_id
        self.b, self.o = oracle.concat_reads(reads)
        dev = torch.device("cuda:0")
        self.buf = torch.zeros(len(self.b) + shift + 64, dtype=torch.uint8, device=dev)
        self.buf[shift:shift + len(self.b)] = torch.from_numpy(self.b).to(dev)
        if outside is not None:
            front, back = outside
            assert len(front) == shift and len(back) == 64
            around = np.frombuffer(bytes(front) + bytes(back), dtype=np.uint8).copy()
            self.buf[:shift] = torch.from_numpy(around[:shift]).to(dev)
            self.buf[shift + len(self.b):] = torch.from_numpy(around[shift:]).to(dev)
        self.d_b = self.buf[shift:]
        assert self.d_b.data_ptr() % 16 == shift % 16
        self.d_o = torch.from_numpy(self.o.view(np.int64)).to(dev)
        self.d_u = torch.from_numpy(unit_id.view(np.int32)).to(dev) if unit_id is not None else None
        self.n_units = int(unit_id[-1]) + 1 if unit_id is not None else len(reads)
        self.d_keep = torch.full((max(self.n_units, 1),), 7, dtype=torch.uint8, device=dev)
        self.d_hits = torch.full((max(self.n_units, 1),), -1, dtype=torch.int32, device=dev) if counts else None
        self.d_total = torch.full((max(self.n_units, 1),), -1, dtype=torch.int32, device=dev) if counts else None
        torch.cuda.synchronize()

    def enqueue(self, proc):
        proc.filter_batch_device(self.d_b.data_ptr(), self.d_o.data_ptr(), len(self.reads), len(self.b), self.d_keep.data_ptr(),
                                 self.d_hits.data_ptr() if self.d_hits is not None else None,
                                 self.d_total.data_ptr() if self.d_total is not None else None,
                                 d_unit_id=self.d_u.data_ptr() if self.d_u is not None else None, n_units=self.n_units)

    def results(self):
        keep = self.d_keep.cpu().numpy()[:self.n_units]
        if self.d_hits is None:
            return keep, None, None
        return keep, self.d_hits.cpu().numpy()[:self.n_units].astype(np.uint32), self.d_total.cpu().numpy()[:self.n_units].astype(np.uint32)

    def check(self, oracle, oidx, proc):
        want = oracle.filter_batch(oidx, self.b, self.o, self.unit_id, abs_threshold=proc.abs_threshold,
                                   rel_threshold=proc.rel_threshold, prefix_length=proc.prefix_length, deplete=proc.deplete, threads=4)
        keep, hits, total = self.results()
        if hits is not None:
            assert total.tolist() == want[2].tolist(), "total minimizers differ"
            assert hits.tolist() == want[1].tolist(), "distinct hit counts differ"
        assert keep.tolist() == want[0].astype(np.uint8).tolist(), "keep decisions differ"
        return want


def run_one(oracle, dcn, oidx, gidx, reads, short, unit_id=None, shift=0, outside=None, **kw):
    """one batch on a fresh processor: results and counters against the oracle, and the path it took"""
    proc = make_proc(dcn, gidx, **kw)
    batch = DeviceBatch(oracle, reads, unit_id, shift, outside=outside)
    batch.enqueue(proc)
    proc.synchronize()
    assert proc.last_batch_short() is short
    want = batch.check(oracle, oidx, proc)
    assert proc.stats() == SC.expected_stats(reads, want[0], unit_id)
    return batch, proc


# 1. wave and planning-block seams
def test_wave_and_block_seams(oracle, dcn, world, seam):
    g, oidx, gidx = world
    run_one(oracle, dcn, oidx, gidx, seam, True)


# 2. newlines
def test_trailing_and_inner_newlines(oracle, dcn, world, newline):
    g, oidx, gidx = world
    run_one(oracle, dcn, oidx, gidx, newline, True)


# 3. alignment and stream ends
@pytest.mark.parametrize("shift", [1, 7, 15])
def test_any_alignment_of_the_bases(oracle, dcn, world, newline, shift):
    g, oidx, gidx = world
    run_one(oracle, dcn, oidx, gidx, newline, True, shift=shift)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_batches_and_the_stream_front(oracle, dcn, world, seam, n):
    """the first read starts at stream offset 0: its lead-in lies in front of the stream"""
    g, oidx, gidx = world
    reads = [g[100:100 + SC.LMAX]] + [r for r in seam if len(r) >= SC.L][:n - 1]
    for shift in (0, 3):
        run_one(oracle, dcn, oidx, gidx, reads, True, shift=shift)


# 4. falling back
def test_one_longer_read_takes_the_classic_path(oracle, dcn, world, seam):
    g, oidx, gidx = world
    reads = list(seam[:700])
    reads[333] = g[9000:9000 + SC.LMAX + 1]
    run_one(oracle, dcn, oidx, gidx, reads, False)
    reads[333] = g[9000:9000 + SC.LMAX]
    run_one(oracle, dcn, oidx, gidx, reads, True)


def test_pairs_take_the_classic_path(oracle, dcn, world, seam):
    g, oidx, gidx = world
    reads = seam[:700]
    run_one(oracle, dcn, oidx, gidx, reads, False, unit_id=(np.arange(len(reads)) // 2).astype(np.uint32))


def test_a_prefix_takes_the_classic_path(oracle, dcn, world, seam):
    g, oidx, gidx = world
    run_one(oracle, dcn, oidx, gidx, seam[:700], False, prefix_length=50)


@pytest.mark.parametrize("k,w", [(33, 15), (31, 11)])
def test_other_geometries_take_the_classic_path(oracle, dcn, world, k, w):
    g = world[0]
    oidx = oracle.Index.build([g], k=k, w=w)
    gidx = dcn.Index.from_keys(oidx.keys(), k, w)
    rng = np.random.default_rng(7)
    reads = [SC._read(rng, g, int(rng.integers(40, SC.LMAX + 1)), rng.random() < 0.5) for _ in range(500)]
    run_one(oracle, dcn, oidx, gidx, reads, False)


def test_bad_offsets_are_reported_as_before(oracle, dcn, world, seam):
    g, oidx, gidx = world
    proc = make_proc(dcn, gidx)
    batch = DeviceBatch(oracle, seam[:300])
    o = batch.o.copy()
    o[100], o[101] = o[101], o[100]  # decreasing
    batch.d_o = torch.from_numpy(o.view(np.int64)).to(batch.d_b.device)
    torch.cuda.synchronize()
    batch.enqueue(proc)
    with pytest.raises(dcn.DeaconHipError) as e:
        proc.synchronize()
    assert e.value.code == dcn._native.DCN_ERR_ARG
    assert proc.last_batch_short() is False
    good = DeviceBatch(oracle, seam[:300])  # the context stays usable
    good.enqueue(proc)
    proc.synchronize()
    assert proc.last_batch_short() is True
    good.check(oracle, oidx, proc)


# 5. no stale state between batches of different kinds
def test_no_stale_state_between_paths(oracle, dcn, world, seam, newline):
    g, oidx, gidx = world
    rng = np.random.default_rng(11)
    long_reads = [SC._read(rng, g, int(rng.integers(500, 3000)), True) for _ in range(40)]
    paired = seam[1100:1500]
    uid = (np.arange(len(paired)) // 2).astype(np.uint32)
    plan = [(seam[:900], None, True), (long_reads, None, False), (newline, None, True), (paired, uid, False),
            (seam[2000:2700], None, True)]
    proc = make_proc(dcn, gidx)
    batches = [DeviceBatch(oracle, r, u) for r, u, _ in plan]
    for b in batches:  # no synchronize in between
        b.enqueue(proc)
    proc.synchronize()
    assert proc.last_batch_short() is True
    wants = [b.check(oracle, oidx, proc) for b in batches]
    s1 = proc.stats()
    want_stats = {n: sum(SC.expected_stats(r, w[0], u)[n] for (r, u, _), w in zip(plan, wants)) for n in s1}
    assert s1 == want_stats
    # each batch alone: the path it takes
    for (r, u, short), b in zip(plan, batches):
        b.enqueue(proc)
        proc.synchronize()
        assert proc.last_batch_short() is short
    s2 = proc.stats()
    # the same sequence, counting and decisions-only calls interleaved
    both = []
    for r, u, _ in plan:
        both += [DeviceBatch(oracle, r, u), DeviceBatch(oracle, r, u, counts=False)]
    for b in both:
        b.enqueue(proc)
    proc.synchronize()
    for b in both:
        b.check(oracle, oidx, proc)
    s3 = proc.stats()
    assert {n: s3[n] - s2[n] for n in s1} == {n: 2 * s1[n] for n in s1}, "counters differ between the two modes"
    assert {n: s2[n] - s1[n] for n in s1} == s1


# 6. the same bits with the path switched off
def test_bit_identity_with_the_switch(oracle, dcn, world, seam, newline, monkeypatch):
    g, oidx, gidx = world
    for reads in (seam, newline):
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


# 7. thresholds
@pytest.mark.parametrize("abs_t,rel_t,deplete", SC.THRESHOLDS)
def test_thresholds(oracle, dcn, world, seam, abs_t, rel_t, deplete):
    g, oidx, gidx = world
    run_one(oracle, dcn, oidx, gidx, seam, True, abs_threshold=abs_t, rel_threshold=rel_t, deplete=deplete)

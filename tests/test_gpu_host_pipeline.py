"""GPU parity tests of the pipelined host entry points, all through the C ABI and all against the CPU oracle:
chunked copy/compute overlap inside dcn_filter_batch, dcn_filter_batch_submit / _wait with two batches in flight,
2-bit packed input (dcn_filter_batch_packed, dcn_pack_ascii), the sticky record-overflow word of the
device-pointer API, and the in-process multi-context pieces (dcn_index_clone, dcn_stats_allreduce)."""
import os

import numpy as np
import pytest

from conftest import random_reads
from test_gpu_parity import make_index_pair, sample_reads

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["lean", "three-streams"])
def submission_form(request, monkeypatch):
    """every test of this file twice: batches of up to 16 Mbp that fit one chunk are submitted on ONE stream in their plain
    form (64-bit offsets, whole mask words; host_batch.hip submit_impl, `lean`), larger or chunked ones with copies, kernels and result
    copies on three streams; DCN_LEAN_MAX_BASES=0 sends everything the second way, so that narrow offsets, the sparse mask and
    the events between the streams are tested at test sizes too"""
    if request.param == "three-streams":
        monkeypatch.setenv("DCN_LEAN_MAX_BASES", "0")
    return request.param


@pytest.fixture(scope="module")
def genome():
    return random_reads(np.random.default_rng(101), 1, 150_000, 150_000)[0]


@pytest.fixture(scope="module")
def index_pair(oracle, dcn, genome):
    return make_index_pair(oracle, dcn, [genome])


def small_chunks(monkeypatch, n=20_000):
    """contexts created afterwards cut host batches every ~n bases"""
    monkeypatch.setenv("DCN_CHUNK_BASES", str(n))


def mixed_reads(rng, genome, n_short=3000, n_long=12):
    reads = sample_reads(rng, genome, n_short, 30, 400)
    for _ in range(n_long):  # long reads straddle many chunks' worth of tiles
        ln = int(rng.integers(5_000, 60_000))
        s = int(rng.integers(0, len(genome) - ln))
        reads.insert(int(rng.integers(0, len(reads))), genome[s:s + ln])
    reads.insert(7, b"")
    reads.insert(8, b"ACGT")
    return reads


def oracle_batch(oracle, oidx, proc, b, o, uid):
    return oracle.filter_batch(oidx, b, o, uid, abs_threshold=proc.abs_threshold, rel_threshold=proc.rel_threshold,
                               prefix_length=proc.prefix_length, deplete=proc.deplete, threads=4)


def assert_same(got, want):
    assert got[2].tolist() == want[2].tolist(), "total minimizers differ"
    assert got[1].tolist() == want[1].tolist(), "distinct hit counts differ"
    assert got[0].tolist() == want[0].tolist(), "keep decisions differ"


@pytest.mark.parametrize("pinned", [False, True, "dma"])
@pytest.mark.parametrize("paired", [False, True])
def test_chunked_batch_matches_oracle(oracle, dcn, genome, index_pair, monkeypatch, pinned, paired):
    """a batch cut into dozens of chunks (pageable: host-packed into the staging ring; page-locked: the same where the
    host packs with AVX-512, else -- and always with DCN_PINNED_ASCII_DMA, the "dma" case -- ASCII DMA + device pack)
    gives the oracle's results, chunk seams inside and between units included"""
    small_chunks(monkeypatch)
    if pinned == "dma":
        monkeypatch.setenv("DCN_PINNED_ASCII_DMA", "1")
    oidx, gidx = index_pair
    rng = np.random.default_rng(102 + bool(pinned) + 2 * paired)
    reads = mixed_reads(rng, genome)
    b, o = oracle.concat_reads(reads)
    uid = (np.arange(len(reads)) // 2).astype(np.uint32) if paired else None
    proc = dcn.FilterProcessor(gidx, deplete=paired, max_batch_bases=len(b) + 100, max_batch_reads=len(reads) + 8)
    want = oracle_batch(oracle, oidx, proc, b, o, uid)
    if pinned:
        pb, po = dcn.PinnedBuffer(len(b), np.uint8), dcn.PinnedBuffer(len(o), np.uint64)
        pb.array[:], po.array[:] = b, o
        got = proc.filter_batch(pb.array, po.array, uid)
    else:
        got = proc.filter_batch(b, o, uid)
    assert_same(got, want)
    s = proc.stats()
    assert s["total_seqs"] == len(reads) and s["total_bp"] == len(b)
    assert len(reads) % 2 == 0
    assert s["output_seq_counter"] == (2 if paired else 1) * int(want[0].sum())
    # decisions only, same chunks
    assert proc.filter_batch(b, o, uid, counts=False).tolist() == want[0].tolist()
    proc.close()


@pytest.mark.parametrize("mode", ["tiny-cap", "off"])
def test_invalid_mask_sparse_and_whole(oracle, dcn, genome, index_pair, monkeypatch, mode):
    """the invalid-base mask of a packed stream crosses the link as its non-zero words only; a batch whose words do not fit
    the pair buffer (here: room for 40 pairs, so the first chunks go sparse and the rest whole) and the form switched off give
    the same results, for the library's own pack and for a caller-packed batch, N-rich reads included"""
    small_chunks(monkeypatch, 30_000)
    if mode == "tiny-cap":
        monkeypatch.setenv("DCN_SPARSE_MASK_CAP", "40")
    else:
        monkeypatch.setenv("DCN_NO_SPARSE_MASK", "1")
    oidx, gidx = index_pair
    rng = np.random.default_rng(171)
    reads = mixed_reads(rng, genome, 1500, 5)
    reads += [bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), 400, p=[0.2, 0.2, 0.2, 0.2, 0.2])) for _ in range(40)]
    b, o = oracle.concat_reads(reads)
    proc = dcn.FilterProcessor(gidx, max_batch_bases=len(b) + 64, max_batch_reads=len(reads))
    want = oracle_batch(oracle, oidx, proc, b, o, None)
    assert_same(proc.filter_batch(b, o), want)
    packed, mask = dcn.pack_ascii(b)
    assert int(np.count_nonzero(mask)) > 40
    assert_same(proc.filter_batch_packed(packed, mask, o), want)
    proc.close()


@pytest.mark.parametrize("host_pack", [True, False])
def test_small_staging_ring_many_pieces_per_chunk(oracle, dcn, genome, index_pair, monkeypatch, host_pack):
    """pageable input through 8 KB staging buffers: every chunk's payload (host-packed stream + mask, or ASCII with
    DCN_NO_HOST_PACK), offsets and unit ids pass through the three-buffer ring in dozens of pieces, the ring wraps
    many times, and two batches in flight share it"""
    small_chunks(monkeypatch, 150_000)
    monkeypatch.setenv("DCN_STAGE_BYTES", "8192")
    if not host_pack:
        monkeypatch.setenv("DCN_NO_HOST_PACK", "1")
    oidx, gidx = index_pair
    rng = np.random.default_rng(150 + host_pack)
    reads = mixed_reads(rng, genome, 2000, 5)
    b, o = oracle.concat_reads(reads)
    uid = (np.arange(len(reads)) // 2).astype(np.uint32)
    proc = dcn.FilterProcessor(gidx, deplete=True, max_batch_bases=len(b) + 64, max_batch_reads=len(reads))
    want = oracle_batch(oracle, oidx, proc, b, o, uid)
    want1 = oracle_batch(oracle, oidx, proc, b, o, None)
    p1 = proc.submit(b, o, uid)
    p2 = proc.submit(b, o, None)
    assert_same(p1.wait(), want)
    assert_same(p2.wait(), want1)
    packed, mask = dcn.pack_ascii(b)
    assert_same(proc.filter_batch_packed(packed, mask, o, uid), want)  # pageable packed input: staged piecewise too
    proc.close()


def test_empty_batches_between_real_ones(oracle, dcn, genome, index_pair):
    """a batch without reads has no chunk: its report must still be this batch's (all zero), not the previous one's"""
    oidx, gidx = index_pair
    reads = sample_reads(np.random.default_rng(160), genome, 800, 50, 200)
    b, o = oracle.concat_reads(reads)
    proc = dcn.FilterProcessor(gidx, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    want = oracle_batch(oracle, oidx, proc, b, o, None)
    empty_b, empty_o = np.zeros(0, np.uint8), np.zeros(1, np.uint64)
    for _ in range(3):
        assert_same(proc.filter_batch(b, o), want)
        for _ in range(4):
            k = proc.submit(empty_b, empty_o, counts=False).wait()
            assert len(k) == 0
    s = proc.stats()
    assert s["total_seqs"] == 3 * len(reads) and s["total_bp"] == 3 * len(b)
    proc.close()


def test_submit_wait_two_in_flight(oracle, dcn, genome, index_pair, monkeypatch):
    small_chunks(monkeypatch, 50_000)
    oidx, gidx = index_pair
    rng = np.random.default_rng(110)
    batches = []
    for i in range(5):
        reads = sample_reads(rng, genome, 1500 + 200 * i, 40, 300)
        b, o = oracle.concat_reads(reads)
        uid = (np.arange(len(reads)) // 2).astype(np.uint32) if i % 2 else None
        batches.append((b, o, uid))
    proc = dcn.FilterProcessor(gidx, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    wants = [oracle_batch(oracle, oidx, proc, *x) for x in batches]
    pending = [proc.submit(*batches[0]), proc.submit(*batches[1])]
    with pytest.raises(dcn.DeaconHipError) as e:  # a third one without a wait
        proc.submit(*batches[2])
    assert e.value.code == dcn._native.DCN_ERR_CAPACITY
    with pytest.raises(dcn.DeaconHipError):  # the device-pointer API and the dump seam refuse while batches fly
        proc.minimizer_hashes_batch(batches[0][0], batches[0][1])
    results = []
    for nxt in (2, 3, 4):
        results.append(pending.pop(0).wait())
        pending.append(proc.submit(*batches[nxt], counts=nxt != 3))
    # out-of-order wait of the last two
    last = pending[1].wait()
    results.append(pending[0].wait())
    results.append(last)
    for i, (got, want) in enumerate(zip(results, wants)):
        if i == 3:
            assert got.tolist() == want[0].tolist()
        else:
            assert_same(got, want)
    s = proc.stats()
    assert s["total_seqs"] == sum(len(x[1]) - 1 for x in batches)
    assert s["total_bp"] == sum(len(x[0]) for x in batches)
    with pytest.raises(dcn.DeaconHipError):
        dcn._native.check(dcn._native.lib().dcn_filter_batch_wait(proc._h, 12345))
    proc.close()


@pytest.mark.parametrize("paired", [False, True])
def test_packed_input(oracle, dcn, genome, index_pair, monkeypatch, paired):
    """dcn_filter_batch_packed on the stream dcn_pack_ascii produces == the oracle on the ASCII"""
    small_chunks(monkeypatch, 30_000)
    oidx, gidx = index_pair
    rng = np.random.default_rng(120 + paired)
    reads = mixed_reads(rng, genome, 2500, 6)
    reads += random_reads(rng, 200, 60, 200, p_n=0.02, p_lower=0.3, alphabet=b"ACGTNRYKM")
    b, o = oracle.concat_reads(reads)
    uid = (np.arange(len(reads)) // 2).astype(np.uint32) if paired else None
    packed, mask = dcn.pack_ascii(b)
    for prefix in (0, 120):
        proc = dcn.FilterProcessor(gidx, prefix_length=prefix, deplete=not paired, max_batch_bases=len(b) + 64,
                                   max_batch_reads=len(reads))
        want = oracle_batch(oracle, oidx, proc, b, o, uid)
        assert_same(proc.filter_batch_packed(packed, mask, o, uid), want)
        assert proc.filter_batch_packed(packed, mask, o, uid, counts=False).tolist() == want[0].tolist()
        # page-locked packed buffers: straight DMA
        pp, pm = dcn.PinnedBuffer(len(packed), np.uint32), dcn.PinnedBuffer(len(mask), np.uint32)
        pp.array[:], pm.array[:] = packed, mask
        assert_same(proc.filter_batch_packed(pp.array, pm.array, o, uid), want)
        proc.close()
    with pytest.raises(ValueError):
        dcn.FilterProcessor(gidx, max_batch_bases=1 << 20, max_batch_reads=1 << 12).filter_batch_packed(
            packed[:10], mask, o, uid)


def test_trailing_newline_reads_through_the_host_packed_path(oracle, dcn, genome, index_pair, monkeypatch):
    """src/filter_common.rs:229 strips one trailing newline; the host-packed transport cannot see read ends, so a
    batch holding any newline byte is sent again as ASCII"""
    small_chunks(monkeypatch, 40_000)
    oidx, gidx = index_pair
    rng = np.random.default_rng(130)
    reads = sample_reads(rng, genome, 1200, 45, 200)
    for i in range(0, len(reads), 7):
        reads[i] = reads[i] + b"\n"
    reads[3] = reads[3][:20] + b"\n" + reads[3][21:]  # one in the middle too: an invalid base, not stripped
    b, o = oracle.concat_reads(reads)
    for prefix in (0, 100):
        proc = dcn.FilterProcessor(gidx, prefix_length=prefix, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
        want = oracle_batch(oracle, oidx, proc, b, o, None)
        assert_same(proc.filter_batch(b, o), want)
        pb = dcn.PinnedBuffer(len(b), np.uint8)
        pb.array[:] = b
        assert_same(proc.filter_batch(pb.array, o), want)
        proc.close()


def test_record_overflow_in_a_pipelined_batch_is_rerun(oracle, dcn, genome, index_pair, monkeypatch):
    """long reads overflow the small default record scratch of a small context in some chunks; wait() grows it and
    runs the batch again, counters counted once"""
    small_chunks(monkeypatch, 100_000)
    monkeypatch.setenv("DCN_RECORD_CAPACITY", "64")  # no room for the global sets of units with > 2800 hits
    oidx, gidx = index_pair
    reads = [genome[i * 10_000:i * 10_000 + 60_000] for i in range(8)] + [genome[:50_000]] * 2
    reads += sample_reads(np.random.default_rng(131), genome, 500, 50, 150)
    b, o = oracle.concat_reads(reads)
    proc = dcn.FilterProcessor(gidx, max_batch_bases=len(b) + 64, max_batch_reads=1 << 10)
    want = oracle_batch(oracle, oidx, proc, b, o, None)
    p1 = proc.submit(b, o)
    p2 = proc.submit(b, o)
    assert_same(p1.wait(), want)
    assert_same(p2.wait(), want)
    s = proc.stats()
    assert s["total_seqs"] == 2 * len(reads) and s["total_bp"] == 2 * len(b)
    proc.close()


def test_sticky_overflow_of_the_device_pointer_api(oracle, dcn, genome, index_pair, monkeypatch):
    """an overflow in batch N must not be erased by the status clearing of batch N+1"""
    torch = pytest.importorskip("torch")
    monkeypatch.setenv("DCN_RECORD_CAPACITY", "64")
    oidx, gidx = index_pair
    dev = torch.device("cuda:0")
    big = [genome[:120_000]] * 6
    small = [genome[100:250]] * 4
    proc = dcn.FilterProcessor(gidx, max_batch_bases=1 << 20, max_batch_reads=64)
    bufs = []
    for reads in (big, small):
        b, o = oracle.concat_reads(reads)
        d_b, d_o = torch.from_numpy(b).to(dev), torch.from_numpy(o.view(np.int64)).to(dev)
        d_k = torch.zeros(len(reads), dtype=torch.uint8, device=dev)
        d_h = torch.zeros(len(reads), dtype=torch.int32, device=dev)
        d_t = torch.zeros(len(reads), dtype=torch.int32, device=dev)
        bufs.append((reads, b, o, d_b, d_o, d_k, d_h, d_t))
    torch.cuda.synchronize()

    def enqueue(x):
        reads, b, o, d_b, d_o, d_k, d_h, d_t = x
        proc.filter_batch_device(d_b.data_ptr(), d_o.data_ptr(), len(reads), len(b), d_k.data_ptr(), d_h.data_ptr(),
                                 d_t.data_ptr())

    enqueue(bufs[0])
    enqueue(bufs[1])
    with pytest.raises(dcn.DeaconHipError) as e:
        proc.synchronize()
    assert e.value.code == dcn._native.DCN_ERR_CAPACITY
    proc.reserve_records(1 << 20)
    proc.reset_stats()
    enqueue(bufs[0])
    enqueue(bufs[1])
    proc.synchronize()
    for reads, b, o, d_b, d_o, d_k, d_h, d_t in bufs:
        want = oracle.filter_batch(oidx, b, o, None, threads=2)
        assert d_h.cpu().numpy().tolist() == want[1].tolist()
        assert d_k.cpu().numpy().astype(bool).tolist() == want[0].tolist()
    assert proc.stats()["total_seqs"] == len(big) + len(small)
    proc.close()


def test_device_pointer_batch_with_offsets_that_were_never_written(oracle, dcn, genome, index_pair):
    """Nobody looks at the offsets of a device-pointer batch before the GPU does (the host entry points validate theirs).  An
    array that is not the offsets yet when the kernels run -- a producer on another stream that was not waited for (found that
    way: profiles/placement_probe2.py, a memory fault), leftovers of another allocation -- must end in DCN_ERR_ARG at the next
    synchronize, with every read of a bad range planned as empty, not in tiles that point outside the batch's buffers; the
    context is as good as new afterwards."""
    torch = pytest.importorskip("torch")
    oidx, gidx = index_pair
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(11)
    reads = [genome[s:s + 150] for s in rng.integers(0, len(genome) - 150, 3000).tolist()] + [genome[:40_000]]
    b, o = oracle.concat_reads(reads)
    n = len(reads)
    d_b = torch.from_numpy(b).to(dev)
    d_good = torch.from_numpy(o.view(np.int64)).to(dev)
    d_k = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_h = torch.zeros(n, dtype=torch.int32, device=dev)
    d_t = torch.zeros(n, dtype=torch.int32, device=dev)
    proc = dcn.FilterProcessor(gidx, max_batch_bases=1 << 20, max_batch_reads=4096)
    bad_arrays = {
        "leftovers": rng.integers(0, 2**63 - 1, n + 1, dtype=np.int64),                   # whatever was in that memory
        "decreasing": o.view(np.int64)[::-1].copy(),
        "beyond the batch": o.view(np.int64) + np.int64(len(b)),
        "one bad read": np.concatenate([o.view(np.int64)[:1500], [np.int64(7)], o.view(np.int64)[1501:]]),
        "all ones": np.full(n + 1, -1, dtype=np.int64),
    }
    want = oracle.filter_batch(oidx, b, o, None, threads=2)
    for name, arr in bad_arrays.items():
        d_bad = torch.from_numpy(np.ascontiguousarray(arr)).to(dev)
        torch.cuda.synchronize()
        proc.filter_batch_device(d_b.data_ptr(), d_bad.data_ptr(), n, len(b), d_k.data_ptr(), d_h.data_ptr(), d_t.data_ptr())
        with pytest.raises(dcn.DeaconHipError) as e:
            proc.synchronize()
        assert e.value.code == dcn._native.DCN_ERR_ARG and "d_offsets" in str(e.value), name
        proc.synchronize()  # (reported once)
        # the same context, the real offsets: results as if nothing had happened
        proc.reset_stats()
        proc.filter_batch_device(d_b.data_ptr(), d_good.data_ptr(), n, len(b), d_k.data_ptr(), d_h.data_ptr(), d_t.data_ptr())
        proc.synchronize()
        assert d_k.cpu().numpy().astype(bool).tolist() == want[0].tolist(), name
        assert d_h.cpu().numpy().tolist() == want[1].tolist(), name
        assert d_t.cpu().numpy().tolist() == want[2].tolist(), name
        assert proc.stats()["total_seqs"] == n and proc.stats()["total_bp"] == len(b), name
    # unit ids nobody has looked at either: 0, then equal or +1, ending at n_units - 1 -- anything else is refused
    uid = (np.arange(n, dtype=np.uint32) // 2).astype(np.uint32)
    n_units = int(uid[-1]) + 1
    want = oracle.filter_batch(oidx, b, o, uid, threads=2)
    gap = uid.copy()
    gap[2000:] += 1                                  # unit 1000 has no read: its first-read entry would be a stale one
    bad_ids = {
        "beyond the units": uid + np.uint32(n_units),
        "leftovers": rng.integers(0, 2**32 - 1, n, dtype=np.uint32),
        "decreasing": uid[::-1].copy(),
        "a unit without a read": np.minimum(gap, np.uint32(n_units - 1)),
        "does not start at 0": np.maximum(uid, np.uint32(1)),
        "stops short": np.minimum(uid, np.uint32(n_units - 2)),
    }
    d_uid = torch.from_numpy(uid.view(np.int32)).to(dev)
    for name, arr in bad_ids.items():
        d_bad = torch.from_numpy(np.ascontiguousarray(arr).view(np.int32)).to(dev)
        torch.cuda.synchronize()
        proc.filter_batch_device(d_b.data_ptr(), d_good.data_ptr(), n, len(b), d_k.data_ptr(), d_h.data_ptr(), d_t.data_ptr(),
                                 d_unit_id=d_bad.data_ptr(), n_units=n_units)
        with pytest.raises(dcn.DeaconHipError) as e:
            proc.synchronize()
        assert e.value.code == dcn._native.DCN_ERR_ARG, name
        proc.reset_stats()
        proc.filter_batch_device(d_b.data_ptr(), d_good.data_ptr(), n, len(b), d_k.data_ptr(), d_h.data_ptr(), d_t.data_ptr(),
                                 d_unit_id=d_uid.data_ptr(), n_units=n_units)
        proc.synchronize()
        assert d_k.cpu().numpy()[:n_units].astype(bool).tolist() == want[0].tolist(), name
        assert d_h.cpu().numpy()[:n_units].tolist() == want[1].tolist(), name
        assert d_t.cpu().numpy()[:n_units].tolist() == want[2].tolist(), name
        assert proc.stats()["total_seqs"] == n and proc.stats()["total_bp"] == len(b), name
    proc.close()


def test_runs_of_the_record_array_grow_when_a_batch_fills_them(oracle, dcn, monkeypatch):
    """The record array keeps one slot per four windows (2 B per base instead of 8: VERDICT r2, weak 11).  A unit with a hit
    in more than every fourth window of a wave cannot be real sequence at w = 15, but w = 1 makes every k-mer a minimizer:
    reads of the indexed genome then hit in every window.  The host entry points run such a batch again with one slot
    per window; the device-pointer API reports it at synchronize, switches the context over, and the batch enqueued
    again comes out right.  DCN_REC_SHIFT=0 starts a context that way."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(17)
    genome = random_reads(rng, 1, 60_000, 60_000)[0]
    oidx = oracle.Index.build([genome], k=31, w=1)
    gidx = dcn.Index.from_keys(oidx.keys(), 31, 1)
    reads = [genome[s:s + n] for s, n in ((0, 9_000), (10_000, 3_000), (20_000, 700), (30_000, 20_000))] + random_reads(rng, 20, 100, 3_000)
    reads += [genome[100:130], genome[200:231], genome[300:340]]  # 0, 1 and 10 windows: tails far smaller than a slot
    b, o = oracle.concat_reads(reads)
    want = oracle.filter_batch(oidx, b, o, None, threads=2)
    assert want[1][0] > 8_000 and want[1][-2] == 1
    for shift in (None, "0", "2", "3"):  # (None: a context of an index with w <= 7 starts with one slot per window by itself)
        if shift is None:
            monkeypatch.delenv("DCN_REC_SHIFT", raising=False)
        else:
            monkeypatch.setenv("DCN_REC_SHIFT", shift)
        proc = dcn.FilterProcessor(gidx, max_batch_bases=len(b) + 64, max_batch_reads=len(reads) + 1)
        for _ in range(2):  # the second call finds the context already switched over
            got = proc.filter_batch(b, o)
            assert all(g.tolist() == w.tolist() for g, w in zip(got, want)), shift
        assert proc.filter_batch(b, o, counts=False).tolist() == want[0].tolist()
        assert proc.stats()["total_seqs"] == 3 * len(reads)  # an overflowed attempt is not counted
        proc.close()
    monkeypatch.setenv("DCN_REC_SHIFT", "2")  # the geometry contexts of a w >= 8 index start with: the switch-over is under test
    dev = torch.device("cuda:0")
    d_b, d_o = torch.from_numpy(b).to(dev), torch.from_numpy(o.view(np.int64)).to(dev)
    d_k = torch.zeros(len(reads), dtype=torch.uint8, device=dev)
    d_h = torch.zeros(len(reads), dtype=torch.int32, device=dev)
    d_t = torch.zeros(len(reads), dtype=torch.int32, device=dev)
    proc = dcn.FilterProcessor(gidx, max_batch_bases=len(b) + 64, max_batch_reads=len(reads) + 1)
    proc.filter_batch_device(d_b.data_ptr(), d_o.data_ptr(), len(reads), len(b), d_k.data_ptr(), d_h.data_ptr(), d_t.data_ptr())
    with pytest.raises(dcn.DeaconHipError, match="one slot per window") as e:
        proc.synchronize()
    assert e.value.code == dcn._native.DCN_ERR_CAPACITY
    proc.reset_stats()
    proc.filter_batch_device(d_b.data_ptr(), d_o.data_ptr(), len(reads), len(b), d_k.data_ptr(), d_h.data_ptr(), d_t.data_ptr())
    proc.synchronize()
    assert d_h.cpu().numpy().tolist() == want[1].tolist() and d_k.cpu().numpy().astype(bool).tolist() == want[0].tolist()
    assert d_t.cpu().numpy().tolist() == want[2].tolist() and proc.stats()["total_seqs"] == len(reads)
    proc.close()


def test_index_clone_and_stats_allreduce(oracle, dcn, genome, index_pair):
    oidx, gidx = index_pair
    clone = gidx.clone(0)  # same device on the 1-GPU box: the device-to-device copy path
    assert clone.header() == gidx.header()
    keys = oidx.keys()
    assert clone.contains(keys).all() and not clone.contains(keys ^ np.uint64(1)).all()
    rng = np.random.default_rng(140)
    reads = sample_reads(rng, genome, 2000, 50, 250)
    b, o = oracle.concat_reads(reads)
    p1 = dcn.FilterProcessor(gidx, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    p2 = dcn.FilterProcessor(clone, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    half = 1000
    a = p1.filter_batch(b[:int(o[half])], o[:half + 1])
    c = p2.filter_batch(b[int(o[half]):], o[half:] - o[half])
    want = oracle.filter_batch(oidx, b, o, None, threads=2)
    assert np.concatenate([a[0], c[0]]).tolist() == want[0].tolist()
    assert np.concatenate([a[1], c[1]]).tolist() == want[1].tolist()
    tot = dcn.stats_allreduce([p1, p2])
    assert tot["total_seqs"] == len(reads) and tot["total_bp"] == len(b)
    assert tot["output_seq_counter"] == int(want[0].sum())
    with pytest.raises(dcn.DeaconHipError):
        gidx.clone(99)


@pytest.mark.parametrize("n_keys", [0, 1, 200_000])
def test_index_clone_by_keys_is_the_same_set(oracle, dcn, n_keys, monkeypatch):
    """A replica on ANOTHER GPU is made from the compacted keys (a tenth of the table's bytes over xGMI), not from the table:
    dcn_table_clone_by_keys.  On the one-GPU box DCN_CLONE_BY_KEYS=1 sends a same-device clone down that path (export kernel,
    peer copy of the key array, insert into an empty table of the same geometry): same header, same key set (incl. key 0),
    same answers; the copy form beside it."""
    rng = np.random.default_rng(141 + n_keys)
    keys = np.unique(rng.integers(1, 2**63, n_keys, dtype=np.int64).astype(np.uint64))
    if n_keys > 1:
        keys = np.concatenate([keys, np.array([0, 2**64 - 1], np.uint64)])  # key 0 lives in a flag, not in a slot
    src = dcn.Index.from_keys(keys, 31, 15, device=0)
    monkeypatch.setenv("DCN_CLONE_BY_KEYS", "1")
    by_keys = src.clone(0)
    monkeypatch.delenv("DCN_CLONE_BY_KEYS")
    by_copy = src.clone(0)
    probe = np.concatenate([keys, keys ^ np.uint64(1), rng.integers(0, 2**63, 1000, dtype=np.int64).astype(np.uint64)])
    for rep in (by_keys, by_copy):
        assert rep.header() == src.header() and rep.n_keys == len(keys)
        assert sorted(rep.keys().tolist()) == sorted(keys.tolist())
        assert rep.contains(probe).tolist() == src.contains(probe).tolist()
        rep.close()
    src.close()


def test_contexts_on_several_threads_pack_side_by_side(oracle, dcn, genome, index_pair, monkeypatch):
    """Round 4: the host pool runs the jobs of several contexts at a time.  Three contexts, each on its
    own thread, each filtering its own pageable batches cut into dozens of chunks (so their packing jobs interleave on the
    shared workers) -- every call must give the oracle's results, as the same calls do one after another."""
    import threading
    small_chunks(monkeypatch)
    oidx, gidx = index_pair
    rng = np.random.default_rng(77)
    jobs = []
    for t in range(3):
        batches = []
        for _ in range(4):
            reads = mixed_reads(rng, genome, n_short=1500, n_long=4)
            b, o = oracle.concat_reads(reads)
            uid = None if t != 1 else (np.arange(len(reads)) // 2).astype(np.uint32)
            batches.append((b, o, uid))
        jobs.append(batches)
    procs = [dcn.FilterProcessor(gidx, deplete=(t == 2), max_batch_bases=1 << 21, max_batch_reads=1 << 13) for t in range(3)]
    want = [[oracle_batch(oracle, oidx, procs[t], *bt) for bt in jobs[t]] for t in range(3)]
    got, errors = [[None] * 4 for _ in range(3)], []

    def work(t):
        try:
            for rep in range(3):
                for i, (b, o, uid) in enumerate(jobs[t]):
                    got[t][i] = procs[t].filter_batch(b, o, uid)
        except Exception as ex:  # noqa: BLE001
            errors.append((t, repr(ex)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(3)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=300)
        assert not th.is_alive()
    assert not errors, errors
    for t in range(3):
        for i in range(4):
            assert_same(got[t][i], want[t][i])
    for p in procs:
        p.close()


def test_device_pointer_batches_queued_back_to_back(oracle, dcn, genome, index_pair, monkeypatch):
    """Round 4: on the device-pointer API the pack kernel of batch i+1 can run on a side stream, into a second packed buffer,
    while the kernels of batch i run (csrc/ctx.hip, ensure_pack_ahead; DCN_PACK_AHEAD=1 -- off by default, it bought nothing).  Nine batches of three different shapes -- sizes that
    differ by 4 x, reads with N and trailing newlines (the pack kernel's newline flag travels with its buffer), pairs -- are
    queued without a synchronize in between, each with result arrays of its own; every one must give the oracle's
    results.  Then the same in the default order (packed in line), and with per-stage profiling on (which packs in line too)."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    oidx, gidx = index_pair
    rng = np.random.default_rng(91)
    shapes = []
    for n_short, n_long, paired, newline in ((2500, 6, False, False), (600, 1, True, False), (1200, 3, False, True)):
        reads = mixed_reads(rng, genome, n_short=n_short, n_long=n_long)
        if newline:
            reads = [r + b"\n" if i % 3 == 0 and len(r) else r for i, r in enumerate(reads)]
        if paired and len(reads) % 2:
            reads.pop()
        b, o = oracle.concat_reads(reads)
        uid = (np.arange(len(reads)) // 2).astype(np.uint32) if paired else None
        shapes.append((b, o, uid, len(reads) // 2 if paired else len(reads)))
    cap_b, cap_r = max(len(s[0]) for s in shapes) + 64, max(len(s[1]) for s in shapes)
    for mode in ("ahead", "inline", "profiled"):
        if mode == "inline":
            monkeypatch.delenv("DCN_PACK_AHEAD", raising=False)
        else:
            monkeypatch.setenv("DCN_PACK_AHEAD", "1")
        proc = dcn.FilterProcessor(gidx, deplete=True, max_batch_bases=cap_b, max_batch_reads=cap_r)
        want = [oracle_batch(oracle, oidx, proc, b, o, uid) for b, o, uid, _ in shapes]
        if mode == "profiled":
            proc.set_profiling(1)
        dev_in = [(torch.from_numpy(b).to(dev), torch.from_numpy(o.view(np.int64)).to(dev),
                   None if uid is None else torch.from_numpy(uid.view(np.int32)).to(dev)) for b, o, uid, _ in shapes]
        torch.cuda.synchronize()
        outs = []
        for i in range(9):
            b, o, uid, nu = shapes[i % 3]
            d_b, d_o, d_u = dev_in[i % 3]
            k = torch.zeros(nu, dtype=torch.uint8, device=dev)
            h = torch.zeros(nu, dtype=torch.int32, device=dev)
            t = torch.zeros(nu, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()  # (the result arrays are zeroed on torch's stream)
            proc.filter_batch_device(d_b.data_ptr(), d_o.data_ptr(), len(o) - 1, len(b), k.data_ptr(), h.data_ptr(), t.data_ptr(),
                                     d_unit_id=None if d_u is None else d_u.data_ptr(), n_units=nu)
            outs.append((k, h, t))
        proc.synchronize()
        for i, (k, h, t) in enumerate(outs):
            w = want[i % 3]
            assert t.cpu().numpy().tolist() == w[2].tolist(), (mode, i)
            assert h.cpu().numpy().tolist() == w[1].tolist(), (mode, i)
            assert k.cpu().numpy().astype(bool).tolist() == w[0].tolist(), (mode, i)
        assert proc.stats()["total_seqs"] == 3 * sum(len(s[1]) - 1 for s in shapes)
        proc.close()

#!/usr/bin/env python3
"""What dcn_anchor_map_genotype costs over a whole record.  The map is profiles/pileup_qual_rate.py's (the 64 Mbp synthetic
host genome as one record, quality sums kept), filled once by its `short` workload (reads x 150 bp, qualities uniform in
0 .. 41, min_base_qual 20) on the rows of one dcn_place_split_batch call (N = 4).  Then, in this one process, medians of REPS
after one untimed call of each, alternating:
    genotype, count only      gt = gq = NULL, capacity 0: the counting pass, the scan and an 8-byte read-back (the call returns
                              DCN_ERR_CAPACITY with the count unless the range has no site)
    genotype, whole call      AnchorMap.genotype: gt and gq copied back, then the writing pass and the sites' read-back
    pileup_call, whole call   AnchorMap.pileup_call over the same range: the yardstick (one byte per position back, 12 B sites)
each as host time around the blocking call.  The floor of the stream is printed beside them: 32 B read and 2 B written per
position (the packed reference base adds 0.375 B), at the device-to-device copy rate profiles/ records for this box.
  DCN_GENOTYPE_FORM selected the kernel's form in the build this script was written for (wide: four positions per lane, a
16-byte load per plane; simple: one position per lane), read per call, so both were timed in one process.  The build that
ships keeps one form and does not read the variable: the two rows are then the same kernel.
  Kernel times are not taken here: run the script under `rocprofv3 --kernel-trace --stats` in a run of its own (argument
`kernels`: one repetition of each) and read genotype_kernel<...> and pileup_call_kernel<...> from its statistics.
usage: python profiles/genotype_rate.py [short_reads] [kernels]"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402

import bench as B  # noqa: E402

import deacon_server_amd as dcn  # noqa: E402

N_ = dcn._native
KERNELS_ONLY = "kernels" in sys.argv[1:]
REPS = 1 if KERNELS_ONLY else 5
COPY_GBPS = 4790.0  # a device-to-device torch copy on this box (profiles/hbm_stream_probe.py, profiles/README.md)
short_reads = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 10_000_000
dev = torch.device("cuda", 0)
genome = B.make_host_genome(64_000_000, 3, dev)
host = genome.cpu().numpy()
index = dcn.Index.build([host], B.K, B.W, device=0)
amap = dcn.AnchorMap(index, keep_bases=True)
amap.add_records([host])
amap.pileup_enable()
amap.pileup_keep_qualities()
batch = B.make_batches("short", genome, short_reads, 5, dev, rotate=1)[0]
bases = batch.d_bases.cpu().numpy()
offsets = batch.d_offsets.cpu().numpy().astype(np.uint64)
n_reads, n_bases = len(offsets) - 1, int(offsets[-1])
del batch
torch.cuda.empty_cache()
quals = (np.random.default_rng(18).integers(0, 42, n_bases, dtype=np.uint8) + 33).astype(np.uint8)
placer = dcn.Placer(amap, max_batch_bases=n_bases, max_batch_reads=n_reads)
po, rows, _ = placer.place_split_batch(bases, offsets, max_placements=4)
_, n_added = placer.pileup_batch(bases, offsets, rows, row_offsets=po, quals=quals, min_base_qual=20)
placer.close()
del bases, quals, rows, po
n = len(host)
print(f"map: {amap.info()}; {n_reads:,} reads x 150 bp, {n_added:,} rows added; the range: record 0, all {n:,} positions", flush=True)

params = N_.GenotypeParams(2, 3, 20, 20, 477, 301, (C.c_uint32 * 2)(0, 0))
n_sites = C.c_uint64()


def count_only():
    rc = N_.lib().dcn_anchor_map_genotype(amap._h, C.byref(params), 0, 0, n, None, None, None, 0, C.byref(n_sites))
    assert rc in (N_.DCN_OK, N_.DCN_ERR_CAPACITY)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def form(name, fn):
    def run():
        os.environ["DCN_GENOTYPE_FORM"] = name
        return fn()
    return run


calls = {}
for name in ("wide", "simple"):
    calls[f"genotype {name}, count only"] = form(name, count_only)
    calls[f"genotype {name}, whole call"] = form(name, lambda: amap.genotype(0))
calls["pileup_call, whole call"] = lambda: amap.pileup_call(0)
results = {}
for kind, fn in calls.items():  # (untimed)
    results[kind] = fn()
a, b = results["genotype wide, whole call"], results["genotype simple, whole call"]
assert all(np.array_equal(x, y) for x, y in zip(a, b)), "the two forms differ"
gt, gq, sites = a
called = int((gt != dcn.GENOTYPE_NONE).sum())
print(f"defaults: {called:,} positions called, {len(sites):,} sites ({len(sites) * 48 / 1e6:.2f} MB read back), "
      f"pileup_call: {len(results['pileup_call, whole call'][1]):,} sites", flush=True)
times = {kind: [] for kind in calls}
for _ in range(REPS):
    for kind, fn in calls.items():
        times[kind].append(timed(fn))
for kind, t in times.items():
    print(f"  {kind}: {statistics.median(t) * 1e3:.3f} ms median of {REPS} ({min(t) * 1e3:.3f} best, {max(t) * 1e3:.3f} worst)", flush=True)
stream = n * (32 + 2 + 0.375)
line = f"  the stream: {stream / 1e9:.3f} GB per pass (32 B read, 2 B written, 0.375 B of reference per position)"
line += (f"; at the recorded copy rate of {COPY_GBPS:.0f} GB/s its floor is {stream / COPY_GBPS / 1e6:.3f} ms")
print(line, flush=True)
print("not measured: more than one GPU, ploidy 1 at scale, the tool end to end", flush=True)

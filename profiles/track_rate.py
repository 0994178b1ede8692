#!/usr/bin/env python3
"""Depth tracks (dcn_depth_track_batch) beside locate (dcn_locate_batch) on the same host batch, against the same labelled
set, in the same process: both run pack -> plan -> dump scan and differ in what follows (track: the probe sweep that marks
every position and reads its counter + the reduction into bins; locate: the probe sweep that marks hits + the segment
passes).  The set is one member = bench.py's index (the host genome's minimizers + mix64 keys up to 409.9 M) with depth
enabled and warm: the batch is classified once before anything is timed.  locate_rate.py's two workloads:
  short  reads x 150 bp, half drawn from the 64 Mbp host genome
  long   bench.py's long-read shape (lognormal, mean 10 kbp), half of the reads host-derived with 5 % substitutions
All calls are the blocking host forms on pageable memory, so the wall clock of a call includes staging the batch over
PCIe and the copy back; the stage split (dcn_ctx_profile) is device time alone and is the comparison that matters.
Calls alternate, medians of REPS after one untimed call of each.
usage: python profiles/track_rate.py [short_reads] [long_bases]"""
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
import bench as B  # noqa: E402
import deacon_server_amd as dcn  # noqa: E402

REPS = 5
short_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
long_bases = int(sys.argv[2]) if len(sys.argv) > 2 else 1_500_000_000
dev = torch.device("cuda", 0)
genome = B.make_host_genome(64_000_000, 3, dev)
member0, keys0, host_keys, _, build0 = B.build_index(genome, B.PANHUMAN_KEYS, 0)
del keys0, host_keys
print(f"member 0: {member0.n_keys:,} keys ({member0.table_bytes / 1e9:.1f} GB, built in {build0:.1f} s)", flush=True)
iset = dcn.IndexSet([member0])
iset.enable_depth()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def stages_of(obj, fn):
    obj.set_profiling(True)
    fn()
    st, _ = obj.profile()
    obj.set_profiling(False)
    return {k: round(v, 3) for k, v in st.items()}


for name in ("short", "long"):
    if name == "short":
        batch = B.make_batches("short", genome, short_reads, 5, dev, rotate=1)[0]
    else:
        batch = B.make_batches("long", genome, long_bases // B.READ_LEN, 5, dev, rotate=1)[0]
    bases = batch.d_bases.cpu().numpy()
    offsets = batch.d_offsets.cpu().numpy().astype(np.uint64)
    n_reads, n_bases = len(offsets) - 1, int(offsets[-1])
    del batch
    torch.cuda.empty_cache()
    iset.reset_depth()
    clf = dcn.Classifier(iset, max_batch_bases=n_bases, max_batch_reads=n_reads)
    clf.classify_batch(bases, offsets)  # the counters the tracks read
    clf.close()
    stats = iset.depth_stats()
    loc = dcn.Locator(iset, max_batch_bases=n_bases, max_batch_reads=n_reads)
    trk = dcn.DepthTracker(iset, max_batch_bases=n_bases, max_batch_reads=n_reads)  # (one context: bin_bases is per call)
    widths = (1000, 0)
    out = {}

    def locate():
        out["so"], out["segs"] = loc.locate_batch(bases, offsets)

    def track(bb):
        trk.bin_bases = bb
        out[bb] = trk.track_batch(bases, offsets)

    locate()
    locate()  # (the first call sized the segment buffers)
    for bb in widths:
        track(bb)
    tl, tt = [], {bb: [] for bb in widths}
    for _ in range(REPS):
        tl.append(timed(locate))
        for bb in widths:
            tt[bb].append(timed(lambda: track(bb)))
    sl = stages_of(loc, locate)
    st = {bb: stages_of(trk, lambda bb=bb: track(bb)) for bb in widths}
    ml = statistics.median(tl)
    yard = sl["distinct"] + sl["finish"]
    print(f"{name}: {n_reads:,} reads, {n_bases / 1e6:.1f} Mbp, host pageable, {int(stats['observed'][0]):,} keys observed "
          f"(sum {int(stats['sum'][0]):,}, {int(stats['saturated'][0]):,} saturated) | locate {ml * 1e3:.2f} ms median "
          f"({min(tl) * 1e3:.2f} best) | locate stages (ms) {sl} | mark + segments {yard:.3f} ms", flush=True)
    # consistency: the positions that are keys of the set are locate's hits (min_hits = 1, one member)
    hits = int(out["segs"]["n_hits"].astype(np.int64).sum())
    for bb in widths:
        bo, bins = out[bb]
        m = statistics.median(tt[bb])
        own = st[bb]["distinct"] + st[bb]["finish"]
        print(f"{name}: track bin_bases={bb}: {len(bins):,} bins, {m * 1e3:.2f} ms median ({min(tt[bb]) * 1e3:.2f} best) = "
              f"{n_bases / m / 1e6:,.0f} Mbp/s | stages (ms) {st[bb]} | mark + reduce {own:.3f} ms = {own / yard:.2f} x locate's "
              f"mark + segments | n_positions {int(bins['n_positions'].astype(np.int64).sum()):,}, n_keys "
              f"{int(bins['n_keys'].astype(np.int64).sum()):,} (locate's hits {hits:,}: "
              f"{int(bins['n_keys'].astype(np.int64).sum()) == hits}), n_observed {int(bins['n_observed'].astype(np.int64).sum()):,}, "
              f"sum_depth {int(bins['sum_depth'].sum()):,}, max_depth {int(bins['max_depth'].max())}", flush=True)
    loc.close()
    trk.close()
    del bases, offsets, out

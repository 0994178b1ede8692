#!/usr/bin/env python3
"""Placement (dcn_place_batch) beside locate (dcn_locate_batch) on the same host batch in the same process: both run
pack -> plan -> dump scan and differ in what follows (locate: the probe sweep that marks hits + the segment passes;
place: the probe sweep that marks positions and stores each one's anchor + the vote).  The map and locate's index are the
64 Mbp synthetic host genome's own minimizers; the genome is one record.  Two workloads, locate_rate.py's:
  short  reads x 150 bp, half drawn from the host genome
  long   bench.py's long-read shape (lognormal, mean 10 kbp), half of the reads host-derived with 5 % substitutions
Both calls are the blocking host forms on pageable memory, so the wall clock of a call includes staging the batch over
PCIe and the copy back; the stage split (dcn_ctx_profile) is device time alone and is the comparison that matters.
Calls alternate, medians of REPS after one untimed call of each.
usage: python profiles/place_rate.py [short_reads] [long_bases]"""
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
host = genome.cpu().numpy()
index = dcn.Index.build([host], B.K, B.W, device=0)
amap = dcn.AnchorMap(index)
amap.add_records([host[:1_000_000]])  # (untimed: makes the map's context; a map of its own below is the one timed)
amap.close()
amap = dcn.AnchorMap(index)
amap._context(len(host), 1).set_profiling(True)
t0 = time.perf_counter()
amap.add_records([host])
add_s = time.perf_counter() - t0
ms, _ = amap._ctx.profile()
info = amap.info()
print(f"map: {info} over {index.n_keys:,} keys ({index.table_bytes / 1e9:.2f} GB of table, {index.table_bytes / 1e9:.2f} GB of words) | "
      f"dcn_anchor_map_add of the 64 Mbp record: {add_s * 1e3:.1f} ms wall, stages (ms) "
      f"{ {k: round(v, 3) for k, v in ms.items()} } (distinct = the anchor sweep)", flush=True)


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
    loc = dcn.Locator(index, max_batch_bases=n_bases, max_batch_reads=n_reads)
    plc = dcn.Placer(amap, max_batch_bases=n_bases, max_batch_reads=n_reads)
    out = {}

    def locate():
        out["so"], out["segs"] = loc.locate_batch(bases, offsets)

    def place():
        out["pl"] = plc.place_batch(bases, offsets)

    locate()
    locate()  # (the first call sized the segment buffers)
    place()
    tl, tp = [], []
    for _ in range(REPS):
        tl.append(timed(locate))
        tp.append(timed(place))
    sl, sp = stages_of(loc, locate), stages_of(plc, place)
    pl = out["pl"]
    placed = pl["record"] != 0xFFFFFFFF
    located = np.diff(out["so"].astype(np.int64)) > 0
    ml, mp = statistics.median(tl), statistics.median(tp)
    print(f"{name}: {n_reads:,} reads, {n_bases / 1e6:.1f} Mbp, host pageable | locate {ml * 1e3:.2f} ms median "
          f"({min(tl) * 1e3:.2f} best) = {n_bases / ml / 1e6:,.0f} Mbp/s | place {mp * 1e3:.2f} ms median "
          f"({min(tp) * 1e3:.2f} best) = {n_bases / mp / 1e6:,.0f} Mbp/s | locate stages (ms) {sl} | place stages (ms) {sp} | "
          f"place mark {sp['distinct']:.3f} + vote {sp['finish']:.3f} = {sp['distinct'] + sp['finish']:.3f} ms against locate's "
          f"mark + segments {sl['distinct'] + sl['finish']:.3f} ms ({(sp['distinct'] + sp['finish']) / (sl['distinct'] + sl['finish']):.2f} x) | "
          f"placed {int(placed.sum()):,} reads ({placed.mean():.1%}; {int(pl['reverse'][placed].sum()):,} reverse), reads with a segment "
          f"{int(located.sum()):,}, anchor hits {int(pl['n_anchors'].sum()):,} of {int(pl['n_positions'].sum()):,} positions, "
          f"votes {int(pl['votes'].sum()):,}", flush=True)
    loc.close()
    plc.close()
    del bases, offsets, out

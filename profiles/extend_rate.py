#!/usr/bin/env python3
"""Extended placements (dcn_extend_batch) beside aligned placements (dcn_align_batch) on the rows of one
dcn_place_split_batch call, on one context in one process.  The map, the genome and the two workloads are
profiles/align_rate.py's: the 64 Mbp synthetic host genome as one record kept on the device;
  short  reads x 150 bp, half drawn from the host genome
  long   bench.py's long-read shape (lognormal, mean 10 kbp), half of the reads host-derived with 5 % substitutions
extend_batch and align_batch alternate, medians of REPS after one untimed call of each; align_batch is given the capacity
its first call reported.  Both are the blocking host forms on pageable memory.  Stage times are dcn_ctx_profile's (device
time between the events: for extend, FINISH is the extend kernel alone).  Reported for extend_batch: the call's time and the
kernel's; the share of the placed reads' bases inside the read extents before and after; the rows that gained bases.
The yardsticks are records of the parent, not this run: the verify kernel's FINISH on the same rows in
profiles/verify_rate.txt, and align_batch's times in profiles/align_rate.txt.
usage: python profiles/extend_rate.py [short_reads] [long_bases]"""
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
import bench as B  # noqa: E402
import deacon_server_amd as dcn  # noqa: E402

REPS = 5
N = 4
short_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
long_bases = int(sys.argv[2]) if len(sys.argv) > 2 else 1_500_000_000
dev = torch.device("cuda", 0)
genome = B.make_host_genome(64_000_000, 3, dev)
host = genome.cpu().numpy()
index = dcn.Index.build([host], B.K, B.W, device=0)
amap = dcn.AnchorMap(index, keep_bases=True)
amap.add_records([host])
print(f"map: {amap.info()} | store: {len(host) * 0.375 / 1e6:.1f} MB | penalty 6, end_bonus 4, max_edits 1023 (conventions)", flush=True)


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
    plc = dcn.Placer(amap, max_batch_bases=n_bases, max_batch_reads=n_reads)
    po, rows, _ = plc.place_split_batch(bases, offsets, max_placements=N)
    out = {}

    def extend():
        out["extend"] = plc.extend_batch(bases, offsets, rows, row_offsets=po)

    extend()
    _, co, _ = plc.align_batch(bases, offsets, rows, row_offsets=po)  # (untimed: an estimate, then the size reported)
    total = int(co[-1])

    def align():
        out["align"] = plc.align_batch(bases, offsets, rows, row_offsets=po, capacity=total)

    align()
    tx, ta = [], []
    for _ in range(REPS):
        tx.append(timed(extend))
        ta.append(timed(align))
    s_extend, s_align = stages_of(plc, extend), stages_of(plc, align)
    xrows, ext = out["extend"]
    before = (rows["read_end"] - rows["read_start"]).astype(np.int64)
    after = (xrows["read_end"] - xrows["read_start"]).astype(np.int64)
    lens = np.diff(offsets.astype(np.int64))
    first = po[:-1][np.diff(po.astype(np.int64)) > 0].astype(np.int64)  # the first row of every placed read
    placed_bases = int(lens[np.diff(po.astype(np.int64)) > 0].sum())
    mx, ma = statistics.median(tx), statistics.median(ta)
    print(f"{name}: {n_reads:,} reads, {n_bases / 1e6:.1f} Mbp, host pageable, {len(rows):,} rows (N={N})\n"
          f"  extend: {mx * 1e3:.2f} ms median ({min(tx) * 1e3:.2f} best) | stages (ms) {s_extend} | the kernel: FINISH {s_extend['finish']:.3f}\n"
          f"  align:  {ma * 1e3:.2f} ms median ({min(ta) * 1e3:.2f} best) | stages (ms) {s_align}\n"
          f"  rank-0 extents hold {before[first].sum() / placed_bases:.4f} of the placed reads' bases before and "
          f"{after[first].sum() / placed_bases:.4f} after | mean extent of all rows {before.mean():.1f} -> {after.mean():.1f} | "
          f"{int((after > before).sum()):,} of {len(rows):,} rows gained bases, {int((after[first] == lens[np.diff(po.astype(np.int64)) > 0]).sum()):,} "
          f"rank-0 rows are full length | flank edits {int(ext['left_edits'].sum() + ext['right_edits'].sum()):,}",
          flush=True)
    plc.close()
    del bases, offsets, out, rows, po

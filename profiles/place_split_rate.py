#!/usr/bin/env python3
"""Split placements (dcn_place_split_batch) beside placement (dcn_place_batch) on the same host batch, the same map and
ONE context in the same process: both run pack -> plan -> dump scan -> the mark sweep and differ in the vote (place: the
best cell per read; split: up to max_placements rounds per read over a copy of the anchor bitmap, then the exclusive scan
of the per-read counts and the rows with rival and quality) and in what is copied back (place: 48 B per read; split:
8 B of offset and 8 B of counts per read + 64 B per placement).  Map and workloads are profiles/place_rate.py's:
  short  reads x 150 bp, half drawn from the host genome
  long   bench.py's long-read shape (lognormal, mean 10 kbp), half of the reads host-derived with 5 % substitutions
Blocking host forms on pageable memory; the stage split (dcn_ctx_profile) is device time alone.  Calls alternate (place,
split N = 1, 2, 4), medians of REPS after one untimed call of each.
usage: python profiles/place_split_rate.py [short_reads] [long_bases]"""
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
import bench as B  # noqa: E402
import deacon_server_amd as dcn  # noqa: E402

REPS = 5
NS = (1, 2, 4)
short_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
long_bases = int(sys.argv[2]) if len(sys.argv) > 2 else 1_500_000_000
dev = torch.device("cuda", 0)
genome = B.make_host_genome(64_000_000, 3, dev)
host = genome.cpu().numpy()
index = dcn.Index.build([host], B.K, B.W, device=0)
amap = dcn.AnchorMap(index)
amap.add_records([host])
print(f"map: {amap.info()} over {index.n_keys:,} keys", flush=True)


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
    out = {}

    def place():
        out["pl"] = plc.place_batch(bases, offsets)

    def split(n):
        def run():
            out[n] = plc.place_split_batch(bases, offsets, max_placements=n)
        return run

    calls = [("place", place)] + [(f"split N={n}", split(n)) for n in NS]
    for _, fn in calls:
        fn()
    times = {what: [] for what, _ in calls}
    for _ in range(REPS):
        for what, fn in calls:
            times[what].append(timed(fn))
    stages = {what: stages_of(plc, fn) for what, fn in calls}
    pl = out["pl"]
    placed = pl["record"] != 0xFFFFFFFF
    print(f"{name}: {n_reads:,} reads, {n_bases / 1e6:.1f} Mbp, host pageable; place: {int(placed.sum()):,} reads placed, "
          f"{48 * n_reads / 1e6:.1f} MB copied back", flush=True)
    for what, _ in calls:
        med, st = statistics.median(times[what]), stages[what]
        line = (f"  {what}: {med * 1e3:.2f} ms median ({min(times[what]) * 1e3:.2f} best) = {n_bases / med / 1e6:,.0f} Mbp/s | "
                f"stages (ms) {st} | mark {st['distinct']:.3f} + vote {st['finish']:.3f}")
        if what != "place":
            po, rows, counts = out[int(what.split("=")[1])]
            per = np.diff(po.astype(np.int64))
            back = po.nbytes + counts.nbytes + rows.nbytes
            line += (f" ({st['finish'] / stages['place']['finish']:.2f} x place's vote) | {len(rows):,} placements, "
                     f"{int((per > 0).sum()):,} reads placed, {int((per > 1).sum()):,} with two or more, mapq 60: "
                     f"{int((rows['mapq'] == 60).sum()):,}, mapq 0: {int((rows['mapq'] == 0).sum()):,} | {back / 1e6:.1f} MB copied back "
                     f"({back / n_reads:.1f} B per read against 48)")
            first = rows[po[:-1][per > 0].astype(np.int64)]
            assert np.array_equal(per > 0, placed) and (first["votes"] == pl["votes"][placed]).all()
        print(line, flush=True)
    plc.close()
    del bases, offsets, out

#!/usr/bin/env python3
"""The pileup (dcn_pileup_batch) beside aligned placements (dcn_align_batch) on the rows of one dcn_place_split_batch
call (N = 4), on one context in one process.  The map, the genome and the two workloads are profiles/align_rate.py's:
the 64 Mbp synthetic host genome as one record kept on the device;
  short  reads x 150 bp, half drawn from the host genome
  long   bench.py's long-read shape (lognormal, mean 10 kbp), half of the reads host-derived with 5 % substitutions
align_batch and pileup_batch alternate, medians of REPS after one untimed call of each; align_batch is given the capacity
its first call reported, so that every timed call is one dcn_align_batch.  Both are the blocking host forms on pageable
memory.  Stage times are dcn_ctx_profile's: for both calls FINISH spans everything behind the pack (for the pileup: the
verify kernel, the read-back of the edits, the host's walk to the work list, the align kernel of every group, the scan, the
read-back of the total, the gather and the pileup kernel), so it holds host time between the kernels as well; what the
pileup kernel adds is the difference of the two FINISH times less the read-back of the runs that align_batch alone makes
behind its FINISH mark.  The adds are counted from the counters themselves: the sum of all eight columns after one call.
align_batch's numbers are to be read beside profiles/align_rate.txt's: its kernels are the same code.
DCN_LIB_PATH names another build of the library (the position-major layout: -DDCN_PILEUP_POSITION_MAJOR).
usage: python profiles/pileup_rate.py [short_reads] [long_bases]"""
import os
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
amap.pileup_enable()
print(f"library: {os.environ.get('DCN_LIB_PATH', 'the default build (column-major)')}\n"
      f"map: {amap.info()} | store: {len(host) * 0.375 / 1e6:.1f} MB | pileup: {len(host) * 32 / 1e6:.1f} MB", flush=True)


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
    _, co, _ = plc.align_batch(bases, offsets, rows, row_offsets=po)  # (untimed: an estimate, then the size reported)
    total = int(co[-1])

    def align():
        out["align"] = plc.align_batch(bases, offsets, rows, row_offsets=po, capacity=total)

    def pileup():
        out["pileup"] = plc.pileup_batch(bases, offsets, rows, row_offsets=po)

    amap.pileup_reset()
    pileup()
    columns = amap.pileup_fetch(0).sum(axis=0, dtype=np.int64)  # one call's adds, column by column
    adds = int(columns.sum())
    align()
    ta, tp = [], []
    for _ in range(REPS):
        ta.append(timed(align))
        tp.append(timed(pileup))
    s_align, s_pileup = stages_of(plc, align), stages_of(plc, pileup)
    (a_edits, _, cigar), (p_edits, n_added) = out["align"], out["pileup"]
    assert np.array_equal(a_edits, p_edits) and n_added == int((p_edits < dcn.VERIFY_OVER).sum())
    ln, op = cigar >> 4, cigar & 15
    want = int(ln[op != 1].sum()) + int((op == 1).sum())  # one add per step on T, one per inserted run
    assert int(columns[:7].sum()) == want, (columns, want)
    ma, mp = statistics.median(ta), statistics.median(tp)
    over = s_pileup["finish"] - s_align["finish"]
    print(f"{name}: {n_reads:,} reads, {n_bases / 1e6:.1f} Mbp, host pageable, {len(rows):,} rows (N={N}), {n_added:,} added, {len(cigar):,} runs\n"
          f"  align:  {ma * 1e3:.2f} ms median ({min(ta) * 1e3:.2f} best, {max(ta) * 1e3:.2f} worst) | stages (ms) {s_align}\n"
          f"  pileup: {mp * 1e3:.2f} ms median ({min(tp) * 1e3:.2f} best, {max(tp) * 1e3:.2f} worst), {(mp - ma) * 1e3:+.2f} ms against align | stages (ms) {s_pileup}\n"
          f"  FINISH {s_pileup['finish']:.3f} against align's {s_align['finish']:.3f}: {over:+.3f} ms for {adds:,} adds "
          f"({columns.tolist()} by column)" + (f", {adds / over / 1e6:,.1f} G adds/s if all of it is the pileup kernel" if over > 0 else ""),
          flush=True)
    plc.close()
    del bases, offsets, out, rows, po

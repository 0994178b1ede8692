#!/usr/bin/env python3
"""Aligned placements (dcn_align_batch) beside verified placements (dcn_verify_batch) on the rows of one
dcn_place_split_batch call, on one context in one process.  The map, the genome and the two workloads are
profiles/verify_rate.py's: the 64 Mbp synthetic host genome as one record kept on the device;
  short  reads x 150 bp, half drawn from the host genome
  long   bench.py's long-read shape (lognormal, mean 10 kbp), half of the reads host-derived with 5 % substitutions
verify_batch and align_batch alternate, medians of REPS after one untimed call of each; align_batch is given the capacity
its first call reported, so that every timed call is one dcn_align_batch.  Both are the blocking host forms on pageable
memory.  Stage times are dcn_ctx_profile's (device time between the events; for align, FINISH spans the verify kernel, the
read-back of the edits, the host's walk to the work list, the align kernel of every group, the scan, the read-back of the
offsets and the gather, so it holds host time between the kernels as well).  The groups of the default budget are
recomputed here from the edits by the rule of the header (a group closes when the next row's trace would pass the budget).
Then verify_batch alone, REPS more calls, for its stage times beside profiles/verify_rate.txt's.
usage: python profiles/align_rate.py [short_reads] [long_bases]"""
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
BUDGET = int(os.environ.get("DCN_ALIGN_TRACE_BYTES", 1 << 30))
dev = torch.device("cuda", 0)
genome = B.make_host_genome(64_000_000, 3, dev)
host = genome.cpu().numpy()
index = dcn.Index.build([host], B.K, B.W, device=0)
amap = dcn.AnchorMap(index, keep_bases=True)
amap.add_records([host])
print(f"map: {amap.info()} | store: {len(host) * 0.375 / 1e6:.1f} MB | trace budget {BUDGET:,} bytes", flush=True)


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


def groups_of(d):
    """the groups of the rule, from the distances of the aligned rows in row order"""
    words, budget = (d.astype(np.int64) + 1) ** 2, BUDGET // 4
    n, acc = 0, 0
    for x in words.tolist():
        if n == 0 or acc + x > budget:
            n, acc = n + 1, 0
        acc += x
    return n


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

    def verify():
        out["edits"] = plc.verify_batch(bases, offsets, rows, row_offsets=po)

    verify()
    _, co, _ = plc.align_batch(bases, offsets, rows, row_offsets=po)  # (untimed: an estimate, then the size reported)
    total = int(co[-1])

    def align():
        out["align"] = plc.align_batch(bases, offsets, rows, row_offsets=po, capacity=total)

    align()
    tv, ta = [], []
    for _ in range(REPS):
        tv.append(timed(verify))
        ta.append(timed(align))
    s_verify, s_align = stages_of(plc, verify), stages_of(plc, align)
    tv2 = [timed(verify) for _ in range(REPS)]
    s_verify2 = stages_of(plc, verify)
    edits, (a_edits, co, cigar) = out["edits"], out["align"]
    assert np.array_equal(edits, a_edits)
    ok = edits < dcn.VERIFY_OVER
    d = edits[ok]
    n_ops = np.diff(co.astype(np.int64))
    ln, op = cigar >> 4, cigar & 15
    per_op = {k: int(ln[op == v].sum()) for k, v in (("=", 7), ("X", 8), ("I", 1), ("D", 2))}
    assert per_op["X"] + per_op["I"] + per_op["D"] == int(d.sum())
    trace_bytes = int(4 * ((d.astype(np.int64) + 1) ** 2).sum())
    mv, ma = statistics.median(tv), statistics.median(ta)
    print(f"{name}: {n_reads:,} reads, {n_bases / 1e6:.1f} Mbp, host pageable, {len(rows):,} rows (N={N}), {int(ok.sum()):,} aligned, "
          f"mean edits {d.mean():.2f}, largest {int(d.max())}\n"
          f"  verify: {mv * 1e3:.2f} ms median ({min(tv) * 1e3:.2f} best) | stages (ms) {s_verify}\n"
          f"  align:  {ma * 1e3:.2f} ms median ({min(ta) * 1e3:.2f} best), {(ma - mv) * 1e3:.2f} ms over verify | stages (ms) {s_align} | "
          f"FINISH {s_align['finish']:.3f} against verify's {s_verify['finish']:.3f}\n"
          f"  trace {trace_bytes / 1e6:,.1f} MB in {groups_of(d):,} group(s) of at most {BUDGET / 1e6:,.0f} MB (largest row {4 * (int(d.max()) + 1) ** 2 / 1e6:.2f} MB) | "
          f"run slots {4 * int((2 * d.astype(np.int64) + 1).sum()) / 1e6:,.1f} MB | {len(cigar):,} runs, {n_ops[ok].mean():.2f} per aligned row, "
          f"largest {int(n_ops.max())} | bases {per_op}\n"
          f"  verify alone, {REPS} more calls: {statistics.median(tv2) * 1e3:.2f} ms median ({min(tv2) * 1e3:.2f} best) | stages (ms) {s_verify2}",
          flush=True)
    plc.close()
    del bases, offsets, out, rows, po

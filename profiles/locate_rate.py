#!/usr/bin/env python3
"""Locate (dcn_locate_batch) beside classification against one member (dcn_classify_batch, N = 1) on the same host batch
in the same process: both run pack -> plan -> dump scan and differ in what follows (the probe sweep that marks hits + the
segment passes, against classify's lane and workgroup kernels).  Two workloads, member 0 = bench.py's index (the host
genome's minimizers + mix64 keys up to 409.9 M):
  short  classify_rate.py's: reads x 150 bp, half drawn from the 64 Mbp host genome
  long   bench.py's long-read shape (lognormal, mean 10 kbp), half of the reads host-derived with 5 % substitutions
Both calls are the blocking host forms on pageable memory, so the wall clock of a call includes staging the batch over
PCIe and the copy back; the stage split (dcn_ctx_profile) is device time alone and is the comparison that matters.
Calls alternate, medians of REPS after one untimed call of each.
usage: python profiles/locate_rate.py [short_reads] [long_bases]"""
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
    loc = dcn.Locator(member0, max_batch_bases=n_bases, max_batch_reads=n_reads)
    clf = dcn.Classifier(iset, max_batch_bases=n_bases, max_batch_reads=n_reads)
    out = {}

    def locate():
        out["so"], out["segs"] = loc.locate_batch(bases, offsets)

    def classify():
        out["match"], out["hits"], out["total"] = clf.classify_batch(bases, offsets)

    locate()
    locate()  # (the first call sized the segment buffers)
    classify()
    tl, tc = [], []
    for _ in range(REPS):
        tl.append(timed(locate))
        tc.append(timed(classify))
    sl, sc = stages_of(loc, locate), stages_of(clf, classify)
    so, segs = out["so"], out["segs"]
    per_read = np.diff(so.astype(np.int64))
    # consistency: a read has a segment (min_hits = 1) exactly when it has a distinct hit
    same = bool(((per_read > 0) == (out["hits"][:, 0] > 0)).all())
    ml, mc = statistics.median(tl), statistics.median(tc)
    print(f"{name}: {n_reads:,} reads, {n_bases / 1e6:.1f} Mbp, host pageable | locate {ml * 1e3:.2f} ms median "
          f"({min(tl) * 1e3:.2f} best) = {n_bases / ml / 1e6:,.0f} Mbp/s | classify N=1 {mc * 1e3:.2f} ms median "
          f"({min(tc) * 1e3:.2f} best) = {n_bases / mc / 1e6:,.0f} Mbp/s | locate stages (ms) {sl} | classify stages (ms) {sc} | "
          f"mark + segments {sl['distinct'] + sl['finish']:.3f} ms against classify's two kernels "
          f"{sc['distinct'] + sc['finish']:.3f} ms | {len(segs):,} segments in {int((per_read > 0).sum()):,} reads, "
          f"{int((segs['end'] - segs['start']).sum()) / 1e6:.1f} Mbp covered | reads with a segment == reads with a hit: {same}",
          flush=True)
    loc.close()
    clf.close()
    del bases, offsets, out

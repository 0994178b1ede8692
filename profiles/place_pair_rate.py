#!/usr/bin/env python3
"""Paired placements (dcn_place_pair_batch) beside split placements (dcn_place_split_batch) on the same host batch, the
same map and ONE context in the same process: both run pack -> plan -> dump scan -> the mark sweep -> the copy of the
anchor bitmap -> the rounds, and differ in the consumer of the rounds (split: the exclusive scan of the per-read counts
and the CSR rows; pair: one lane per pair over the two mates' rounds, and the insert histogram) and in what is copied
back (split: 16 B of offset and counts per read + 64 B per placement; pair: 80 B per read + 2 KB).  The split call is
the code as it was before the pair call existed, in the same run: it is the only baseline.
Map: profiles/place_rate.py's (the 64 Mbp host genome, its own minimizers).  Batch: pairs of 2 x 150 bp, half of them
the two ends of a fragment of 200 .. 600 bases of the host (mate 1 on either strand), half random.  Blocking host forms
on pageable memory; the stage split (dcn_ctx_profile) is device time alone.  Calls alternate (split N, pair N at N = 1,
2, 4), medians of REPS after one untimed call of each.
usage: python profiles/place_pair_rate.py [pairs]"""
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
MATE = 150
n_pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 5_000_000
dev = torch.device("cuda", 0)
genome = B.make_host_genome(64_000_000, 3, dev)
host = genome.cpu().numpy()
del genome
torch.cuda.empty_cache()
index = dcn.Index.build([host], B.K, B.W, device=0)
amap = dcn.AnchorMap(index)
amap.add_records([host])
print(f"map: {amap.info()} over {index.n_keys:,} keys", flush=True)

# the batch: pair u is reads 2u and 2u + 1
rng = np.random.default_rng(5)
comp = np.zeros(256, np.uint8)
comp[list(b"ACGT")] = list(b"TGCA")
mates = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n_pairs, 2, MATE), dtype=np.uint8)]
from_host = np.flatnonzero(np.arange(n_pairs) % 2 == 0)
span = np.arange(MATE)
for lo in range(0, len(from_host), 200_000):
    u = from_host[lo:lo + 200_000]
    frag = rng.integers(200, 601, len(u))
    start = rng.integers(0, len(host) - 600, len(u))
    fwd = host[start[:, None] + span]
    rev = comp[host[(start + frag - 1)[:, None] - span]]
    flip = (u // 2) % 2 == 1
    mates[u, 0] = np.where(flip[:, None], rev, fwd)
    mates[u, 1] = np.where(flip[:, None], fwd, rev)
bases = mates.reshape(-1)
n_reads = 2 * n_pairs
offsets = (np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(MATE))
n_bases = int(offsets[-1])
del mates


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


plc = dcn.Placer(amap, max_batch_bases=n_bases, max_batch_reads=n_reads)
out = {}


def split(n):
    def run():
        out["split", n] = plc.place_split_batch(bases, offsets, max_placements=n)
    return run


def pair(n):
    def run():
        out["pair", n] = plc.place_pair_batch(bases, offsets, max_placements=n)
    return run


calls = [(kind, n, fn(n)) for n in NS for kind, fn in (("split", split), ("pair", pair))]
for _, _, fn in calls:
    fn()
times = {(kind, n): [] for kind, n, _ in calls}
for _ in range(REPS):
    for kind, n, fn in calls:
        times[kind, n].append(timed(fn))
stages = {(kind, n): stages_of(plc, fn) for kind, n, fn in calls}
print(f"{n_pairs:,} pairs of 2 x {MATE} bp, {n_bases / 1e6:.1f} Mbp, host pageable; one run", flush=True)
for n in NS:
    po, srows, counts = out["split", n]
    rows, hist = out["pair", n]
    for kind in ("split", "pair"):
        t, st = times[kind, n], stages[kind, n]
        med = statistics.median(t)
        line = (f"  {kind} N={n}: {med * 1e3:.2f} ms median ({min(t) * 1e3:.2f} best) = {n_bases / med / 1e6:,.0f} Mbp/s | "
                f"stages (ms) {st} | mark {st['distinct']:.3f} + finish {st['finish']:.3f}")
        if kind == "split":
            back = po.nbytes + counts.nbytes + srows.nbytes
            line += f" | {len(srows):,} placements | {back / 1e6:.1f} MB copied back ({back / n_reads:.1f} B per read)"
        else:
            back = rows.nbytes + hist.nbytes
            per = np.diff(po.astype(np.int64))
            placed = rows["record"] != 0xFFFFFFFF
            alone = np.zeros(n_reads, np.uint32)
            alone[per > 0] = srows["mapq"][po[:-1][per > 0].astype(np.int64)]
            changed = placed & ((per == 0) | (rows["mapq"] != alone))
            proper = int((rows["flags"][0::2] & 1).sum())
            run, median = 0, None
            for i, c in enumerate(hist.tolist()):
                run += c
                if median is None and proper and run * 2 >= proper:
                    median = i * 8
            assert int(hist.sum()) == proper
            line += (f" ({st['finish'] / stages['split', n]['finish']:.2f} x split's finish) | {proper:,} proper pairs, "
                     f"{int(((rows['flags'] & 2) != 0).sum()):,} rescued mates, {int(placed.sum()):,} mates placed, "
                     f"{int(changed.sum()):,} mates whose mapq the partner changed, median insert bin {median} | "
                     f"{back / 1e6:.1f} MB copied back ({back / n_reads:.1f} B per read)")
        print(line, flush=True)
plc.close()

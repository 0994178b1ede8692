#!/usr/bin/env python3
"""What a deletion ledger costs dcn_pileup_batch_qual, and what dcn_anchor_map_indels_genotype costs beside
dcn_anchor_map_insertions_call and dcn_anchor_map_genotype.  The map, the genome and the batch are
profiles/insertions_rate.py's `short` workload (the 64 Mbp synthetic host genome as one record, reads x 150 bp), with
deletions planted at the rate of its insertions: after one call on the batch as it is, which counts the insertion events,
as many single bases are taken out of the reads, at random places that are not a read's first base.  Rows of one
dcn_place_split_batch call (N = 4) on the planted batch, qualities of 30 throughout, in one process on one context.
  Append: three maps over the same index and record: no ledger, the insertion ledger only, both ledgers.  pileup_batch
with qualities alternates between them; after one untimed call of each, the median of REPS with best and worst, host clocks
around calls that end in a synchronise, and FINISH from dcn_ctx_profile.  The first two maps run the parent's code: they are
the yardstick, and the difference between the third and the second is what the deletion append adds.
  Genotype: after a reset and one call, over the whole record a stretch of 2^20 bases at a time as the tool calls them:
indels_genotype count-only (NULLs) and whole, insertions_call, genotype.
usage: python profiles/indels_rate.py [short_reads]     (writes profiles/indels_rate.txt beside what it prints)"""
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

REPS = 5
N = 4
short_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "indels_rate.txt")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def finish_of(obj, fn):
    obj.set_profiling(True)
    fn()
    st, _ = obj.profile()
    obj.set_profiling(False)
    return st["finish"]


def spread(t, unit=1e3):
    return f"{statistics.median(t) * unit:.2f} ms median of {len(t)} ({min(t) * unit:.2f} best, {max(t) * unit:.2f} worst)"


dev = torch.device("cuda", 0)
genome = B.make_host_genome(64_000_000, 3, dev)
host = genome.cpu().numpy()
index = dcn.Index.build([host], B.K, B.W, device=0)
maps = {}
for kind in ("plain", "insertions", "both"):
    m = dcn.AnchorMap(index, keep_bases=True)
    m.add_records([host])
    m.pileup_enable()
    m.pileup_keep_qualities()
    if kind != "plain":
        m.pileup_keep_insertions()
    if kind == "both":
        m.pileup_keep_deletions()
    maps[kind] = m
say(f"map: {maps['plain'].info()}")

batch = B.make_batches("short", genome, short_reads, 5, dev, rotate=1)[0]
bases = batch.d_bases.cpu().numpy()
offsets = batch.d_offsets.cpu().numpy().astype(np.uint64)
del batch
torch.cuda.empty_cache()
n_reads, n_bases = len(offsets) - 1, int(offsets[-1])

# the insertion events of the batch as it is
placer = dcn.Placer(maps["insertions"], max_batch_bases=n_bases, max_batch_reads=n_reads)
po, rows, _ = placer.place_split_batch(bases, offsets, max_placements=N)
placer.pileup_batch(bases, offsets, rows, row_offsets=po, quals=np.full(n_bases, 33 + 30, np.uint8))
ins_events = maps["insertions"].insertions_info()[0]
maps["insertions"].pileup_reset()
placer.close()
# as many deleted bases, none of them a read's first
rng = np.random.default_rng(21)
gone = np.zeros(n_bases, bool)
gone[rng.integers(0, n_bases, ins_events)] = True
gone[offsets[:-1].astype(np.int64)] = False
kept_before = np.concatenate(([0], np.cumsum(~gone)))
bases = np.ascontiguousarray(bases[~gone])
offsets = kept_before[offsets.astype(np.int64)].astype(np.uint64)
n_bases = int(offsets[-1])
quals = np.full(n_bases, 33 + 30, np.uint8)
say(f"short: {n_reads:,} reads, {n_bases / 1e6:.1f} Mbp, host pageable; {ins_events:,} insertion events before, {int(gone.sum()):,} bases taken out")

placers = {kind: dcn.Placer(m, max_batch_bases=n_bases, max_batch_reads=n_reads) for kind, m in maps.items()}
po, rows, _ = placers["plain"].place_split_batch(bases, offsets, max_placements=N)
calls = {kind: (lambda p=p: p.pileup_batch(bases, offsets, rows, row_offsets=po, quals=quals)) for kind, p in placers.items()}
n_added = {kind: fn()[1] for kind, fn in calls.items()}  # (untimed: buffers grow)
assert len(set(n_added.values())) == 1
ins_info, del_info = maps["both"].insertions_info(), maps["both"].deletions_info()
times = {kind: [] for kind in calls}
for _ in range(REPS):
    for kind, fn in calls.items():  # alternating
        times[kind].append(timed(fn))
finish = {kind: [finish_of(placers[kind], fn) for _ in range(3)] for kind, fn in calls.items()}
say(f"  {len(rows):,} rows (N={N}), {n_added['plain']:,} added; per call {ins_info[0]:,} insertion events of {ins_info[1]:,} bases, "
    f"{del_info[0]:,} deletion events of {del_info[1]:,} bases")
for kind in calls:
    say(f"  pileup_batch with qualities, {kind}: {spread(times[kind])} | FINISH {statistics.median(finish[kind]):.3f} ms median of 3 "
        f"({min(finish[kind]):.3f} - {max(finish[kind]):.3f})")
med = {kind: statistics.median(t) * 1e3 for kind, t in times.items()}
fin = {kind: statistics.median(t) for kind, t in finish.items()}
say(f"  the insertion append adds {med['insertions'] - med['plain']:+.2f} ms of the call ({fin['insertions'] - fin['plain']:+.3f} ms of FINISH) over the plain call, "
    f"the deletion append {med['both'] - med['insertions']:+.2f} ms ({fin['both'] - fin['insertions']:+.3f} ms of FINISH) over that")

# the range calls over the whole record, after one call on fresh state
both = maps["both"]
both.pileup_reset()
calls["both"]()
assert both.deletions_info() == del_info
L = dcn._native.lib()
prm = dcn._native.IndelParams(2, 3, 20, 20, 2, 2000, 301, 0)
stretch, length = 1 << 20, len(host)
found = {}


def whole(what):
    total = 0
    for start in range(0, length, stretch):
        n = min(stretch, length - start)
        if what == "indels_genotype, count only":
            a, b = C.c_uint64(), C.c_uint64()
            rc = L.dcn_anchor_map_indels_genotype(both._h, C.byref(prm), 0, start, n, None, 0, None, 0, C.byref(a), C.byref(b))
            assert rc in (0, dcn._native.DCN_ERR_CAPACITY)
            total += a.value
        elif what == "indels_genotype":
            total += len(both.indels_genotype(0, start, n)[0])
        elif what == "insertions_call":
            total += len(both.insertions_call(0, start, n)[0])
        else:
            total += len(both.genotype(0, start, n)[2])
    found[what] = total


for what in ("indels_genotype, count only", "indels_genotype", "insertions_call", "genotype"):
    whole(what)  # (untimed)
    t = [timed(lambda: whole(what)) for _ in range(REPS)]
    say(f"  {what} over the record, {(length + stretch - 1) // stretch} stretches: {spread(t)}, {found[what]:,} "
        f"{'alleles' if what == 'insertions_call' else 'sites'}")
for p in placers.values():
    p.close()
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")

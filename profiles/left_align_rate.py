#!/usr/bin/env python3
"""What left alignment costs, where it finds next to nothing and where it works.
  short: profiles/indels_rate.py's workload (the 64 Mbp synthetic host genome as one record, reads x 150 bp, single bases
taken out of the reads at the rate of their insertions), rows of one dcn_place_split_batch call (N = 4), qualities of 30
throughout.  Two maps over the same index and record, both with both ledgers and quality sums: the switch off and on.
dcn_pileup_batch_qual alternates between them; after one untimed call of each, the median of REPS with best and worst,
host clocks around calls that end in a synchronise, and FINISH from dcn_ctx_profile.  With a third argument, the path of
another build's library (the parent commit's), the script only times the switch-off call through that library, by the
same protocol, and prints the line to compare: the off path of this build must stay within that run's best-to-worst spread.
(A map without the switch adds no launch, no copy and no allocation: dcn_align_runs skips every added line when its
`left` argument is null.)
  long: bench.py's long-read shape, where rows carry hundreds of gaps: dcn_align_batch against dcn_left_align_batch on the
rows of one dcn_place_split_batch call, alternating, the same protocol; time per row and per gap shifted, and the totals.
usage: python profiles/left_align_rate.py [short_reads] [long_bases] [other_library]
       (writes profiles/left_align_rate.txt beside what it prints; with other_library: left_align_rate_parent.txt)"""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
OTHER = sys.argv[3] if len(sys.argv) > 3 else None
if OTHER:
    os.environ["DCN_LIB_PATH"] = OTHER  # (before the package loads its library)
import torch  # noqa: E402

import bench as B  # noqa: E402

import deacon_server_amd as dcn  # noqa: E402

if OTHER:
    dcn._native.ABI = (1, 21)  # the parent's library: the entry points this run calls are all older
    for name in ("dcn_left_align_batch", "dcn_anchor_map_pileup_left_align", "dcn_anchor_map_pileup_left_align_info"):
        dcn._native._SIGNATURES.pop(name)  # ... and it does not export these

REPS = 5
N = 4
short_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
long_bases = int(sys.argv[2]) if len(sys.argv) > 2 else 1_500_000_000
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "left_align_rate_parent.txt" if OTHER else "left_align_rate.txt")
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
kinds = ("off",) if OTHER else ("off", "on")
maps = {}
for kind in kinds:
    m = dcn.AnchorMap(index, keep_bases=True)
    m.add_records([host])
    m.pileup_enable()
    m.pileup_keep_qualities()
    m.pileup_keep_insertions()
    m.pileup_keep_deletions()
    if kind == "on":
        m.pileup_left_align()
    maps[kind] = m
say("library: " + ("another build's, given on the command line" if OTHER else "this build's"))
say(f"map: {maps['off'].info()}")

# ---- short -----------------------------------------------------------------------------------------------------------
batch = B.make_batches("short", genome, short_reads, 5, dev, rotate=1)[0]
bases = batch.d_bases.cpu().numpy()
offsets = batch.d_offsets.cpu().numpy().astype(np.uint64)
del batch
torch.cuda.empty_cache()
n_reads, n_bases = len(offsets) - 1, int(offsets[-1])
placer = dcn.Placer(maps["off"], max_batch_bases=n_bases, max_batch_reads=n_reads)
po, rows, _ = placer.place_split_batch(bases, offsets, max_placements=N)
placer.pileup_batch(bases, offsets, rows, row_offsets=po, quals=np.full(n_bases, 33 + 30, np.uint8))
ins_events = maps["off"].insertions_info()[0]
maps["off"].pileup_reset()
placer.close()
rng = np.random.default_rng(21)  # as many deleted bases, none of them a read's first (profiles/indels_rate.py)
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
po, rows, _ = placers["off"].place_split_batch(bases, offsets, max_placements=N)
calls = {kind: (lambda p=p: p.pileup_batch(bases, offsets, rows, row_offsets=po, quals=quals)) for kind, p in placers.items()}
n_added = {kind: fn()[1] for kind, fn in calls.items()}  # (untimed: buffers grow)
assert len(set(n_added.values())) == 1
times = {kind: [] for kind in calls}
for _ in range(REPS):
    for kind, fn in calls.items():  # alternating
        times[kind].append(timed(fn))
finish = {kind: [finish_of(placers[kind], fn) for _ in range(3)] for kind, fn in calls.items()}
say(f"  {len(rows):,} rows (N={N}), {n_added['off']:,} added per call")
for kind in calls:
    say(f"  pileup_batch with qualities, both ledgers, left alignment {kind}: {spread(times[kind])} | FINISH {statistics.median(finish[kind]):.3f} ms "
        f"median of 3 ({min(finish[kind]):.3f} - {max(finish[kind]):.3f})")
if not OTHER:
    info = maps["on"].pileup_left_align_info()
    calls_on = 1 + REPS + 3
    say(f"  per call with it on: {info['rows_aligned'] // calls_on:,} rows aligned, {info['rows_changed'] // calls_on:,} changed, "
        f"{info['gaps_shifted'] // calls_on:,} gaps shifted over {info['columns_passed'] // calls_on:,} columns, {info['gaps_merged'] // calls_on:,} merged")
    med = {kind: statistics.median(t) * 1e3 for kind, t in times.items()}
    fin = {kind: statistics.median(t) for kind, t in finish.items()}
    say(f"  the pass adds {med['on'] - med['off']:+.2f} ms of the call ({fin['on'] - fin['off']:+.3f} ms of FINISH); the off call's own spread is "
        f"{(max(times['off']) - min(times['off'])) * 1e3:.2f} ms")
for p in placers.values():
    p.close()

# ---- long ------------------------------------------------------------------------------------------------------------
if not OTHER and long_bases > 0:
    batch = B.make_batches("long", genome, long_bases // B.READ_LEN, 5, dev, rotate=1)[0]
    bases = batch.d_bases.cpu().numpy()
    offsets = batch.d_offsets.cpu().numpy().astype(np.uint64)
    del batch
    torch.cuda.empty_cache()
    n_reads, n_bases = len(offsets) - 1, int(offsets[-1])
    placer = dcn.Placer(maps["off"], max_batch_bases=n_bases, max_batch_reads=n_reads)
    po, rows, _ = placer.place_split_batch(bases, offsets, max_placements=N)
    a, b = placer.align_batch(bases, offsets, rows, row_offsets=po), placer.left_align_batch(bases, offsets, rows, row_offsets=po)  # (untimed)
    plain = lambda: placer.align_batch(bases, offsets, rows, row_offsets=po, capacity=len(a[2]))  # noqa: E731
    left = lambda: placer.left_align_batch(bases, offsets, rows, row_offsets=po, capacity=len(b[2]))  # noqa: E731
    info = b[3]
    assert np.array_equal(a[0], b[0])
    t = {"align_batch": [], "left_align_batch": []}
    for _ in range(REPS):
        t["align_batch"].append(timed(plain))
        t["left_align_batch"].append(timed(left))
    say(f"long: {n_reads:,} reads, {n_bases / 1e6:.1f} Mbp, {len(rows):,} rows; {info['rows_aligned']:,} aligned, {info['rows_changed']:,} changed, "
        f"{info['gaps_shifted']:,} gaps shifted over {info['columns_passed']:,} columns, {info['gaps_merged']:,} merged; runs {len(a[2]):,} -> {len(b[2]):,}")
    for kind in t:
        say(f"  {kind}: {spread(t[kind])}")
    extra = statistics.median(t["left_align_batch"]) - statistics.median(t["align_batch"])
    say(f"  the pass adds {extra * 1e3:+.2f} ms: {extra * 1e9 / max(info['rows_aligned'], 1):.0f} ns per aligned row, "
        f"{extra * 1e9 / max(info['gaps_shifted'], 1):.0f} ns per gap shifted (align_batch's own spread: "
        f"{(max(t['align_batch']) - min(t['align_batch'])) * 1e3:.2f} ms)")
    placer.close()
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")

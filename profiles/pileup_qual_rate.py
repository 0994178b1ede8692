#!/usr/bin/env python3
"""What base qualities cost dcn_pileup_batch: dcn_pileup_batch_qual beside it.  The map, the genome and the two workloads are
profiles/pileup_rate.py's (the 64 Mbp synthetic host genome as one record; `short`: reads x 150 bp, `long`: bench.py's
long-read shape), on the rows of one dcn_place_split_batch call (N = 4), in one process on one context; the qualities are
uniform in 0 .. 41 at offset 33, one byte per base of the batch, in pageable host memory like the bases.
  Two maps over the same index and record, one keeping quality sums and one not.  Five calls alternate, medians of REPS after
one untimed call of each, FINISH from dcn_ctx_profile (it spans everything behind the pack, host time between the kernels
and the copy of the qualities included):
    plain                 pileup_batch without qualities on the map without sums: the call as it was
    q0, q20               pileup_batch with quals at min_base_qual 0 and 20 on the map without sums: the 1 B per base copy and
                          the byte load per counted base
    q0+sums, q20+sums     the same on the map with sums: a second atomic per base counted in A C G T
  With a third argument, the path of the parent commit's library, the script first runs itself in a child process with
DCN_LIB_PATH set to it: the same rows through the parent's dcn_pileup_batch, so that the yardstick of `plain` is the parent
and not this code.  (That library has no quality calls: the child binds the surface it has.)
usage: python profiles/pileup_qual_rate.py [short_reads] [long_bases] [parent_library]"""
import os
import statistics
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, ".")
PARENT = bool(os.environ.get("DCN_PILEUP_QUAL_RATE_PARENT"))
if len(sys.argv) > 3 and not PARENT:
    env = dict(os.environ, DCN_LIB_PATH=os.path.abspath(sys.argv[3]), DCN_PILEUP_QUAL_RATE_PARENT="1")
    print("---- the parent commit's library on the same rows (a child process) ----", flush=True)
    subprocess.run([sys.executable, sys.argv[0]] + sys.argv[1:3], env=env, check=True)
    print("---- this build ----", flush=True)

import torch  # noqa: E402

import bench as B  # noqa: E402

import deacon_server_amd as dcn  # noqa: E402

if PARENT:  # the parent's library lacks the three entry points: bind what it has, before the library is first loaded
    for name in ("dcn_anchor_map_pileup_keep_qualities", "dcn_pileup_batch_qual", "dcn_anchor_map_pileup_fetch_qualities"):
        del dcn._native._SIGNATURES[name]
    dcn._native.ABI = (1, 17)

REPS = 5
N = 4
short_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
long_bases = int(sys.argv[2]) if len(sys.argv) > 2 else 1_500_000_000
dev = torch.device("cuda", 0)
genome = B.make_host_genome(64_000_000, 3, dev)
host = genome.cpu().numpy()
index = dcn.Index.build([host], B.K, B.W, device=0)
maps = {}
for kind in ("plain",) if PARENT else ("plain", "sums"):
    m = dcn.AnchorMap(index, keep_bases=True)
    m.add_records([host])
    m.pileup_enable()
    if kind == "sums":
        m.pileup_keep_qualities()
    maps[kind] = m
print(f"library: {os.path.relpath(os.environ['DCN_LIB_PATH']) if os.environ.get('DCN_LIB_PATH') else 'the default build'}\nmap: {maps['plain'].info()}", flush=True)


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
    quals = (np.random.default_rng(18).integers(0, 42, n_bases, dtype=np.uint8) + 33).astype(np.uint8)
    placers = {kind: dcn.Placer(m, max_batch_bases=n_bases, max_batch_reads=n_reads) for kind, m in maps.items()}
    po, rows, _ = placers["plain"].place_split_batch(bases, offsets, max_placements=N)
    calls = {"plain": lambda: placers["plain"].pileup_batch(bases, offsets, rows, row_offsets=po)}
    if not PARENT:
        for kind, tag in (("plain", ""), ("sums", "+sums")):
            for threshold in (0, 20):
                calls[f"q{threshold}{tag}"] = (lambda p=placers[kind], t=threshold:
                                               p.pileup_batch(bases, offsets, rows, row_offsets=po, quals=quals, min_base_qual=t))
    for m in maps.values():
        m.pileup_reset()
    n_added = {kind: fn()[1] for kind, fn in calls.items()}  # (untimed: buffers grow)
    assert len(set(n_added.values())) == 1
    times = {kind: [] for kind in calls}
    for _ in range(REPS):
        for kind, fn in calls.items():
            times[kind].append(timed(fn))
    finish = {kind: [finish_of(placers["sums" if kind.endswith("+sums") else "plain"], fn) for _ in range(3)] for kind, fn in calls.items()}
    print(f"{name}: {n_reads:,} reads, {n_bases / 1e6:.1f} Mbp, host pageable, {len(rows):,} rows (N={N}), {n_added['plain']:,} added", flush=True)
    med = {kind: (statistics.median(times[kind]) * 1e3, statistics.median(finish[kind])) for kind in calls}
    for kind in calls:
        t = times[kind]
        line = (f"  pileup_batch, {kind}: {med[kind][0]:.2f} ms median of {REPS} ({min(t) * 1e3:.2f} best, {max(t) * 1e3:.2f} worst) | "
                f"FINISH {med[kind][1]:.3f} ms median of 3 ({min(finish[kind]):.3f} - {max(finish[kind]):.3f})")
        if kind != "plain":
            line += f" | against plain: {med[kind][0] - med['plain'][0]:+.2f} ms of the call, {med[kind][1] - med['plain'][1]:+.3f} ms of FINISH"
        print(line, flush=True)
    if not PARENT:
        for t in (0, 20):
            print(f"  the sums add {med[f'q{t}+sums'][1] - med[f'q{t}'][1]:+.3f} ms of FINISH, {med[f'q{t}+sums'][0] - med[f'q{t}'][0]:+.2f} ms of the call "
                  f"at min_base_qual {t}", flush=True)
        # one call on fresh state: how many bases were counted in A C G T, and what they sum to
        maps["sums"].pileup_reset()
        calls["q20+sums"]()
        c = maps["sums"].pileup_fetch(0).sum(axis=0, dtype=np.int64)
        s = maps["sums"].pileup_fetch_qualities(0).sum(axis=0, dtype=np.int64)
        print(f"  one call at 20 with sums: {int(c[:4].sum()):,} bases counted in A C G T (a second add each), {int(c[4]):,} in N, "
              f"quality sum {int(s.sum()):,}; {n_bases / 1e6:.1f} MB of qualities copied per call", flush=True)
    for p in placers.values():
        p.close()
    del bases, offsets, rows, po, quals

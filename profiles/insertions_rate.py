#!/usr/bin/env python3
"""What an insertion ledger costs dcn_pileup_batch, and what dcn_anchor_map_insertions_call costs beside
dcn_anchor_map_pileup_call.  The map, the genome and the two workloads are profiles/pileup_rate.py's (the 64 Mbp synthetic
host genome as one record; `short`: reads x 150 bp, `long`: bench.py's long-read shape), on the rows of one
dcn_place_split_batch call (N = 4), in one process on one context.
  Two maps over the same index and record, one keeping a ledger and one not; pileup_batch alternates between them, medians
of REPS after one untimed call of each, FINISH from dcn_ctx_profile (it spans everything behind the pack, host time between
the kernels included).  The difference of the two FINISH times is what the ledger adds: the counting pass and the 16-byte
read-back always, the two scans and the writing pass when the batch has an I run.  Then, after a reset and one call,
insertions_call and pileup_call over the whole record, a stretch of 2^20 bases at a time as the tool calls them.
  With a third argument, the path of the parent commit's library, the script first runs itself in a child process with
DCN_LIB_PATH set to it: the same rows through the parent's dcn_pileup_batch, so that the yardstick of the map without a
ledger is the parent and not this code.  (That library has no ledger: the child binds the surface it has.)
usage: python profiles/insertions_rate.py [short_reads] [long_bases] [parent_library]"""
import os
import statistics
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, ".")
PARENT = bool(os.environ.get("DCN_INSERTIONS_RATE_PARENT"))
if len(sys.argv) > 3 and not PARENT:
    env = dict(os.environ, DCN_LIB_PATH=os.path.abspath(sys.argv[3]), DCN_INSERTIONS_RATE_PARENT="1")
    print("---- the parent commit's library on the same rows (a child process) ----", flush=True)
    subprocess.run([sys.executable, sys.argv[0]] + sys.argv[1:3], env=env, check=True)
    print("---- this build ----", flush=True)

import torch  # noqa: E402

import bench as B  # noqa: E402

import deacon_server_amd as dcn  # noqa: E402

if PARENT:  # the parent's library lacks the four entry points: bind what it has, before the library is first loaded
    for name in [n for n in dcn._native._SIGNATURES if "insertions" in n]:
        del dcn._native._SIGNATURES[name]
    dcn._native.ABI = (1, 16)

REPS = 5
N = 4
short_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
long_bases = int(sys.argv[2]) if len(sys.argv) > 2 else 1_500_000_000
dev = torch.device("cuda", 0)
genome = B.make_host_genome(64_000_000, 3, dev)
host = genome.cpu().numpy()
index = dcn.Index.build([host], B.K, B.W, device=0)
maps = {}
for kind in ("plain",) if PARENT else ("plain", "ledger"):
    m = dcn.AnchorMap(index, keep_bases=True)
    m.add_records([host])
    m.pileup_enable()
    if kind == "ledger":
        m.pileup_keep_insertions()
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
    placers = {kind: dcn.Placer(m, max_batch_bases=n_bases, max_batch_reads=n_reads) for kind, m in maps.items()}
    po, rows, _ = placers["plain"].place_split_batch(bases, offsets, max_placements=N)
    calls = {kind: (lambda p=p: p.pileup_batch(bases, offsets, rows, row_offsets=po)) for kind, p in placers.items()}
    for m in maps.values():
        m.pileup_reset()
    n_added = {kind: fn()[1] for kind, fn in calls.items()}  # (untimed: buffers grow)
    appended = maps["ledger"].insertions_info() if "ledger" in maps else None
    times = {kind: [] for kind in calls}
    for _ in range(REPS):
        for kind, fn in calls.items():
            times[kind].append(timed(fn))
    finish = {kind: [finish_of(placers[kind], fn) for _ in range(3)] for kind, fn in calls.items()}
    print(f"{name}: {n_reads:,} reads, {n_bases / 1e6:.1f} Mbp, host pageable, {len(rows):,} rows (N={N}), {n_added['plain']:,} added", flush=True)
    for kind in calls:
        t = times[kind]
        print(f"  pileup_batch, {kind}: {statistics.median(t) * 1e3:.2f} ms median of {REPS} ({min(t) * 1e3:.2f} best, {max(t) * 1e3:.2f} worst) | "
              f"FINISH {statistics.median(finish[kind]):.3f} ms median of 3 ({min(finish[kind]):.3f} - {max(finish[kind]):.3f})", flush=True)
    if "ledger" in maps:
        assert n_added["ledger"] == n_added["plain"]
        print(f"  the ledger adds {statistics.median(finish['ledger']) - statistics.median(finish['plain']):+.3f} ms of FINISH, "
              f"{(statistics.median(times['ledger']) - statistics.median(times['plain'])) * 1e3:+.2f} ms of the call, for {appended[0]:,} events and "
              f"{appended[1]:,} bases appended per call", flush=True)
        # calls over the whole record, after one call on fresh state
        led = maps["ledger"]
        led.pileup_reset()
        calls["ledger"]()
        assert led.insertions_info() == appended
        stretch, length = 1 << 20, len(host)
        found = {}

        def whole(what):
            total = 0
            for start in range(0, length, stretch):
                n = min(stretch, length - start)
                total += len(led.insertions_call(0, start, n)[0]) if what == "insertions_call" else len(led.pileup_call(0, start, n)[1])
            found[what] = total

        for what in ("pileup_call", "insertions_call"):
            whole(what)  # (untimed)
            t = [timed(lambda: whole(what)) for _ in range(REPS)]
            print(f"  {what} over the record, {(length + stretch - 1) // stretch} stretches: {statistics.median(t) * 1e3:.2f} ms median of {REPS} "
                  f"({min(t) * 1e3:.2f} best, {max(t) * 1e3:.2f} worst), {found[what]:,} {'alleles' if what == 'insertions_call' else 'sites'}", flush=True)
    for p in placers.values():
        p.close()
    del bases, offsets, rows, po

#!/usr/bin/env python3
"""What dcn_phase_batch takes beside dcn_pileup_batch_qual over the same rows of the same map, and what
dcn_anchor_map_phase_solve takes at 1 M and at 16 M sites.
  The record is profiles/blocks_rate.py's (the 64 Mbp synthetic host genome as one record); the rows are reference-exact reads
written out here (no placement), with a substitution every 997 bases so that a long row has runs: (a) 150-base rows, one every
150 bases of the first 16 Mbp, with a site about every 1,000 bases, so that nearly every row ends behind the search; (b) 10 kbp
rows, one every 2,500 bases of the first 16 Mbp, the same sites.  For the solve, a site every 64 (1 M) and every 4 (16 M)
bases; the links are whatever the last batch left, which does not change what the passes read and write.
  One process; after one untimed call of each, five calls each, host clocks around the blocking calls.  Most of either batch
call is the align passes they share, so the difference of the two medians is what the link kernel costs less than the pileup
kernel, and not either kernel's time.
  Kernel times are not taken here: run the script under `rocprofv3 --kernel-trace --stats` in a run of its own with the
argument `kernels` (two calls each, nothing written) and read phase_link_kernel<true> beside pileup_kernel<true, false>, and
phase_decide_kernel, phase_aggregate_kernel, phase_prefix_kernel and phase_apply_kernel, from its statistics.
usage: python profiles/phase_rate.py [kernels]   (without arguments: writes profiles/phase_rate.txt beside what it prints)"""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402

import bench as B  # noqa: E402

import deacon_server_amd as dcn  # noqa: E402

KERNELS = len(sys.argv) > 1 and sys.argv[1] == "kernels"
REPS = 2 if KERNELS else 5
LENGTH, SPAN = 64_000_000, 16_000_000
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "phase_rate.txt")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def spread(t):
    return f"{statistics.median(t) * 1e3:.2f} ms median of {len(t)} ({min(t) * 1e3:.2f} best, {max(t) * 1e3:.2f} worst)"


dev = torch.device("cuda", 0)
host = B.make_host_genome(LENGTH, 3, dev).cpu().numpy()
index = dcn.Index.build([host], B.K, B.W, device=0)
amap = dcn.AnchorMap(index, keep_bases=True)
amap.add_records([host])
amap.pileup_enable()
amap.pileup_keep_qualities()
say(f"map: {amap.info()}; one record of {LENGTH:,} bases")
COLUMN = np.full(256, 4, np.uint8)
for letter, col in zip(b"ACGT", range(4)):
    COLUMN[letter] = COLUMN[letter + 32] = col


def sites_every(step, span):
    pos = np.arange(step // 2, span, step, dtype=np.uint64)
    ref = COLUMN[host[pos.astype(np.int64)]]
    pos, ref = pos[ref < 4], ref[ref < 4]
    s = np.zeros(len(pos), dcn.PHASE_SITE_DTYPE)
    s["pos"], s["record"], s["a0"], s["a1"] = pos, 0, ref, (ref + 1) % 4
    return s


def rows_of(read_len, step):
    starts = np.arange(0, SPAN - read_len + 1, step, dtype=np.int64)
    at = (starts[:, None] + np.arange(read_len)[None, :]).reshape(-1)
    bases = host[at].copy()
    swap = np.frombuffer(b"CATG", np.uint8)  # another letter at every 997th base of the record: X runs in a long row
    hit = (at % 997 == 0) & (COLUMN[bases] < 4)
    bases[hit] = swap[COLUMN[bases[hit]]]
    offsets = np.arange(len(starts) + 1, dtype=np.uint64) * read_len
    rows = np.zeros(len(starts), dcn.filter.PLACEMENT_DTYPE)
    rows["record"], rows["read_start"], rows["read_end"], rows["ref_start"], rows["ref_end"] = 0, 0, read_len, starts, starts + read_len
    return bases, offsets, rows, np.full(len(bases), 33 + 30, np.uint8)


amap.phase_sites(sites_every(1000, SPAN))
for name, read_len, step in (("(a) 150-base rows", 150, 150), ("(b) 10 kbp rows", 10_000, 2_500)):
    bases, offsets, rows, quals = rows_of(read_len, step)
    placer = dcn.Placer(amap, max_batch_bases=len(bases), max_batch_reads=len(rows))
    pile = lambda: placer.pileup_batch(bases, offsets, rows, quals=quals, min_base_qual=20)  # noqa: E731
    link = lambda: placer.phase_batch(bases, offsets, rows, quals=quals, min_base_qual=20)  # noqa: E731
    _, added = pile()
    _, linking = link()
    t_pile, t_link = [timed(pile) for _ in range(REPS)], [timed(link) for _ in range(REPS)]
    say(f"{name}: {len(rows):,} rows, {len(bases):,} bases, {amap.phase_info()[0]:,} sites, {added:,} rows added, {linking:,} rows linking")
    say(f"  dcn_pileup_batch_qual, whole call: {spread(t_pile)}")
    say(f"  dcn_phase_batch, whole call:       {spread(t_link)}")
    placer.close()
for name, step in (("1 M sites", 64), ("16 M sites", 4)):
    amap.phase_sites(sites_every(step, LENGTH))
    amap.phase_solve()
    t = [timed(amap.phase_solve) for _ in range(REPS)]
    say(f"dcn_anchor_map_phase_solve, {name} ({amap.phase_info()[0]:,}), whole call with the copy of 32 B per site: {spread(t)}")
if not KERNELS:
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")

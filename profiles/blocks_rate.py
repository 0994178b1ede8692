#!/usr/bin/env python3
"""What dcn_anchor_map_reference_blocks takes over a whole 64 Mbp record, beside dcn_anchor_map_genotype over the same range
of the same map: both stream the same planes, so the genotype call is the yardstick.
  The record is profiles/strand_rate.py's (the 64 Mbp synthetic host genome as one record).  Three pile-ups on one map, each
by rows written out here (no placement): none at all, so that the record is one block of one class; 64-base reference-exact
reads 128 bases apart, 1 M blocks (covered and not, in turn); and reads over every base whose qualities are four of 30 and
four of 3 in turn, so that with min_depth 1 and min_gq 0 the class changes every four positions: 16 M blocks.
  One process; after one untimed call of each, five calls each, host clocks around the blocking calls: the genotype call
without its bytes (gt = gq = NULL; the sites it finds are fetched), the blocks call that only counts (blocks NULL, capacity
0: classify, breaks, heads, scan), and the whole blocks call (cls NULL), whose difference to the counting call is the fill,
the reducing pass and the copy of the blocks to the host (and, inside the call, the allocation of the blocks on the
device, which zeroes them once before blocks_fill_kernel writes them).
  Kernel times are not taken here: run the script under `rocprofv3 --kernel-trace --stats` in a run of its own with the
arguments `kernels S` (S = 0, 1 or 2: that scenario alone, two calls each of the genotype call and of the whole blocks
call, nothing written) and read blocks_classify_kernel, blocks_heads_kernel<false> and <true>, blocks_fill_kernel, the
three offsets_scan kernels and genotype_kernel<false> from its statistics; profiles/blocks_rate.txt holds those below the
script's own lines.
usage: python profiles/blocks_rate.py [kernels S]   (without arguments: writes profiles/blocks_rate.txt beside what it prints)"""
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

KERNELS = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[1] == "kernels" else None
REPS = 5
LENGTH = 64_000_000
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "blocks_rate.txt")
N = dcn._native
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


def pile(read_len, step, quals_of):
    """reference-exact forward reads of read_len bases every step bases, the rows written out"""
    starts = np.arange(0, LENGTH - read_len + 1, step, dtype=np.int64)
    bases = host[(starts[:, None] + np.arange(read_len)[None, :]).reshape(-1)]
    offsets = (np.arange(len(starts) + 1, dtype=np.uint64) * read_len)
    rows = np.zeros(len(starts), dcn.filter.PLACEMENT_DTYPE)
    rows["record"], rows["read_start"], rows["read_end"], rows["ref_start"], rows["ref_end"] = 0, 0, read_len, starts, starts + read_len
    placer = dcn.Placer(amap, max_batch_bases=len(bases), max_batch_reads=len(starts))
    amap.pileup_reset()
    _, added = placer.pileup_batch(bases, offsets, rows, quals=quals_of(starts, read_len), min_base_qual=20)
    placer.close()
    assert added == len(starts)
    return len(starts)


def measure(name, params):
    prm = N.BlockParams(2, params["min_depth"], params["min_gq"], 20, 477, 301, 5, 0, (C.c_uint8 * 16)(20, 40, 60, 80, 99))
    gprm = N.GenotypeParams(2, params["min_depth"], params["min_gq"], 20, 477, 301, (C.c_uint32 * 2)(0, 0))
    count, n_sites = C.c_uint64(), C.c_uint64()
    L = N.lib()

    def count_only():
        rc = L.dcn_anchor_map_reference_blocks(amap._h, C.byref(prm), 0, 0, LENGTH, None, 0, None, None, 0, C.byref(count))
        assert rc in (N.DCN_OK, N.DCN_ERR_CAPACITY)

    count_only()
    blocks = np.zeros(max(int(count.value), 1), dcn.REFERENCE_BLOCK_DTYPE)

    def whole():
        N.check(L.dcn_anchor_map_reference_blocks(amap._h, C.byref(prm), 0, 0, LENGTH, None, 0, None, blocks.ctypes.data_as(C.c_void_p), len(blocks),
                                                  C.byref(count)))

    rc = L.dcn_anchor_map_genotype(amap._h, C.byref(gprm), 0, 0, LENGTH, None, None, None, 0, C.byref(n_sites))
    assert rc in (N.DCN_OK, N.DCN_ERR_CAPACITY)
    sites = np.zeros(max(int(n_sites.value), 1), dcn.GENOTYPE_SITE_DTYPE)

    def genotype():
        N.check(L.dcn_anchor_map_genotype(amap._h, C.byref(gprm), 0, 0, LENGTH, None, None, sites.ctypes.data_as(C.c_void_p), len(sites), C.byref(n_sites)))

    for fn in (genotype, count_only, whole):
        fn()
    if KERNELS is not None:  # (the second call of each is the one to read)
        genotype()
        whole()
        say(f"{name}: {int(count.value):,} blocks, {int(n_sites.value):,} genotype sites; two calls each for the kernel trace")
        return
    t = {fn.__name__: [timed(fn) for _ in range(REPS)] for fn in (genotype, count_only, whole)}
    assert int(blocks["len"][:int(count.value)].sum(dtype=np.uint64)) == LENGTH - int(n_sites.value)  # the blocks and the sites tile the record
    g, c, w = (statistics.median(t[k]) for k in ("genotype", "count_only", "whole"))
    say(f"{name}: {int(count.value):,} blocks, {int(n_sites.value):,} genotype sites")
    say(f"  genotype, no bytes:                      {spread(t['genotype'])}")
    say(f"  reference_blocks, counting only:         {spread(t['count_only'])}   {c / g:.2f} x the genotype call")
    say(f"  reference_blocks, whole (cls NULL):      {spread(t['whole'])}   {w / g:.2f} x the genotype call")
    say(f"  fill, reduce and the copy of the blocks: {(w - c) * 1e3:.2f} ms, {(w - c) / c:.2f} x the counting passes; "
        f"{LENGTH / w / 1e9:.2f} G positions/s over all")


if KERNELS in (None, 0):
    measure("no pile-up, one class", dict(min_depth=3, min_gq=20))
if KERNELS in (None, 1):
    n = pile(64, 128, lambda starts, read_len: np.full(len(starts) * read_len, 33 + 30, np.uint8))
    say(f"sparse coverage: {n:,} reads of 64 bases, 128 apart")
    measure("sparse coverage", dict(min_depth=3, min_gq=20))
if KERNELS in (None, 2):
    n = pile(160, 160, lambda starts, read_len: np.tile(np.array([63] * 4 + [36] * 4, np.uint8), len(starts) * read_len // 8))
    say(f"classes alternating: {n:,} reads of 160 bases end to end, qualities 30 30 30 30 3 3 3 3 in turn, min_depth 1, min_gq 0")
    measure("classes alternating", dict(min_depth=1, min_gq=0))
amap.close()
index.close()
if KERNELS is None:
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")

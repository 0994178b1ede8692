#!/usr/bin/env python3
"""The counting index build against the plain one, at the library: host arrays in, device table out.
Two inputs, made from a seed: a synthetic genome of GENOME_BP bases in 8 records, and N_READS reads of 150 bp drawn from
both strands of its first 50 Mbp.  For each, alternating in one process, medians of REPS wall-clock times (every call is
blocking) of
  dcn_index_build                                       (the plain build)
  dcn_index_builder_create + _add + _finish(1, 0)       (the counting build; the builder's front end is made by the add)
and, on the builder of the last repetition, _finish(2, 0) and _hist alone.  Then SPLIT_REPS more runs of each build under
DCN_INDEX_TIMING=1: the library prints where each went (stderr: host seconds for the front end, staging, growth and finish;
pack / plan / scan / sweep from the context's stage events, dcn_ctx_profile).  Those runs wait for each chunk's copies and
record six events per chunk, so their own wall-clock times are not the medians' kind.
Needs no reference data and no downloads.
usage: python profiles/index_builder_rate.py [genome_bp] [n_reads]"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
try:
    import torch  # noqa: F401  (its HIP runtime first, as the tests and bench.py load it)
except Exception:
    pass
import deacon_server_amd as dcn  # noqa: E402
from deacon_server_amd import _native as N  # noqa: E402

REPS = 5
SPLIT_REPS = 3
K, W = 31, 15
GENOME_BP = int(sys.argv[1]) if len(sys.argv) > 1 else 400_000_000
N_READS = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
READ_LEN = 150


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return time.perf_counter() - t0, r


def plain(bases, offsets):
    h = C.c_void_p()
    N.check(N.lib().dcn_index_build(ptr(bases), ptr(offsets), len(offsets) - 1, K, W, 0.0, 0, 0, C.byref(h)))
    return dcn.Index(h, 0)


def counted(bases, offsets):
    b = dcn.IndexBuilder(K, W)
    N.check(N.lib().dcn_index_builder_add(b._h, ptr(bases), ptr(offsets), len(offsets) - 1))
    return b, b.finish(1, 0)


rng = np.random.default_rng(901)
genome = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, GENOME_BP, dtype=np.uint8)]
g_off = np.linspace(0, GENOME_BP, 9).astype(np.uint64)
comp = np.zeros(256, np.uint8)
comp[list(b"ACGT")] = list(b"TGCA")
reads = np.empty(N_READS * READ_LEN, np.uint8)
span = min(GENOME_BP, 50_000_000) - READ_LEN
for r0 in range(0, N_READS, 1_000_000):
    n = min(1_000_000, N_READS - r0)
    at = rng.integers(0, span, n)
    block = genome[at[:, None] + np.arange(READ_LEN)[None, :]]
    block[1::2] = comp[block[1::2, ::-1]]
    reads[r0 * READ_LEN:(r0 + n) * READ_LEN] = block.reshape(-1)
r_off = np.arange(N_READS + 1, dtype=np.uint64) * READ_LEN

for name, bases, offsets in (("genome", genome, g_off), ("reads", reads, r_off)):
    mbp = len(bases) / 1e6
    plain(bases, offsets).close()  # warm-up: code objects, the host pool
    tp, tc, last = [], [], None
    for _ in range(REPS):
        t, idx = timed(lambda: plain(bases, offsets))
        tp.append(t)
        n_plain = idx.n_keys
        idx.close()
        if last:
            last[0].close()
        t, last = timed(lambda: counted(bases, offsets))
        tc.append(t)
        assert last[1].n_keys == n_plain
        last[1].close()
        print(f"  {name} rep: plain {tp[-1]:.3f} s, counting {tc[-1]:.3f} s", flush=True)
    b = last[0]
    info = b.info()
    mp, mc = statistics.median(tp), statistics.median(tc)
    print(f"{name}: {mbp:.0f} Mbp, {len(offsets) - 1} sequences, {info['n_keys']} keys, {info['n_occurrences']} occurrences, "
          f"builder {info['device_bytes'] / 1e9:.2f} GB")
    print(f"  dcn_index_build                  median {mp:.3f} s (min {min(tp):.3f})  {mbp / mp:.0f} Mbp/s")
    print(f"  builder create + add + finish(1,0) median {mc:.3f} s (min {min(tc):.3f})  {mbp / mc:.0f} Mbp/s  ({mc / mp:.2f} x the plain build)")
    tf = [timed(lambda: b.finish(2, 0))[0] for _ in range(REPS)]
    th = [timed(lambda: b.hist(256))[0] for _ in range(REPS)]
    print(f"  finish(2,0) alone median {statistics.median(tf) * 1e3:.1f} ms ({b.finish(2, 0, count_only=True)} keys kept), "
          f"hist(256) median {statistics.median(th) * 1e3:.1f} ms")
    b.close()
    os.environ["DCN_INDEX_TIMING"] = "1"
    for _ in range(SPLIT_REPS):
        sys.stdout.flush()
        t, idx = timed(lambda: plain(bases, offsets))
        idx.close()
        t2, (b, idx) = timed(lambda: counted(bases, offsets))
        idx.close()
        b.close()
        sys.stderr.flush()
        print(f"  {name} split rep (the two lines above): plain {t:.3f} s, counting {t2:.3f} s", flush=True)
    del os.environ["DCN_INDEX_TIMING"]

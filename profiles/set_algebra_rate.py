#!/usr/bin/env python3
"""Set algebra on the index side: three members of 50 M mix64 keys each, A = ids [1, 50 M],
B = ids (25 M, 75 M], C = ids (40 M, 90 M] (A n B 25 M, A n C 10 M, B n C 35 M, A n B n C 10 M keys).  Medians of REPS
wall-clock times (every call is blocking) of
  dcn_index_set_create over the three, dcn_index_set_overlap, a counting and a building dcn_index_set_select
  (the keys at least two members hold), dcn_index_intersect of A and B,
and, alternating with that intersect in the same process, what a user had to do before: a.diff(a.diff(b)) through
dcn_index_diff.  With each sweep, the bytes it must stream: 4 B per slot of masks, plus 8 B per selected key.
Needs no reference data and no downloads.
usage: python profiles/set_algebra_rate.py [keys_per_member]"""
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

REPS = 5
K, W = 31, 15
M1, M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def mix64(lo, hi):  # splitmix64's finalizer, as tests/conftest.py and bench.py
    z = np.arange(lo, hi, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * M1
        z = (z ^ (z >> np.uint64(27))) * M2
        return z ^ (z >> np.uint64(31))


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return time.perf_counter() - t0, r


def median_of(f, keep=False):
    ts, last = [], None
    for _ in range(REPS):
        if last is not None and hasattr(last, "close"):
            last.close()
        t, last = timed(f)
        ts.append(t)
    if not keep and hasattr(last, "close"):
        last.close()
        last = None
    return statistics.median(ts), min(ts), last


n = int(sys.argv[1]) if len(sys.argv) > 1 else 50_000_000
ranges = [(1, n + 1), (n // 2 + 1, n // 2 + n + 1), (4 * n // 5 + 1, 4 * n // 5 + n + 1)]
members = []
for j, (lo, hi) in enumerate(ranges):
    t, idx = timed(lambda: dcn.Index.from_keys(mix64(lo, hi), K, W))
    members.append(idx)
    print(f"member {j}: ids [{lo:,}, {hi:,}), {len(idx):,} keys, table {idx.table_bytes / 1e9:.2f} GB, made in {t:.2f} s", flush=True)
a, b, c = members


def report(name, med, best, stream_bytes=None, note=""):
    rate = f", {stream_bytes / 1e9:.2f} GB to stream = {stream_bytes / med / 1e12:.2f} TB/s at the median" if stream_bytes else ""
    print(f"{name}: median {med * 1e3:.2f} ms, best {best * 1e3:.2f} ms of {REPS}{rate}{note}", flush=True)


med, best, s = median_of(lambda: dcn.IndexSet(members), keep=True)
n_slots = s.memory // 12  # 8 B of key + 4 B of mask per slot
print(f"set: {len(s):,} keys in {n_slots:,} slots, {s.memory / 1e9:.2f} GB (masks {4 * n_slots / 1e9:.2f} GB)")
report("dcn_index_set_create (3 members)", med, best)

med, best, ov = median_of(s.overlap)
print("shared:\n" + "\n".join("  " + " ".join(f"{int(x):>11,}" for x in row) for row in ov["shared"]))
print("exclusive: " + " ".join(f"{int(x):,}" for x in ov["exclusive"]) + "; by_count: " + " ".join(f"{int(x):,}" for x in ov["by_count"]))
report("dcn_index_set_overlap", med, best, 4 * n_slots)

med, best, n_core = median_of(lambda: s.select(min_members=2, count_only=True))
report(f"dcn_index_set_select, counting (min_members=2: {n_core:,} keys)", med, best, 4 * n_slots)

med, best, core = median_of(lambda: s.select(min_members=2), keep=True)
report(f"dcn_index_set_select, building ({len(core):,} keys into a table of {core.table_bytes / 1e9:.2f} GB)", med, best,
       2 * 4 * n_slots + 8 * len(core), " (two sweeps of the masks + the selected keys; the new table's clear and inserts on top)")
core.close()

t_new, t_old = [], []
for _ in range(REPS):  # alternating in the same process
    t, r = timed(lambda: dcn.Index.intersect([a, b]))
    n_new = len(r)
    r.close()
    t_new.append(t)

    def two_diffs():
        only_a = a.diff(b)
        r = a.diff(only_a)
        only_a.close()
        return r
    t, r = timed(two_diffs)
    n_old = len(r)
    r.close()
    t_old.append(t)
assert n_new == n_old, (n_new, n_old)
slots_a = a.table_bytes // 8
report(f"dcn_index_intersect(A, B) ({n_new:,} keys)", statistics.median(t_new), min(t_new), 2 * 8 * slots_a + slots_a // 4,
       " (A's slots twice + the bitmap written and read; one probe of B per key of A on top)")
report(f"a.diff(a.diff(b)) through dcn_index_diff ({n_old:,} keys)", statistics.median(t_old), min(t_old))
print(f"intersect / two diffs: {statistics.median(t_new) / statistics.median(t_old):.2f} of the time")

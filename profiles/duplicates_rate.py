#!/usr/bin/env python3
"""What dcn_mark_duplicates_batch costs.  The rows are made here, field by field (no placement): UNITS single units per call
on one record, strand and unclipped 5' coordinate uniform in 3 * 10^9, each clipped by 0 .. 7 bases; with probability `rate`
a unit repeats the end of an earlier unit of the same call that is not itself a repeat.  The map keeps no bases (the set
needs none), so the coordinates are checked against nothing.
    empty table     the set is reset in front of every call: medians of REPS calls after one untimed call, per rate
    100 M keys      ten untimed calls of distinct keys first; then, per rate, REPS calls one behind the other (the set cannot
                    be put back, so the table holds 100 M keys at the first and up to 100 M + 9 * UNITS at the last)
each as host time around the blocking call: the host's walk over the rows (checks, first placed row per read), 40 B per read
to the device, the three kernels, 9 B per unit back.  A call that makes the table or the log grow is reported apart.
    kernels         one call per rate under `rocprofv3 --kernel-trace --stats` in a run of its own: dup_keys_kernel,
                    dup_insert_kernel, dup_lookup_kernel and dup_rehash_kernel from its statistics.  The call is blocking
                    and copies between any two events of a caller, so device events around the kernels cannot be taken
                    from outside it.
    cli REF FASTQ [PARENT_TOOL]   wall time of `deacon-hip markdup --keep-duplicates` against `deacon-hip genotype` (of
                    PARENT_TOOL when given: the tool of the commit before this mode) on the same file, medians of 3.
    make-cli DIR    writes DIR/ref.fa (2 Mbp) and DIR/reads.fq (400,000 x 150 bp, a tenth of them repeats) for `cli`.
usage: python profiles/duplicates_rate.py [units] [kernels | cli ... | make-cli DIR]"""
import os
import statistics
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, ".")

ARGS = sys.argv[1:]
UNITS = int(ARGS[0]) if ARGS and ARGS[0].isdigit() else 10_000_000
REPS = 5
RATES = (0.0, 0.1, 0.5)
CLI = os.path.join("deacon-server_amd", "bin", "deacon-hip")


def make_cli(d):
    rng = np.random.default_rng(20)
    os.makedirs(d, exist_ok=True)
    ref = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 2_000_000)]
    with open(os.path.join(d, "ref.fa"), "wb") as f:
        f.write(b">chr1\n" + ref.tobytes() + b"\n")
    comp = np.zeros(256, np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    n = 400_000
    starts = rng.integers(0, len(ref) - 150, n)
    repeat = rng.random(n) < 0.1
    starts[repeat] = starts[rng.integers(0, n, int(repeat.sum()))]
    rev = rng.random(n) < 0.5
    with open(os.path.join(d, "reads.fq"), "wb") as f:
        for i in range(n):
            s = ref[starts[i]:starts[i] + 150].copy()
            err = rng.random(150) < 0.005
            s[err] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(err.sum()))]
            if rev[i]:
                s = comp[s[::-1]]
            q = (rng.integers(20, 41, 150) + 33).astype(np.uint8)
            f.write(b"@r%d\n" % i + s.tobytes() + b"\n+\n" + q.tobytes() + b"\n")
    print(f"{d}: ref.fa 2,000,000 bp, reads.fq {n:,} x 150 bp, {int(repeat.sum()):,} repeats", flush=True)


def time_cli(ref, fastq, parent):
    def wall(tool, mode, extra):
        times = []
        for rep in range(4):
            t = time.perf_counter()
            subprocess.run([tool, mode, ref, fastq, "-q", "--vcf", "/dev/null", "-s", "/tmp/duplicates_rate_summary.json"] + extra, check=True)
            times.append(time.perf_counter() - t)
        return times[1:]  # (the first run warms the file cache and the device)
    a = wall(parent or CLI, "genotype", [])
    b = wall(CLI, "markdup", ["--keep-duplicates"])
    print(f"genotype ({'the parent commit' if parent else 'this build'}), wall: median {statistics.median(a):.3f} s of {sorted(round(x, 3) for x in a)}")
    print(f"markdup --keep-duplicates, wall: median {statistics.median(b):.3f} s of {sorted(round(x, 3) for x in b)}")
    print(f"the marking adds {100 * (statistics.median(b) / statistics.median(a) - 1):+.1f} % of genotype's wall time", flush=True)
    print(open("/tmp/duplicates_rate_summary.json").read().split('"time"')[0][-400:])


if "make-cli" in ARGS:
    make_cli(ARGS[ARGS.index("make-cli") + 1])
    sys.exit(0)
if "cli" in ARGS:
    rest = ARGS[ARGS.index("cli") + 1:]
    time_cli(rest[0], rest[1], rest[2] if len(rest) > 2 else None)
    sys.exit(0)

import deacon_server_amd as dcn  # noqa: E402

KERNELS_ONLY = "kernels" in ARGS
rng = np.random.default_rng(20)
record = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 100_000)].copy()
index = dcn.Index.build([record], 31, 15, device=0)
amap = dcn.AnchorMap(index, keep_bases=False)
amap.add_records([record])
amap.duplicates_enable()
DT = dcn.filter.PLACEMENT_DTYPE
offsets = (np.arange(UNITS + 1, dtype=np.uint64) * 150)


def make_rows(rate, salt):
    """UNITS rows: unit u repeats, with probability `rate`, the end of an earlier unit that is not a repeat"""
    g = np.random.default_rng(1000 + salt)
    pos = g.integers(0, 3_000_000_000, UNITS).astype(np.int64) + salt * 4_000_000_000  # (no two calls share an end)
    rev = g.integers(0, 2, UNITS).astype(np.uint32)
    if rate > 0:
        copy = g.random(UNITS) < rate
        copy[0] = False
        originals = np.flatnonzero(~copy)
        before = np.cumsum(~copy) - (~copy)  # originals in front of each unit
        pick = originals[(g.random(UNITS) * np.maximum(before, 1)).astype(np.int64)]
        src = np.where(copy, pick, np.arange(UNITS))
        pos, rev = pos[src], rev[src]
    clip = g.integers(0, 8, UNITS).astype(np.int64)
    rows = np.zeros(UNITS, DT)
    rows["reverse"] = rev
    rows["read_start"] = clip
    rows["read_end"] = 150
    fwd = rev == 0
    rows["ref_start"] = np.where(fwd, pos + clip, pos - 150 + 1_000)
    rows["ref_end"] = np.where(fwd, pos + 150, pos - clip + 1_000)
    return rows


def call(rows):
    t = time.perf_counter()
    dup, first = amap.mark_duplicates(offsets, rows)
    return time.perf_counter() - t, int(dup.sum())


def report(name, rate, times, n_dup, note=""):
    med = statistics.median(times)
    print(f"{name:>11}  {100 * rate:3.0f} % asked, {100 * n_dup / UNITS:5.2f} % marked: median {1e3 * med:8.2f} ms of {len(times)} "
          f"({1e3 * min(times):.2f} - {1e3 * max(times):.2f}), {UNITS / med / 1e6:7.2f} M units/s{note}", flush=True)


print(f"{UNITS:,} single units per call, rows of {DT.itemsize} B; host time around AnchorMap.mark_duplicates", flush=True)
salt = 0
for rate in RATES:
    rows = make_rows(rate, salt)
    salt += 1
    amap.duplicates_reset()
    first_time, n_dup = call(rows)  # untimed for the table: the set grows here
    times = []
    for rep in range(1 if KERNELS_ONLY else REPS):
        amap.duplicates_reset()
        t, n = call(rows)
        assert n == n_dup
        times.append(t)
    report("empty table", rate, times, n_dup, f"; the first call, which sized the set: {1e3 * first_time:.2f} ms")
if KERNELS_ONLY:
    sys.exit(0)
amap.duplicates_reset()
t0 = time.perf_counter()
for i in range(100_000_000 // UNITS):
    rows = make_rows(0.0, salt)
    salt += 1
    call(rows)
print(f"preload: {amap.duplicates_info()} (seen, keyed, keys) in {time.perf_counter() - t0:.1f} s with making the rows", flush=True)
for rate in RATES:
    times, grew = [], []
    for rep in range(3):
        rows = make_rows(rate, salt)
        salt += 1
        t, n_dup = call(rows)
        times.append(t)
    report("100 M keys", rate, times, n_dup, f"; keys behind them: {amap.duplicates_info()[2]:,}")

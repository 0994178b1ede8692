#!/usr/bin/env python3
"""Classification against N indexes in one pass (dcn_classify_batch_device) against N separate counting filter passes
(dcn_filter_batch_device with hits and totals) on the same device-resident batch: BASELINE configs[1]'s shape (10 M x
150 bp, half drawn from a 64 Mbp host genome, as bench.py).  Members: a panhuman-sized member 0 (bench.py's index: the host
genome's minimizers + mix64 keys up to 409.9 M) and N - 1 members of 50 M keys (every (j+1)-th host key + mix64 keys of a
range of their own), so that host reads hit several members.  For N = 1, 2, 4, 8: the set's device memory and build time,
then classify and the N filter passes timed alternately (wall clock around enqueue + synchronize, best and median of REPS),
and one profiled classify call for the stage split (pack, plan, dump scan, lane kernel, workgroup kernel).
--coverage: for N = 1 and 8 only, classify with coverage off, then on (dcn_index_set_coverage_enable) right after a reset
(every key the batch hits is seen first: test-loads and atomics) and again (every key already marked: test-loads only),
timed alternately; the enable cost (bitmap + keys sweep), the read-out sweeps (coverage(), observed_keys()) and the stage
split with coverage on.
--depth [--parent-tree DIR]: for N = 1 and 8 only, and without the filter passes: classify with depth off, then on
(dcn_index_set_depth_enable) right after a reset (every counter starts at zero) and again (counters warm), timed
alternately; the enable cost, the three read-out sweeps (depth_stats(), depth_hist(), depth_keys()) and the stage split
with depth on (the counting sweep is timed in the lane kernel's slot).  With --parent-tree, a checkout of the parent commit
with its library built is loaded beside this one (its package under another name, its library through DCN_LIB_PATH), builds
the same set, and its classify call alternates with this tree's depth-off call: the existing kernels are untouched, so the
two agree within the spread of the parent's own calls.
usage: python profiles/classify_rate.py [reads] [--coverage | --depth [--parent-tree DIR]]"""
import importlib.util
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
import bench as B  # noqa: E402
import deacon_server_amd as dcn  # noqa: E402

REPS = 5
COVERAGE = "--coverage" in sys.argv[1:]
DEPTH = "--depth" in sys.argv[1:]
args = [a for a in sys.argv[1:] if a not in ("--coverage", "--depth")]
PARENT_TREE = None
if "--parent-tree" in args:
    PARENT_TREE = args[args.index("--parent-tree") + 1]
    del args[args.index("--parent-tree"):args.index("--parent-tree") + 2]
reads = int(args[0]) if args else 10_000_000
dev = torch.device("cuda", 0)
genome = B.make_host_genome(64_000_000, 3, dev)
member0, keys0, host_keys, _, build0 = B.build_index(genome, B.PANHUMAN_KEYS, 0)
member_keys = [keys0 if PARENT_TREE else None]  # what the parent tree's copy of each member is built from
del keys0
batch = B.make_batches("short", genome, reads, 5, dev, rotate=1)[0]
n_reads, n_bases = batch.n_reads, batch.n_bases
print(f"batch: {n_reads:,} reads, {n_bases / 1e6:.1f} Mbp, device-resident ASCII; member 0: {member0.n_keys:,} keys "
      f"({member0.table_bytes / 1e9:.1f} GB, built in {build0:.1f} s)", flush=True)

members = [member0]
for j in range(1, 8):
    t0 = time.time()
    hk = host_keys[::j + 1]
    rnd = B.mix64_device((1 << 40) + (j << 32), 50_000_000 - len(hk), dev).cpu().numpy().view(np.uint64)
    member_keys.append(np.concatenate([hk, rnd]))
    members.append(dcn.Index.from_keys(member_keys[-1], B.K, B.W))
    if not PARENT_TREE:
        member_keys[-1] = None
    print(f"member {j}: {members[-1].n_keys:,} keys ({len(hk):,} host), {members[-1].table_bytes / 1e9:.1f} GB, "
          f"built in {time.time() - t0:.1f} s", flush=True)

dcn_parent, parent_members = None, []
if PARENT_TREE:
    pkg = os.path.join(PARENT_TREE, "deacon-server_amd")
    os.environ["DCN_LIB_PATH"] = os.path.join(pkg, "lib", "libdeacon_hip.so")
    spec = importlib.util.spec_from_file_location("dcn_parent", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    dcn_parent = importlib.util.module_from_spec(spec)
    sys.modules["dcn_parent"] = dcn_parent
    spec.loader.exec_module(dcn_parent)
    del os.environ["DCN_LIB_PATH"]
    print(f"parent tree: {dcn_parent._native.LIB_PATH}, ABI {dcn_parent._native.ABI} (this tree: {dcn._native.LIB_PATH}, "
          f"ABI {dcn._native.ABI})", flush=True)

procs = []  # one counting context per member, created once
for m in ([] if DEPTH else members):
    procs.append(dcn.FilterProcessor(m, max_batch_bases=n_bases, max_batch_reads=n_reads))
d_hits = torch.zeros(n_reads, dtype=torch.int32, device=dev)
d_total = torch.zeros(n_reads, dtype=torch.int32, device=dev)


def filter_pass(n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for p in procs[:n]:
        p.filter_batch_device(batch.d_bases.data_ptr(), batch.d_offsets.data_ptr(), n_reads, n_bases,
                              batch.d_keep.data_ptr(), d_hits.data_ptr(), d_total.data_ptr())
        p.synchronize()
    return time.perf_counter() - t0


def coverage_leg(n, s, clf, classify_pass):
    """coverage off / on after a reset / on with every key marked, alternately; then the sweeps and the stage split"""
    t_off, t_cold, t_warm, t_enable = [], [], [], []
    for _ in range(REPS):
        t_off.append(classify_pass())
        t0 = time.perf_counter()
        s.enable_coverage()
        t_enable.append(time.perf_counter() - t0)
        t_cold.append(classify_pass())
        t_warm.append(classify_pass())
        s.enable_coverage(False)
    s.enable_coverage()
    classify_pass()
    t0 = time.perf_counter()
    observed, keys = s.coverage()
    t_cov = time.perf_counter() - t0
    t0 = time.perf_counter()
    any_keys = s.observed_keys()
    t_keys = time.perf_counter() - t0
    clf.set_profiling(True)
    s.reset_coverage()
    classify_pass()
    cold_stages, _ = clf.profile()
    clf.set_profiling(False)
    clf.set_profiling(True)
    classify_pass()
    warm_stages, _ = clf.profile()
    clf.set_profiling(False)
    s.enable_coverage(False)
    med = lambda t: statistics.median(t) * 1e3  # noqa: E731
    r = {"n": n, "off_ms_median": med(t_off), "cold_ms_median": med(t_cold), "warm_ms_median": med(t_warm),
         "off_ms_best": min(t_off) * 1e3, "cold_ms_best": min(t_cold) * 1e3, "warm_ms_best": min(t_warm) * 1e3,
         "enable_ms_median": med(t_enable), "coverage_sweep_ms": t_cov * 1e3, "observed_keys_ms": t_keys * 1e3,
         "observed": observed.tolist(), "keys": keys.tolist(), "observed_any": len(any_keys),
         "cold_stages_ms": {k: round(v, 3) for k, v in cold_stages.items()},
         "warm_stages_ms": {k: round(v, 3) for k, v in warm_stages.items()}}
    print(f"coverage N={n}: classify off {r['off_ms_median']:.2f} ms median ({r['off_ms_best']:.2f} best) | on, after reset "
          f"{r['cold_ms_median']:.2f} ms ({r['cold_ms_best']:.2f}) = {r['cold_ms_median'] / r['off_ms_median']:.2f}x | on, "
          f"keys marked {r['warm_ms_median']:.2f} ms ({r['warm_ms_best']:.2f}) = {r['warm_ms_median'] / r['off_ms_median']:.2f}x"
          f" | enable {r['enable_ms_median']:.1f} ms | coverage() {r['coverage_sweep_ms']:.1f} ms | observed_keys() "
          f"{r['observed_keys_ms']:.1f} ms for {r['observed_any']:,} keys | observed/keys per member "
          f"{list(zip(r['observed'], r['keys']))} | stages (ms) after reset {r['cold_stages_ms']} | keys marked "
          f"{r['warm_stages_ms']}", flush=True)
    return r


def depth_leg(n, s, clf, classify_pass):
    """depth off / on after a reset / on with warm counters, alternately (and the parent tree's call, when given); then the
    sweeps and the stage split"""
    parent_pass = None
    if dcn_parent:
        while len(parent_members) < n:
            parent_members.append(dcn_parent.Index.from_keys(member_keys[len(parent_members)], B.K, B.W))
        ps = dcn_parent.IndexSet(parent_members[:n])
        pclf = dcn_parent.Classifier(ps, max_batch_bases=n_bases, max_batch_reads=n_reads)
        p_m = torch.zeros(n_reads, dtype=torch.int32, device=dev)
        p_h = torch.zeros(n_reads * n, dtype=torch.int32, device=dev)
        p_t = torch.zeros(n_reads, dtype=torch.int32, device=dev)

        def parent_pass():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pclf.classify_batch_device(batch.d_bases.data_ptr(), batch.d_offsets.data_ptr(), n_reads, n_bases,
                                       p_m.data_ptr(), p_h.data_ptr(), p_t.data_ptr())
            pclf.synchronize()
            return time.perf_counter() - t0
        parent_pass()
    t_off, t_parent, t_cold, t_warm, t_enable = [], [], [], [], []
    for _ in range(REPS):
        t_off.append(classify_pass())
        if parent_pass:
            t_parent.append(parent_pass())
        t0 = time.perf_counter()
        s.enable_depth()
        t_enable.append(time.perf_counter() - t0)
        t_cold.append(classify_pass())
        t_warm.append(classify_pass())
        s.enable_depth(False)
    s.enable_depth()
    classify_pass()
    t0 = time.perf_counter()
    stats = s.depth_stats()
    t_stats = time.perf_counter() - t0
    t0 = time.perf_counter()
    hist = s.depth_hist(None, 4096)
    t_hist = time.perf_counter() - t0
    t0 = time.perf_counter()
    any_keys, any_depths = s.depth_keys()
    t_keys = time.perf_counter() - t0
    stages = {}
    for name in ("cold", "warm"):
        if name == "cold":
            s.reset_depth()
        clf.set_profiling(True)
        classify_pass()
        stages[name] = {k: round(v, 3) for k, v in clf.profile()[0].items()}
        clf.set_profiling(False)
    s.enable_depth(False)
    med = lambda t: statistics.median(t) * 1e3  # noqa: E731
    r = {"n": n, "off_ms_median": med(t_off), "off_ms_min": min(t_off) * 1e3, "off_ms_max": max(t_off) * 1e3,
         "cold_ms_median": med(t_cold), "warm_ms_median": med(t_warm), "enable_ms_median": med(t_enable),
         "stats_ms": t_stats * 1e3, "hist_ms": t_hist * 1e3, "keys_ms": t_keys * 1e3, "observed_any": len(any_keys),
         "observed": stats["observed"].tolist(), "sum": stats["sum"].tolist(), "saturated": stats["saturated"].tolist(),
         "max_depth": int(any_depths.max()) if len(any_depths) else 0, "unobserved_any": int(hist[0]), "stages_ms": stages}
    line = (f"depth N={n}: classify off {r['off_ms_median']:.2f} ms median ({r['off_ms_min']:.2f}-{r['off_ms_max']:.2f})")
    if parent_pass:
        r.update(parent_ms_median=med(t_parent), parent_ms_min=min(t_parent) * 1e3, parent_ms_max=max(t_parent) * 1e3,
                 parent_outputs_equal=bool(torch.equal(p_m, d_m) and torch.equal(p_h, d_h) and torch.equal(p_t, d_t)))
        line += (f" | parent commit's library {r['parent_ms_median']:.2f} ms median ({r['parent_ms_min']:.2f}-"
                 f"{r['parent_ms_max']:.2f}), outputs equal: {r['parent_outputs_equal']}")
        pclf.close()
        ps.close()
    print(line + f" | on, after reset {r['cold_ms_median']:.2f} ms = {r['cold_ms_median'] / r['off_ms_median']:.2f}x | on, "
          f"counters warm {r['warm_ms_median']:.2f} ms = {r['warm_ms_median'] / r['off_ms_median']:.2f}x | enable "
          f"{r['enable_ms_median']:.1f} ms | depth_stats() {r['stats_ms']:.1f} ms | depth_hist(4096) {r['hist_ms']:.1f} ms | "
          f"depth_keys() {r['keys_ms']:.1f} ms for {r['observed_any']:,} keys (max depth {r['max_depth']}) | per member "
          f"observed {r['observed']} sum {r['sum']} saturated {r['saturated']} | stages (ms) after reset "
          f"{stages['cold']} | warm {stages['warm']}", flush=True)
    return r


rows = []
for n in ((1, 8) if COVERAGE or DEPTH else (1, 2, 4, 8)):
    t0 = time.time()
    s = dcn.IndexSet(members[:n])
    set_build = time.time() - t0
    clf = dcn.Classifier(s, max_batch_bases=n_bases, max_batch_reads=n_reads)
    d_m = torch.zeros(n_reads, dtype=torch.int32, device=dev)
    d_h = torch.zeros(n_reads * n, dtype=torch.int32, device=dev)
    d_t = torch.zeros(n_reads, dtype=torch.int32, device=dev)

    def classify_pass():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        clf.classify_batch_device(batch.d_bases.data_ptr(), batch.d_offsets.data_ptr(), n_reads, n_bases, d_m.data_ptr(),
                                  d_h.data_ptr(), d_t.data_ptr())
        clf.synchronize()
        return time.perf_counter() - t0

    if DEPTH:
        classify_pass()
        rows.append({"n": n, "depth": depth_leg(n, s, clf, classify_pass)})
        clf.close()
        s.close()
        del d_m, d_h, d_t
        torch.cuda.empty_cache()
        continue
    classify_pass()
    filter_pass(n)
    tc, tf = [], []
    for _ in range(REPS):
        tc.append(classify_pass())
        tf.append(filter_pass(n))
    clf.set_profiling(True)
    classify_pass()
    stages, _ = clf.profile()
    clf.set_profiling(False)
    # consistency: member 0's column equals the last counting pass over member 0
    procs[0].filter_batch_device(batch.d_bases.data_ptr(), batch.d_offsets.data_ptr(), n_reads, n_bases,
                                 batch.d_keep.data_ptr(), d_hits.data_ptr(), d_total.data_ptr())
    procs[0].synchronize()
    same = bool(torch.equal(d_h.view(n_reads, n)[:, 0], d_hits) and torch.equal(d_t, d_total))
    matched = [int(((d_m >> j) & 1).sum()) for j in range(n)]
    r = {"n": n, "set_keys": s.n_keys, "set_gb": s.memory / 1e9, "set_build_s": set_build,
         "classify_ms_best": min(tc) * 1e3, "classify_ms_median": statistics.median(tc) * 1e3,
         "filter_n_ms_best": min(tf) * 1e3, "filter_n_ms_median": statistics.median(tf) * 1e3,
         "stages_ms": {k: round(v, 3) for k, v in stages.items()}, "member0_column_equals_filter": same,
         "units_matched": matched}
    r["classify_mbps"] = n_bases / (r["classify_ms_median"] / 1e3) / 1e6
    r["filter_n_mbps"] = n_bases / (r["filter_n_ms_median"] / 1e3) / 1e6
    r["speedup_vs_n_filters"] = r["filter_n_ms_median"] / r["classify_ms_median"]
    rows.append(r)
    if COVERAGE:
        r["coverage"] = coverage_leg(n, s, clf, classify_pass)
    print(f"N={n}: set {s.n_keys:,} keys, {r['set_gb']:.1f} GB (slots + masks), built in {set_build:.1f} s | classify "
          f"{r['classify_ms_median']:.2f} ms median ({r['classify_ms_best']:.2f} best) = {r['classify_mbps']:,.0f} Mbp/s | "
          f"{n} counting filter passes {r['filter_n_ms_median']:.2f} ms median ({r['filter_n_ms_best']:.2f} best) = "
          f"{r['filter_n_mbps']:,.0f} Mbp/s | {r['speedup_vs_n_filters']:.2f}x | stages (ms) {r['stages_ms']} | "
          f"member 0 column == filter: {same} | units matched per member {matched}", flush=True)
    clf.close()
    s.close()
    del d_m, d_h, d_t
    torch.cuda.empty_cache()

if DEPTH:
    print("depth summary: " + "; ".join(
        f"N={r['n']}: on/off {r['depth']['cold_ms_median'] / r['depth']['off_ms_median']:.2f}x after reset, "
        f"{r['depth']['warm_ms_median'] / r['depth']['off_ms_median']:.2f}x warm" for r in rows), flush=True)
    sys.exit(0)
t1 = rows[0]["classify_ms_median"]
print("summary: " + "; ".join(f"N={r['n']}: {r['classify_ms_median'] / t1:.2f}x the time of N=1, "
                              f"{r['speedup_vs_n_filters']:.2f}x faster than {r['n']} filter passes" for r in rows), flush=True)
if COVERAGE:
    print("coverage summary: " + "; ".join(
        f"N={r['n']}: on/off {r['coverage']['cold_ms_median'] / r['coverage']['off_ms_median']:.2f}x after reset, "
        f"{r['coverage']['warm_ms_median'] / r['coverage']['off_ms_median']:.2f}x with keys marked, sweep "
        f"{r['coverage']['coverage_sweep_ms']:.1f} ms" for r in rows), flush=True)

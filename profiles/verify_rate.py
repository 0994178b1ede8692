#!/usr/bin/env python3
"""Verified placements (dcn_verify_batch) behind split placements (dcn_place_split_batch) on the same host batch, on one
context in one process.  The map, the genome and the two workloads are profiles/place_rate.py's: the 64 Mbp synthetic host
genome as one record, its own minimizers as keys;
  short  reads x 150 bp, half drawn from the host genome
  long   bench.py's long-read shape (lognormal, mean 10 kbp), half of the reads host-derived with 5 % substitutions
place_split_batch alone and place_split_batch + verify_batch alternate, medians of REPS after one untimed call of each.
Both are the blocking host forms on pageable memory: the wall clock of a call includes staging the batch over PCIe and the
copies back.  The verify call stages and packs the batch a second time; its device time (dcn_ctx_profile: pack in its slot,
the verify kernel in FINISH) is stated beside its wall time, and the rest of the wall time -- the host's walk over the rows,
the second staging of the batch, the rows' way to the device and the edits' way back -- is what a device-resident hand-over
from the vote would save.  The script also runs dcn_place_split_batch on a map that keeps bases and on one that does not
and prints both stage splits, to be read against profiles/place_split_rate.txt (no kernel of that call is edited).
usage: python profiles/verify_rate.py [short_reads] [long_bases]"""
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
import bench as B  # noqa: E402
import deacon_server_amd as dcn  # noqa: E402

REPS = 5
N = 4  # max_placements, profiles/place_split_rate.py's last row
short_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
long_bases = int(sys.argv[2]) if len(sys.argv) > 2 else 1_500_000_000
dev = torch.device("cuda", 0)
genome = B.make_host_genome(64_000_000, 3, dev)
host = genome.cpu().numpy()
index = dcn.Index.build([host], B.K, B.W, device=0)
maps = {}
for keep in (False, True):
    t0 = time.perf_counter()
    maps[keep] = dcn.AnchorMap(index, keep_bases=keep)
    maps[keep].add_records([host])
    print(f"map (keep_bases={keep}): {maps[keep].info()} | create + add of the 64 Mbp record {1e3 * (time.perf_counter() - t0):.1f} ms wall "
          f"(the first one includes the context){' | store: %.1f MB' % (len(host) * 0.375 / 1e6) if keep else ''}", flush=True)
assert maps[True].fetch(0, 1_000_003, 77) == host[1_000_003:1_000_080].tobytes()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def stages_of(obj, fn):
    obj.set_profiling(True)
    fn()
    st, _ = obj.profile()
    obj.set_profiling(False)
    return {k: round(v, 3) for k, v in st.items()}


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
    out = {}
    plain = dcn.Placer(maps[False], max_batch_bases=n_bases, max_batch_reads=n_reads)
    plain.place_split_batch(bases, offsets, max_placements=N)
    s_plain = stages_of(plain, lambda: plain.place_split_batch(bases, offsets, max_placements=N))
    plain.close()
    plc = dcn.Placer(maps[True], max_batch_bases=n_bases, max_batch_reads=n_reads)

    def split():
        out["po"], out["rows"], _ = plc.place_split_batch(bases, offsets, max_placements=N)

    def verify():
        out["edits"] = plc.verify_batch(bases, offsets, out["rows"], row_offsets=out["po"])

    def both():
        split()
        verify()

    split()
    both()
    ts, tb, tv = [], [], []
    for _ in range(REPS):
        ts.append(timed(split))
        tb.append(timed(both))
    for _ in range(REPS):
        tv.append(timed(verify))
    s_keep, s_verify = stages_of(plc, split), stages_of(plc, verify)
    edits, rows = out["edits"], out["rows"]
    ok = edits < dcn.VERIFY_OVER
    extent = np.maximum(rows["read_end"] - rows["read_start"], (rows["ref_end"] - rows["ref_start"]).astype(np.uint32))
    ms_, mb, mv = statistics.median(ts), statistics.median(tb), statistics.median(tv)
    dev_ms = s_verify["pack"] + s_verify["finish"]
    print(f"{name}: {n_reads:,} reads, {n_bases / 1e6:.1f} Mbp, host pageable, {len(rows):,} rows (N={N})\n"
          f"  split alone: {ms_ * 1e3:.2f} ms median ({min(ts) * 1e3:.2f} best) | stages (ms), map with kept bases {s_keep} | "
          f"map without {s_plain}\n"
          f"  split + verify: {mb * 1e3:.2f} ms median ({min(tb) * 1e3:.2f} best) = {n_bases / mb / 1e6:,.0f} Mbp/s, "
          f"{(mb - ms_) * 1e3:.2f} ms over split alone\n"
          f"  verify alone: {mv * 1e3:.2f} ms median ({min(tv) * 1e3:.2f} best) | stages (ms) {s_verify} | device pack {s_verify['pack']:.3f} + "
          f"kernel {s_verify['finish']:.3f} = {dev_ms:.3f} ms; the other {mv * 1e3 - dev_ms:.2f} ms are the host's walk over the rows, the "
          f"second staging of the batch ({n_bases / 1e6:.0f} MB of bases, {8 * (n_reads + 1) / 1e6:.0f} MB of offsets), {32 * len(rows) / 1e6:.0f} MB "
          f"of rows to the device and {4 * len(rows) / 1e6:.0f} MB of edits back\n"
          f"  verified {int(ok.sum()):,} of {len(rows):,} rows ({ok.mean():.1%}), mean edits {edits[ok].mean():.2f} over a mean extent of "
          f"{extent[ok].mean():.1f} bases, largest {int(edits[ok].max())}; {int((edits == dcn.VERIFY_OVER).sum()):,} over the threshold",
          flush=True)
    plc.close()
    del bases, offsets, out

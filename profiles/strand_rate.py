#!/usr/bin/env python3
"""What the strand planes cost in the pile-up, and what the two read-outs take.
  The workload is profiles/left_align_rate.py's short one (the 64 Mbp synthetic host genome as one record, reads x 150 bp,
single bases taken out of the reads at the rate of their insertions, the rows of one dcn_place_split_batch call at N = 4,
qualities of 30 throughout), twice: as it is there, `forward only` (bench.py cuts every read from the forward strand), and
`half reverse`, every other read as its reverse complement, the same bases taken out.  Two maps over the same index and
record, both with quality sums and both ledgers: the strand planes off and on.  dcn_pileup_batch_qual alternates between
them; after one untimed call of each, the median of REPS with best and worst, host clocks around calls that end in a
synchronise, and FINISH from dcn_ctx_profile.  With a second argument, the path of another build's library (the parent
commit's), the script only times the planes-off calls through that library, by the same protocol, and prints the lines to
compare: the off path of this build must stay within the run-to-run spread.
(A map without planes launches the kernels it launched before, instruction for instruction: pileup.hip.)
  The read-outs run over the record in stretches of 2^20 bases, as profiles/indels_rate.py's do: dcn_anchor_map_strand_evidence
at the sites of dcn_anchor_map_genotype (collected before the clock starts), and dcn_anchor_map_indels_strand at the sites of
dcn_anchor_map_indels_genotype with every threshold at its loosest, so that the few hundred events of this workload give sites.
usage: python profiles/strand_rate.py [short_reads] [other_library]
       (writes profiles/strand_rate.txt beside what it prints; with other_library: strand_rate_parent.txt)"""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
OTHER = sys.argv[2] if len(sys.argv) > 2 else None
if OTHER:
    os.environ["DCN_LIB_PATH"] = OTHER  # (before the package loads its library)
import torch  # noqa: E402

import bench as B  # noqa: E402

import deacon_server_amd as dcn  # noqa: E402

if OTHER:
    dcn._native.ABI = (1, 22)  # the parent's library: the entry points this run calls are all older
    for name in ("dcn_anchor_map_pileup_keep_strands", "dcn_anchor_map_pileup_fetch_strands", "dcn_anchor_map_strand_evidence",
                 "dcn_anchor_map_indels_strand"):
        dcn._native._SIGNATURES.pop(name)  # ... and it does not export these

REPS = 5
N = 4
STRETCH = 1 << 20
short_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "strand_rate_parent.txt" if OTHER else "strand_rate.txt")
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
        m.pileup_keep_strands()
    maps[kind] = m
say("library: " + ("another build's, given on the command line" if OTHER else "this build's"))
say(f"map: {maps['off'].info()}")

batch = B.make_batches("short", genome, short_reads, 5, dev, rotate=1)[0]
bases0 = batch.d_bases.cpu().numpy()
offsets0 = batch.d_offsets.cpu().numpy().astype(np.uint64)
del batch
torch.cuda.empty_cache()
n_reads = len(offsets0) - 1
read_len = int(offsets0[1] - offsets0[0])
assert np.array_equal(offsets0, np.arange(n_reads + 1, dtype=np.uint64) * read_len)  # (every read has the same length)
placer = dcn.Placer(maps["off"], max_batch_bases=int(offsets0[-1]), max_batch_reads=n_reads)
po, rows, _ = placer.place_split_batch(bases0, offsets0, max_placements=N)
placer.pileup_batch(bases0, offsets0, rows, row_offsets=po, quals=np.full(len(bases0), 33 + 30, np.uint8))
ins_events = maps["off"].insertions_info()[0]
maps["off"].pileup_reset()
placer.close()
# the bench's reads are all forward.  `half reverse`: every other read as its reverse complement, so that half the rows take
# the branch that holds REV's add and rule S2's
complement = np.arange(256, dtype=np.uint8)
for x, y in zip(b"ACGTacgt", b"TGCAtgca"):
    complement[x] = y
mixed0 = bases0.reshape(n_reads, read_len).copy()
mixed0[1::2] = complement[mixed0[1::2, ::-1]]
mixed0 = mixed0.reshape(-1)
rng = np.random.default_rng(21)  # as many deleted bases, none of them a read's first (profiles/indels_rate.py)
gone = np.zeros(len(bases0), bool)
gone[rng.integers(0, len(bases0), ins_events)] = True
gone[offsets0[:-1].astype(np.int64)] = False
kept_before = np.concatenate(([0], np.cumsum(~gone)))
offsets = kept_before[offsets0.astype(np.int64)].astype(np.uint64)
n_bases = int(offsets[-1])
quals = np.full(n_bases, 33 + 30, np.uint8)
workloads = {"forward only": np.ascontiguousarray(bases0[~gone]), "half reverse": np.ascontiguousarray(mixed0[~gone])}
del bases0, mixed0
say(f"short: {n_reads:,} reads, {n_bases / 1e6:.1f} Mbp, host pageable; {ins_events:,} insertion events before, {int(gone.sum()):,} bases taken out")

placers = {kind: dcn.Placer(m, max_batch_bases=n_bases, max_batch_reads=n_reads) for kind, m in maps.items()}
for label, bases in workloads.items():
    po, rows, _ = placers["off"].place_split_batch(bases, offsets, max_placements=N)
    reverse_share = float(rows["reverse"].mean())
    calls = {kind: (lambda p=p: p.pileup_batch(bases, offsets, rows, row_offsets=po, quals=quals)) for kind, p in placers.items()}
    for m in maps.values():
        m.pileup_reset()
    n_added = {kind: fn()[1] for kind, fn in calls.items()}  # (untimed: buffers grow; the counters of this call are the ones read out below)
    assert len(set(n_added.values())) == 1
    say(f"{label}: {len(rows):,} rows (N={N}), {n_added['off']:,} added per call, {100 * reverse_share:.1f} % of the rows reverse")

    if not OTHER and label == "half reverse":  # the read-outs, over the counters of exactly one call
        m = maps["on"]
        length = len(host)
        stretches = [(s, min(STRETCH, length - s)) for s in range(0, length, STRETCH)]
        rev = int(m.pileup_fetch(0, 0, STRETCH)[:, dcn.PILEUP_REV].sum())
        planes = int(m.pileup_fetch_strands(0, 0, STRETCH).sum(dtype=np.int64))
        say(f"  first stretch: REV {rev:,}, RA + RC + RG + RT {planes:,}")
        geno = [m.genotype(0, s, n)[2] for s, n in stretches]
        queries = [m.strand_queries_of_genotypes(g) for g in geno]
        loose = dict(min_depth=1, min_gq=0, min_qual=0, min_count=1)
        indel = [m.indels_genotype(0, s, n, **loose) for s, n in stretches]
        m.strand_evidence(0, queries[0])
        t_ev, t_is = [], []
        for _ in range(REPS):
            t_ev.append(timed(lambda: [m.strand_evidence(0, q) for q in queries]))
            t_is.append(timed(lambda: [m.indels_strand(0, s, b) for s, b in indel]))
        ev = np.concatenate([m.strand_evidence(0, q) for q in queries])
        a_rev = np.concatenate([m.indels_strand(0, s, b) for s, b in indel])
        n_sites, n_indel = sum(len(g) for g in geno), sum(len(s) for s, _ in indel)
        flags = np.bincount(ev["flags"], minlength=4)
        say(f"  strand_evidence over the record, {len(stretches)} stretches, {n_sites:,} genotype sites: {spread(t_ev)}; "
            f"PASS {flags[0]:,}, strand_bias {flags[1]:,}, one_strand {flags[2]:,}, both {flags[3]:,}")
        say(f"  indels_strand over the record, {len(stretches)} stretches, {n_indel:,} indel sites (loosest thresholds) over "
            f"{m.insertions_info()[0]:,} + {m.deletions_info()[0]:,} events: {spread(t_is)}; {int(a_rev.sum()):,} reverse carriers of "
            f"{int(sum(int(s['count'].sum()) for s, _ in indel)):,}")

    times = {kind: [] for kind in calls}
    for _ in range(REPS):
        for kind, fn in calls.items():  # alternating
            times[kind].append(timed(fn))
    finish = {kind: [finish_of(placers[kind], fn) for _ in range(3)] for kind, fn in calls.items()}
    for kind in calls:
        say(f"  pileup_batch with qualities, both ledgers, strand planes {kind}: {spread(times[kind])} | FINISH {statistics.median(finish[kind]):.3f} ms "
            f"median of 3 ({min(finish[kind]):.3f} - {max(finish[kind]):.3f})")
    if not OTHER:
        med = {kind: statistics.median(t) * 1e3 for kind, t in times.items()}
        fin = {kind: statistics.median(t) for kind, t in finish.items()}
        say(f"  the planes add {med['on'] - med['off']:+.2f} ms of the call ({fin['on'] - fin['off']:+.3f} ms of FINISH, "
            f"{100 * (fin['on'] - fin['off']) / fin['off']:+.1f} %); the off call's own spread is {(max(times['off']) - min(times['off'])) * 1e3:.2f} ms")
for p in placers.values():
    p.close()
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")

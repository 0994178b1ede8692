"""The world of tests/test_gpu_geometry_sweep.py and tests/test_gpu_consumers_differential.py: for one (k, w) the three
genomes and members of tests/_depth_worker.py, their oracle indexes, one read batch with the edge reads every consumer of
the minimizer dump can get wrong, and what the per-feature models say about it.  Everything here is CPU only and comes
from the oracle and the models of the per-feature tests (_depth_worker.occurrences, _depth_track_worker.Model,
_place_worker.AnchorModel, _place_split_worker.place_split_all, _index_builder_worker.occurrences,
test_gpu_locate.model_batch); nothing is taken from the code under test.

The geometries, and why each is in the list:
  (31,15)   control: what the per-feature tests already pass
  (41,15)   the 128-bit scan (k > 32) with w = 15 specialised
  (56,2)    the largest k, generic w; plc_strand's 128-bit branch at hb = 48; most k-mers at the end of a batch
  (33,15)   just above the switch to the 128-bit scan
  (32,16)   just below it; even k (a k-mer can be its own reverse complement), generic w
  (5,5)     the table holds nearly every possible key, most anchor words are REPEAT, locate walks bits for every read
  (31,1)    w = 1 specialised: every position is a minimizer
  (21,129)  l = 149: the window ring is 66,048 B of dynamic LDS, the builder's seam is 148 bits across five words"""
import os
import sys
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import _depth_worker as DW  # noqa: E402
import _index_builder_worker as BW  # noqa: E402
from _depth_track_worker import Model as TrackModel  # noqa: E402
from _place_split_worker import place_split_all  # noqa: E402
from _place_worker import AnchorModel  # noqa: E402
from _place_worker import occurrences as positions_of  # noqa: E402
from conftest import random_reads, revcomp  # noqa: E402

GEOMETRIES = [(31, 15), (41, 15), (56, 2), (33, 15), (32, 16), (5, 5), (31, 1), (21, 129)]
MORE_GEOMETRIES = [(15, 11), (13, 7), (27, 19), (31, 65)]  # the differential test draws from both lists
TIGHT = [(56, 2), (21, 129), (32, 16)]  # run a second time with small tiles, a loaded table and the workgroup vote
TIGHT_ENV = {"DCN_TILE_WINDOWS": "16", "DCN_TABLE_SLOTS_PER_KEY": "2", "DCN_PLACE_LANE_BASES": "64", "DCN_PLACE_LDS_CELLS": "16"}
SEED = 1301
_worlds, _members, _builder_worlds = {}, {}, {}


def kw_id(kw):
    return "k%dw%d" % tuple(kw)


def self_complement(rng, k, w, O):
    """(record, read, position in the read): s + revcomp(s) with |s| = k/2 in the middle of a random record of which the
    read is a cut; the flanks are drawn again until the oracle reports the k-mer's position in the read, which makes it a
    minimizer of a window that lies in both"""
    assert k % 2 == 0
    flank = w + 40
    for _ in range(4000):
        s = random_reads(rng, 1, k // 2, k // 2)[0]
        kmer = s + revcomp(s)
        assert revcomp(kmer) == kmer
        left, right = random_reads(rng, 2, 200, 200)
        record = left + kmer + right
        read = record[200 - flank:200 + k + flank]
        if any(q == flank for _, q in positions_of(O, read, k, w)) and any(q == 200 for _, q in positions_of(O, record, k, w)):
            return record, read, flank
    raise AssertionError("no self-complementary minimizer found")


def read_ending_in_a_hit(O, genome, k, w, keys):
    """a cut of the genome whose last k-mer is a minimizer position with a key of `keys`: as the last read of a batch its
    k-mer ends exactly where the batch ends"""
    ln = k + w - 1 + 40
    for at in range(3000, len(genome) - ln):
        read = genome[at:at + ln]
        occ = positions_of(O, read, k, w)
        if occ and occ[-1][1] == ln - k and occ[-1][0] in keys:
            return read
    raise AssertionError("no read ends in a hit")


def members_of(O, k, w, extra=()):
    """(genomes, oracle indexes of the three members, their key sets, the sorted union); `extra` sequences join member 2"""
    key = (k, w, tuple(extra))
    if key not in _members:
        genomes = DW.make_genomes()
        seqs = DW.member_seqs(genomes)
        seqs[2] = seqs[2] + list(extra)
        ol = [O.Index.build(s, k=k, w=w) for s in seqs]
        _members[key] = (genomes, ol, [set(o.keys().tolist()) for o in ol], np.unique(np.concatenate([o.keys() for o in ol])))
    return _members[key]


def make_batch(O, rng, genomes, k, w, union_set, palindrome_read=None, n=140):
    """about 150 reads: DW.sample plus the fixed edge reads; -> (reads, {name: index of the edge read})"""
    l = k + w - 1
    reads = DW.sample(rng, genomes, n, k, 400)
    at = {}

    def put(name, r):
        at[name] = len(reads)
        reads.append(r)
    for i, ln in enumerate((k - 1, k, l - 1, l, l + 1)):  # below k, one k-mer, below one window, one window, two
        s = 900 + 37 * i
        put("len%d" % i, genomes[i % 3][s:s + ln])
    s = int(rng.integers(0, 15_000))
    put("long", genomes[int(rng.integers(0, 3))][s:s + 3000])  # several tiles at 256 windows a tile; the workgroup paths
    put("nn", genomes[2][s:s + 160] + b"NN" + genomes[2][s + 162:s + 400])
    put("lower", genomes[0][s + 50:s + 350].lower())
    put("empty", b"")
    t = int(rng.integers(0, 15_000))
    put("chimera", genomes[0][s:s + 1200] + revcomp(genomes[2][t:t + 1200]))  # two placements, on two strands
    if palindrome_read is not None:
        put("palindrome", palindrome_read)
    put("last", read_ending_in_a_hit(O, genomes[1], k, w, union_set))  # (stays the last read of the batch)
    return reads, at


def world(O, k, w, seed=SEED):
    """everything the sweep asserts at one geometry, in the order its calls are made"""
    key = (k, w, seed)
    if key in _worlds:
        return _worlds[key]
    from test_gpu_locate import model_batch, plain_label, set_label
    rng = np.random.default_rng(seed + 1000 * k + w)
    pal = self_complement(rng, k, w, O) if k % 2 == 0 else None
    genomes, ol, mkeys, union_keys = members_of(O, k, w, extra=[pal[0]] if pal else [])
    union_set = set(union_keys.tolist())
    reads, at = make_batch(O, rng, genomes, k, w, union_set, pal[1] if pal else None)
    b, o = O.concat_reads(reads)
    assert int(o[-1]) == len(b) and reads[-1] == reads[at["last"]]
    gap = 2 * w - 1
    union = O.Index(union_keys, k, w)
    flt = lambda idx: O.filter_batch(idx, b, o, None, abs_threshold=2, rel_threshold=0.01, deplete=False, threads=4)
    keep, hits, total = flt(union)
    occ = DW.occurrences(O, reads, k, w)
    adds = [list(genomes[:2]), list(genomes[2:]) + ([pal[0]] if pal else [])]
    a1 = AnchorModel(O, k, w, union_keys).add(adds[0])
    a2 = AnchorModel(O, k, w, union_keys).add(adds[0]).add(adds[1])
    wd = {
        "k": k, "w": w, "gap": gap, "genomes": genomes, "ol": ol, "mkeys": mkeys, "union_keys": union_keys,
        "reads": reads, "at": at, "b": b, "o": o, "palindrome": pal, "adds": adds,
        "filter": (keep.tolist(), hits.tolist(), total.tolist()),
        "classify": [flt(oj) for oj in ol],
        "occurrences": occ,
        "locate_plain": model_batch(O, reads, k, w, plain_label(ol[0]), 0, gap, 1),
        "locate_set": model_batch(O, reads, k, w, set_label(ol), 0, gap, 1),
        "locate_masked": model_batch(O, reads, k, w, set_label(ol), 0, gap, 2, member_mask=0b101),
        "track_before": TrackModel(O, reads, k, w, mkeys, Counter()).bins(100, 7),  # before any classify call: depth 0
        "track_after": TrackModel(O, reads, k, w, mkeys, occ).bins(0, 7),
        "track_after_100": TrackModel(O, reads, k, w, mkeys, occ).bins(100, 7),
        "anchors": [a1, a2],
        "place": [a1.place_all(reads), a2.place_all(reads)],
        "split": place_split_all(a2, reads, max_placements=4),
    }
    _worlds[key] = wd
    return wd


# ---- the index builder's sequences ---------------------------------------------------------------------------------
def builder_sequences(k, w):
    """the genomes, the messy sequences of tests/test_gpu_index_builder.py (IUPAC, N runs, lower case, a low-complexity
    tail) and ramps from a run of one base into random sequence: along a ramp the entropy of the k-mers rises through the
    floor, and a k-mer longer than 32 bases has a low-entropy head with a tail that lifts it"""
    from test_gpu_index_builder import messy_sequences
    rng = np.random.default_rng(1400 + k)
    ramps = []
    for c in b"ACGT":
        for _ in range(8):
            ramps.append(bytes([c]) * 60 + random_reads(rng, 1, 120, 120)[0])
            ramps.append(random_reads(rng, 1, 120, 120)[0] + bytes([c]) * 60)
    return list(DW.make_genomes()) + messy_sequences(k, w) + ramps


def occurrences_head_entropy(O, seqs, k, w, thr, head):
    """BW.occurrences with the entropy taken over the first `head` bases of each k-mer only: what a builder that cut the
    k-mer at 32 bases would count (used to show that the case can tell)"""
    c = Counter()
    thr = np.float32(thr)
    for s in seqs:
        s = bytes(s)
        pos = BW.positions_of(O, s, k, w)
        if not len(pos):
            continue
        h, p = O.minimizer_hashes_and_positions(BW.canonicalise(O, s), k, w)
        hash_at = dict(zip(p.tolist(), h.tolist()))
        for q in pos.tolist():
            kmer = s[q:q + k]
            if BW.ACGT.issuperset(kmer) and np.float32(O.scaled_entropy(kmer[:head], min(k, head))) >= thr:
                c[hash_at[q]] += 1
    return c


def builder_world(O, k, w):
    key = (k, w)
    if key not in _builder_worlds:
        seqs = builder_sequences(k, w)
        _builder_worlds[key] = {
            "seqs": seqs, "models": {thr: BW.occurrences(O, seqs, k, w, thr) for thr in (0.0, 0.5)},
            "shared": sum(BW.pieces_share_a_position(O, s, k, w, 4096) for s in seqs if len(s) > 4096),
        }
    return _builder_worlds[key]


# ---- what the CPU-only test asserts, so that a later change of seed cannot hollow the sweep out ---------------------
def assert_not_vacuous(O, k, w):
    wd = world(O, k, w)
    reads, at = wd["reads"], wd["at"]
    l = k + w - 1
    assert [len(reads[at["len%d" % i]]) for i in range(5)] == [k - 1, k, l - 1, l, l + 1]
    assert sum(1 for s in wd["locate_set"] if s) >= 50, "reads with a locate segment"
    members = set().union(*wd["mkeys"])
    assert sum(n for h, n in wd["occurrences"].items() if h in members) >= 200, "observed occurrences"
    info = wd["anchors"][1].info()
    if (k, w) == (5, 5):
        assert info["repeats"] > info["anchors"], info
    else:
        assert info["anchors"] >= 500, info
    assert any(len(r) > 8 * 256 for r in reads)
    # the last k-mer of the batch is a hit, of the filter and of locate
    last = reads[-1]
    assert wd["locate_set"][-1] and wd["locate_set"][-1][-1][1] == len(last)
    # the vote has something to decide, and the split has more than one row for some read
    if (k, w) == (5, 5):
        assert sum(p[3] for p in wd["place"][1]) > 0, "anchor hits"
    else:
        assert sum(1 for p in wd["place"][1] if p[0] != 0xFFFFFFFF) >= 25, "placed reads"
        off = wd["split"][0]
        assert off[at["chimera"] + 1] - off[at["chimera"]] >= 2, "the chimera's two placements"
    if k % 2 == 0:
        record, read, q = wd["palindrome"]
        a2 = wd["anchors"][1]
        hit = [h for h, p in positions_of(O, read, k, w) if p == q]
        assert hit and a2.state.get(hit[0]) == (len(wd["adds"][0]) + len(wd["adds"][1]) - 1, 200), "self-complement anchor"
        cells = a2.cells(read)[0]
        assert any((q, 200) in hits and o == 0 for (_, o, _), hits in cells.items())  # a hit, on the '+' strand
    bw = builder_world(O, k, w)
    m0, m5 = bw["models"][0.0], bw["models"][0.5]
    if w > 1:
        assert bw["shared"] >= 1, "no position is reported by two pieces of 4,096 bases"
    else:  # (two pieces share l - 1 = k - 1 bases: no k-mer lies in both)
        assert bw["shared"] == 0
    if k >= 10:  # (below 10 bases the scaled entropy is 1 by definition: nothing to drop)
        assert len(m5) < len(m0)
    else:
        assert m5 == m0
    if k > 32:  # a builder that took the entropy of 32 bases only would count otherwise
        assert occurrences_head_entropy(O, bw["seqs"], k, w, 0.5, 32) != m5
    return wd

"""Randomized differential test of the consumers of the minimizer dump, after tests/test_gpu_differential.py's run_seed:
per seed a geometry, tile and chunk sizes, a table load and the switches of the vote and of the builder's pieces are
drawn; then four cases each draw a batch (the four read-length styles, N / IUPAC / lower-case alphabets, low-complexity
repeats), a prefix length and the parameters of each consumer, and run a random non-empty subset of the consumers in
random order on ONE context against the models of the per-feature tests over the CPU oracle.  The set's depth counters
and the anchor map live through the seed's cases, so what one call leaves behind shows in the next.  Seeds are fixed;
every assert carries (seed, case, k, w, environment, parameters).  Integers only, compared exactly."""
import ctypes as C
import os
from collections import Counter

import numpy as np
import pytest

import _depth_worker as DW
import _geometry_cases as G
import _index_builder_worker as BW
from _depth_track_worker import Model as TrackModel
from _depth_track_worker import assert_track
from _place_split_worker import assert_split, place_split_all
from _place_worker import AnchorModel, assert_map, assert_placements
from conftest import mutate, random_reads, revcomp
from test_gpu_locate import assert_same, model_batch, plain_label, set_label

pytestmark = pytest.mark.gpu

KW = G.GEOMETRIES + G.MORE_GEOMETRIES
CONSUMERS = ("filter", "classify", "locate_plain", "locate_set", "track", "add", "place", "split", "builder")
MAX_BASES = 120_000  # of one batch: the models are Python


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def random_batch(rng, genomes, k, w):
    """the batch of test_gpu_differential.random_case, drawn from three genomes and capped at their length"""
    n = int(rng.integers(1, 150))
    style = int(rng.integers(0, 4))
    reads, total = [], 0
    for _ in range(n):
        if style == 0:
            ln = int(rng.integers(0, 320))
        elif style == 1:
            ln = int(rng.choice([k - 1, k, k + w - 2, k + w - 1, k + w, 150, 151, 250]))
        elif style == 2:
            ln = int(min(40_000, max(1, rng.lognormal(6.5, 1.2))))
        else:
            ln = int(rng.integers(100, 3000))
        genome = genomes[int(rng.integers(0, len(genomes)))]
        ln = min(ln, len(genome) - 1)
        r = rng.random()
        if r < 0.45 and ln > 0:
            s = int(rng.integers(0, len(genome) - ln))
            x = mutate(rng, genome[s:s + ln], float(rng.choice([0.0, 0.01, 0.1])))
            if rng.random() < 0.5:
                x = revcomp(x)
        elif r < 0.55 and ln > 0:
            unit = random_reads(rng, 1, 1, 12)[0]
            x = (unit * (ln // len(unit) + 1))[:ln]  # low complexity: ties, re-emitted positions
        else:
            x = random_reads(rng, 1, ln, ln, p_n=float(rng.choice([0.0, 0.001, 0.05])),
                             p_lower=float(rng.choice([0.0, 0.3])),
                             alphabet=b"ACGT" if rng.random() < 0.8 else b"ACGTNRYKMSWBDHV")[0]
        reads.append(x)
        total += len(x)
        if total > MAX_BASES:
            break
    return style, reads


def record_batches(rng, genomes):
    """what the seed's add calls add, in turn: two genomes, the third, then cuts of them (their keys become repeats) beside
    a record too short for a window and an empty one"""
    cuts = [genomes[i % 3][s:s + ln] for i, (s, ln) in enumerate(zip(rng.integers(0, 15_000, 4), rng.integers(200, 3000, 4)))]
    return [list(genomes[:2]), list(genomes[2:]), cuts[:2] + [b"ACGT", b""], [revcomp(cuts[2]), cuts[3].lower()]]


@pytest.mark.parametrize("seed", range(int(os.environ.get("DCN_FUZZ_SEEDS", "8"))))  # more seeds for a soak run
def test_consumers_differential(oracle, dcn, seed, monkeypatch):
    run_seed(oracle, dcn, seed, monkeypatch, 4)


def run_seed(O, dcn, seed, monkeypatch, n_cases):
    rng = np.random.default_rng(7000 + seed)
    k, w = KW[int(rng.integers(0, len(KW)))]
    env = {"DCN_TILE_WINDOWS": str(int(rng.choice([16, 64, 256, 2048]))),
           "DCN_CHUNK_BASES": [None, "1024", "5000"][int(rng.integers(0, 3))],
           "DCN_TABLE_SLOTS_PER_KEY": str(int(rng.choice([2, 4, 8]))),
           "DCN_PLACE_LANE_BASES": [None, "64"][int(rng.integers(0, 2))],
           "DCN_BUILD_CHUNK_BASES": [None, "4096"][int(rng.integers(0, 2))]}
    for name, value in env.items():
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    env = {name[4:]: value for name, value in env.items() if value is not None}
    genomes, ol, mkeys, union_keys = G.members_of(O, k, w)
    N = dcn._native
    lib = N.lib()
    gl = [dcn.Index.from_keys(x.keys(), k, w) for x in ol]
    s = dcn.IndexSet(gl)
    s.enable_depth()
    s.enable_coverage()
    map_index = dcn.Index.from_keys(union_keys, k, w)
    amap = dcn.AnchorMap(map_index)
    map_index.close()
    clf = dcn.Classifier(s, max_batch_bases=MAX_BASES + 50_000, max_batch_reads=1 << 9)
    ctx = clf._h
    builder_thr = float(rng.choice([0.0, 0.5]))
    builder = dcn.IndexBuilder(k, w, entropy_threshold=builder_thr)
    depth, anchors, built = Counter(), AnchorModel(O, k, w, union_keys), Counter()
    to_add = record_batches(rng, genomes)
    labels = {"locate_plain": plain_label(ol[0]), "locate_set": set_label(ol)}
    try:
        for case in range(n_cases):
            style, reads = random_batch(rng, genomes, k, w)
            b, o = O.concat_reads(reads)
            n = len(reads)
            prefix = int(rng.choice([0, 60, 5000]))
            names = [c for c in CONSUMERS if rng.random() < 0.6] or [CONSUMERS[int(rng.integers(0, len(CONSUMERS)))]]
            names = [names[i] for i in rng.permutation(len(names))]
            what = ("seed", seed, "case", case, "k", k, "w", w, env, "style", style, "reads", n, "prefix", prefix, names)
            pb = ptr(b) if len(b) else None

            def run_filter():
                prm = N.Params(int(rng.choice([1, 2, 3, 10])), float(rng.choice([0.0, 0.01, 0.2, 1.0])), prefix, int(rng.integers(0, 2)), 0)
                par = ("filter", prm.abs_threshold, prm.rel_threshold, prm.deplete)
                union = O.Index(union_keys, k, w)
                want = O.filter_batch(union, b, o, None, abs_threshold=prm.abs_threshold, rel_threshold=prm.rel_threshold,
                                      prefix_length=prefix, deplete=bool(prm.deplete), threads=4)
                keep, hits, total = np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
                N.check(lib.dcn_filter_batch(ctx, pb, ptr(o), None, n, C.byref(prm), ptr(keep), ptr(hits), ptr(total)))
                assert total.tolist() == want[2].tolist(), what + par + ("total",)
                assert hits.tolist() == want[1].tolist(), what + par + ("hits",)
                assert keep.astype(bool).tolist() == want[0].tolist(), what + par + ("keep",)

            def run_classify():
                clf.abs_threshold, clf.rel_threshold = int(rng.choice([1, 2, 3])), float(rng.choice([0.0, 0.01, 0.2]))
                clf.prefix_length = prefix
                par = ("classify", clf.abs_threshold, clf.rel_threshold)
                match, hits, total = clf.classify_batch(b, o)
                for j, oj in enumerate(ol):
                    keep, h, t = O.filter_batch(oj, b, o, None, abs_threshold=clf.abs_threshold, rel_threshold=clf.rel_threshold,
                                                prefix_length=prefix, deplete=False, threads=4)
                    assert total.tolist() == t.tolist() and hits[:, j].tolist() == h.tolist(), what + par + ("member", j)
                    assert ((match >> j) & 1).astype(bool).tolist() == keep.tolist(), what + par + ("match", j)
                depth.update(DW.occurrences(O, reads, k, w, prefix))
                try:
                    DW.assert_depths(s, depth, mkeys, bins=(256,))
                except AssertionError as e:
                    raise AssertionError(what + par + tuple(e.args)) from e
                for j in (None, 0, 1, 2):
                    assert set(s.observed_keys(j).tolist()) == set(DW.expected(depth, mkeys, j)), what + par + ("observed", j)

            def run_locate(name):
                max_gap = int(rng.choice([0, w, 2 * w - 1, 1000]))
                min_hits = int(rng.choice([1, 2, 5]))
                mask = int(rng.integers(1, 8)) if name == "locate_set" else 0xFFFFFFFF
                par = (name, "max_gap", max_gap, "min_hits", min_hits, "mask", mask)
                want = model_batch(O, reads, k, w, labels[name], prefix, max_gap, min_hits, member_mask=mask)
                prm = N.LocateParams(max_gap, min_hits, mask, 0, prefix)
                so = np.zeros(n + 1, np.uint64)
                segs = np.zeros(sum(len(x) for x in want) + 1, dcn.filter.SEGMENT_DTYPE)
                index = gl[0] if name == "locate_plain" else s
                N.check(lib.dcn_locate_batch(ctx, index._h, pb, ptr(o), n, C.byref(prm), ptr(so), ptr(segs), len(segs)))
                got = [[tuple(int(x) for x in q) for q in segs[int(so[r]):int(so[r + 1])]] for r in range(n)]
                try:
                    assert_same(got, want)
                except AssertionError as e:
                    raise AssertionError(what + par + tuple(e.args)) from e

            def run_track():
                bin_bases = int(rng.choice([0, 1, 32, 33, 100, 1000]))
                mask, cap = int(rng.integers(1, 8)), int(rng.choice([0, 1, 255]))
                par = ("track", "bin_bases", bin_bases, "mask", mask, "cap", cap)
                want = TrackModel(O, reads, k, w, mkeys, depth, prefix).bins(bin_bases, mask, cap)
                prm = N.TrackParams(bin_bases, mask, cap, 0, prefix)
                bo = np.zeros(n + 1, np.uint64)
                bins = np.zeros(max(int(want[0][-1]), 1), dcn.filter.TRACK_BIN_DTYPE)
                N.check(lib.dcn_depth_track_batch(ctx, s._h, pb, ptr(o), n, C.byref(prm), ptr(bo), ptr(bins), int(want[0][-1])))
                assert_track((bo, bins[:int(want[0][-1])]), want, what + par)

            def run_add():
                if not to_add:
                    return
                records = to_add.pop(0)
                rb, ro = O.concat_reads(records)
                first = C.c_uint32()
                N.check(lib.dcn_anchor_map_add(amap._h, ctx, ptr(rb), ptr(ro), len(records), C.byref(first)))
                assert first.value == len(anchors.records), what + ("add",)
                anchors.add(records)
                assert_map(amap, anchors, what + ("add", len(anchors.records)))

            def run_place():
                band, min_votes = int(rng.choice([1, 64, 256])), int(rng.choice([1, 2, 5]))
                par = ("place", "band", band, "min_votes", min_votes, "records", len(anchors.records))
                prm = N.PlaceParams(band, min_votes, prefix, (C.c_uint32 * 2)(0, 0))
                out = np.zeros(max(n, 1), dcn.filter.PLACEMENT_DTYPE)
                N.check(lib.dcn_place_batch(ctx, amap._h, pb, ptr(o), n, C.byref(prm), ptr(out)))
                assert_placements(out[:n], anchors.place_all(reads, W=band, min_votes=min_votes, prefix=prefix), what + par)

            def run_split():
                band, min_votes = int(rng.choice([1, 64, 256])), int(rng.choice([1, 2, 5]))
                most = int(rng.choice([1, 4, 8]))
                par = ("split", "band", band, "min_votes", min_votes, "max_placements", most, "records", len(anchors.records))
                prm = N.PlaceSplitParams(band, min_votes, prefix, most, (C.c_uint32 * 3)(0, 0, 0))
                po = np.zeros(n + 1, np.uint64)
                rows = np.zeros(max(n * most, 1), dcn.filter.SPLIT_PLACEMENT_DTYPE)
                counts = np.zeros((max(n, 1), 2), np.uint32)
                N.check(lib.dcn_place_split_batch(ctx, amap._h, pb, ptr(o), n, C.byref(prm), ptr(po), ptr(rows), n * most, ptr(counts)))
                want = place_split_all(anchors, reads, W=band, min_votes=min_votes, prefix=prefix, max_placements=most)
                assert_split((po, rows[:int(po[n])], counts[:n]), want, what + par)

            def run_builder():
                built.update(BW.occurrences(O, reads, k, w, builder_thr))
                builder.add(reads)
                try:
                    BW.assert_counts(builder, built, bins=(3, 256))
                except AssertionError as e:
                    raise AssertionError(what + ("builder", builder_thr) + tuple(e.args)) from e
                idx = builder.finish(2, 0)
                assert sorted(idx.keys().tolist()) == BW.selected(built, 2, 0), what + ("builder", builder_thr, "finish")
                idx.close()

            calls = {"filter": run_filter, "classify": run_classify, "track": run_track, "add": run_add, "place": run_place,
                     "split": run_split, "builder": run_builder,
                     "locate_plain": lambda: run_locate("locate_plain"), "locate_set": lambda: run_locate("locate_set")}
            for name in names:
                calls[name]()
    finally:
        builder.close()
        clf.close()
        amap.close()
        s.close()
        for g in gl:
            g.close()

"""The second and third trip of every capped-grid kernel's work loop.  Most kernels behind the row calls, the vote, classify
and locate launch a grid capped at a multiple of the device's CU count and stride over the rest of their work, many of them
with state carried from one item to the next in LDS or registers; every other test calls them with fewer items than one
trip takes.  Here DCN_GRID_CUS = 1 (a test hook read at call time by dcn_cu_count, ctx.hip) shrinks the grids so that a few
hundred items loop, and one call of 256 * C + 517 rows loops the row kernels at the full grid without the hook.

The inputs and what they must contain are tests/_grid_trip_cases.py's, held to it without a GPU by
tests/test_grid_trip_cases.py.  Expected values are the existing models'; every comparison is exact.  The existing seam
cases are called as functions of their modules, with the modules' own fixtures; nothing is collected twice."""
import time

import numpy as np
import pytest

import _align_worker as AW
import _grid_trip_cases as G
import _insertion_worker as IW
import _pileup_worker as PW
import _place_pair_worker as PPW
import _place_split_worker as PSW
import _place_worker as PLW
import _verify_worker as VW
import test_gpu_classify_coverage as CC
import test_gpu_depth as TD
import test_gpu_depth_track_seams as TT
import test_gpu_index_builder as TB
import test_gpu_locate_seams as TL
import test_gpu_set_algebra as TS
from test_gpu_align_seams import env as align_env  # noqa: F401
from test_gpu_classify import check as classify_check
from test_gpu_classify_coverage import genomes, members31  # noqa: F401  (members31 asks for genomes by that name)
from test_gpu_depth_track_seams import edges_plan, g31  # noqa: F401
from test_gpu_extend_seams import env as extend_env  # noqa: F401
from test_gpu_index_builder import reads_case  # noqa: F401
from test_gpu_insertions_seams import env as insertions_env  # noqa: F401
from test_gpu_pileup_seams import env as pileup_env  # noqa: F401
from test_gpu_verify_seams import env as verify_env  # noqa: F401

pytestmark = pytest.mark.gpu

H = G.HOOK_CUS
SWEEP_ITEMS = G.sweep_blocks(H) * G.SWEEP_THREADS  # what a thread-strided sweep takes in one trip under the hook
SWEEP_SLOTS = 4 * SWEEP_ITEMS                      # ... in slots, where a thread takes four of them (the label quads)


@pytest.fixture
def one_cu(monkeypatch):
    monkeypatch.setenv("DCN_GRID_CUS", str(H))


# ---- the existing seam cases of the row calls ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.SEAM_CASES, ids=G.seam_id)
def test_seam_case_under_the_hook(case, one_cu, verify_env, align_env, extend_env, pileup_env, insertions_env):
    env = {"test_gpu_verify_seams": verify_env, "test_gpu_align_seams": align_env, "test_gpu_extend_seams": extend_env,
           "test_gpu_pileup_seams": pileup_env, "test_gpu_insertions_seams": insertions_env}[case[0]]
    counting = G.run_seam_case(case, env, env[4])
    for name in case[3]:
        G.assert_looped(counting, name)


# ---- the map chain ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain_map(dcn, oracle):
    records = G.chain_records()
    amap = VW.build_map(oracle, dcn, records)
    amap.pileup_enable()
    amap.pileup_keep_insertions()
    yield records, amap
    amap.close()


def assert_extension(got_rows, got, want_rows, want):
    for name in want.dtype.names:
        bad = np.flatnonzero(got[name] != want[name])
        assert len(bad) == 0, ("extension", name, [(int(t), int(got[name][t]), int(want[name][t])) for t in bad[:5]])
    for name in IW.ROW.names:
        assert np.array_equal(got_rows[name], want_rows[name]), ("extended rows", name)


def assert_runs(got, edits, offs, cigar):
    """(edits, cigar_offsets, cigar) of align_batch against the model's three arrays, the first row that differs named"""
    ge, go, gc = got
    bad = np.flatnonzero(np.asarray(ge) != edits)
    assert len(bad) == 0, ("edits", [(int(i), int(ge[i]), int(edits[i])) for i in bad[:5]])
    bad = np.flatnonzero(np.diff(np.asarray(go).astype(np.int64)) != np.diff(offs.astype(np.int64)))
    assert len(bad) == 0 and len(go) == len(offs), ("run counts", [int(i) for i in bad[:5]])
    bad = np.flatnonzero(np.asarray(gc) != cigar)
    assert len(bad) == 0, ("runs", [(int(np.searchsorted(offs, i, "right")) - 1, AW.cigar_text(gc[i:i + 1]), AW.cigar_text(cigar[i:i + 1]))
                                    for i in bad[:5]])


def test_map_chain_under_the_hook(dcn, oracle, chain_map, one_cu, monkeypatch):
    """600 hand-written rows through extend, verify, align and pileup with the ledger: three trips and more of every wave, a
    d = 0 row behind a large d, rows that add nothing between adding ones, one run behind 130, no I run behind twelve; the row
    of (1=1I) x 150: 150 events in one fetch and 150 alleles in one call; the whole record in one call: a second chunk of 64
    positions for the waves of the winner pass"""
    records, amap = chain_map
    monkeypatch.delenv("DCN_ALIGN_TRACE_BYTES", raising=False)  # the default budget: one trace group (G.trace_bytes)
    _, reads, rows, _ = G.chain_inputs()
    M = G.chain_model()
    placer = dcn.Placer(amap, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    try:
        b, o = oracle.concat_reads(reads)
        rows = IW.rows_as(dcn.filter.PLACEMENT_DTYPE, rows)
        got_rows, got = placer.extend_batch(b, o, rows, max_edits=G.CHAIN_KW["max_edits"])
        assert_extension(got_rows, got, M["ext_rows"], M["ext"])
        bad = np.flatnonzero(placer.verify_batch(b, o, got_rows, **G.CHAIN_KW) != M["edits"])
        assert len(bad) == 0, ("verify", [(int(i), int(M["edits"][i])) for i in bad[:5]])
        assert_runs(placer.align_batch(b, o, got_rows, **G.CHAIN_KW), M["edits"], M["offs"], M["cigar"])
        amap.pileup_reset()
        edits, n_added = placer.pileup_batch(b, o, got_rows, **G.CHAIN_KW)
        assert edits.tolist() == M["edits"].tolist() and n_added == M["n_added"]
        PW.assert_counts(amap, records, M["counts"])
        IW.assert_ledger(amap, records, M["counts"], M["ledger"], settings=((3, 500), (1, 0)))
        ev, bases = amap.insertions_fetch(0, G.N_AT, G.N_BASES)
        IW.assert_dense(ev, bases)
        assert IW.events_as_tuples(ev, bases) == IW.fetch_range(M["ledger"][0], G.N_AT, G.N_BASES) and len(ev) == G.N_BASES
        al, bases = amap.insertions_call(0, G.N_AT, G.N_BASES, min_depth=1, min_permille=0)
        IW.assert_dense(al, bases)
        assert IW.alleles_as_tuples(al, bases) == IW.call_range(M["counts"][0], M["ledger"][0], records[0], G.N_AT, G.N_BASES, 1, 0)
        assert len(al) == G.N_BASES and bases == b"N" * G.N_BASES
        for R in (0, 1):
            PW.assert_calls(amap, records, M["counts"], R, min_depth=1, min_permille=0)
    finally:
        placer.close()


# ---- one call at the full grid, without the hook -------------------------------------------------------------------------
def test_full_grid_without_the_hook(dcn, oracle, chain_map, monkeypatch):
    """n = 256 * C + 517 rows (66,053 on an MI355X), a seeded draw from 200 unique (read, row) pairs, one row per read:
    extend, verify, align and pileup with the ledger loop at the grids production runs with.  The models run on the unique
    pairs; edits, extents and runs are gathered through the draw, counters weighted by it, events repeated."""
    import torch
    monkeypatch.delenv("DCN_GRID_CUS", raising=False)
    monkeypatch.delenv("DCN_ALIGN_TRACE_BYTES", raising=False)  # the default budget: one trace group (G.trace_bytes)
    C = torch.cuda.get_device_properties(0).multi_processor_count
    n = G.full_rows(G.FULL_CUS)
    assert n > 256 * C, "a device with more CUs: the call no longer exceeds extend's cap (raise FULL_CUS)"
    records, amap = chain_map
    t0 = time.perf_counter()
    _, reads_u, rows_u = G.full_unique()
    M = G.full_model(G.FULL_CUS)
    draw = M["draw"]
    b, o = oracle.concat_reads([reads_u[u] for u in draw])
    rows = IW.rows_as(dcn.filter.PLACEMENT_DTYPE, rows_u)[draw]
    t1 = time.perf_counter()
    placer = dcn.Placer(amap, max_batch_bases=1 << 24, max_batch_reads=1 << 17)
    try:
        got_rows, got = placer.extend_batch(b, o, rows)
        assert_extension(got_rows, got, M["ext_rows"], M["ext"])
        assert np.array_equal(placer.verify_batch(b, o, got_rows), M["edits"])
        assert_runs(placer.align_batch(b, o, got_rows), M["edits"], M["offs"], M["cigar"])
        amap.pileup_reset()
        edits, n_added = placer.pileup_batch(b, o, got_rows)
        assert np.array_equal(edits, M["edits"]) and n_added == M["n_added"] > 2 * G.wave4_items(C)
        t2 = time.perf_counter()
        PW.assert_counts(amap, records, M["counts"])
        IW.assert_ledger(amap, records, M["counts"], M["ledger"], settings=((3, 500),))
    finally:
        placer.close()
    print("full grid: %d rows; inputs and models %.2f s, the four calls %.2f s, fetch, call and consensus against the models %.2f s"
          % (n, t1 - t0, t2 - t1, time.perf_counter() - t2))


# ---- place, split and pairs --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def place_map(dcn, oracle):
    records, _, reads = G.place_case()
    model, amap = PLW.build_map(oracle, dcn, records, 31, 1)
    yield records, model, amap, reads
    amap.close()


@pytest.mark.parametrize("cells", [None, G.PLACE_CELLS], ids=["default-set", "16-cells"])
def test_place_workgroups_take_ten_reads_each(dcn, oracle, place_map, one_cu, monkeypatch, cells):
    """48 reads, all listed (DCN_PLACE_LANE_BASES = 0), four workgroups: a read stitched from scattered cuts in front of a clean
    one on every workgroup, with the default LDS set and with 16 cells (partitions)"""
    records, model, amap, reads = place_map
    monkeypatch.setenv("DCN_PLACE_LANE_BASES", "0")
    if cells:
        monkeypatch.setenv("DCN_PLACE_LDS_CELLS", str(cells))
    PLW.assert_map(amap, model, ("grid trips",))  # (the sweep over the table's slots, which loops as well)
    assert amap.table_bytes // 8 > SWEEP_SLOTS
    for W in (1, 64):
        PLW.assert_placements(PLW.place(dcn, amap, reads, oracle, band_bases=W), model.place_all(reads, W=W), ("grid trips", W, cells))
        for n in (2, 8):
            PSW.check_split(dcn, oracle, model, amap, reads, ("grid trips", cells), max_placements=n, band_bases=W)
        PPW.check_pairs(dcn, oracle, model, amap, reads, ("grid trips", cells), max_placements=4, band_bases=W)


@pytest.mark.parametrize("case,env", [(PLW.case_partitions, {"DCN_PLACE_LDS_CELLS": "16", "DCN_PLACE_LANE_BASES": "0"}),
                                      (PSW.case_partitions, {"DCN_PLACE_LDS_CELLS": "16", "DCN_PLACE_LANE_BASES": "0"}),
                                      (PPW.case_partitions, {"DCN_PLACE_LDS_CELLS": "16", "DCN_PLACE_LANE_BASES": "200"}),
                                      (PLW.case_switch, {"DCN_PLACE_LANE_BASES": "100"})],
                         ids=["place-partitions", "split-partitions", "pair-partitions", "place-switch"])
def test_place_seam_case_under_the_hook(dcn, oracle, one_cu, monkeypatch, case, env):
    """the partition and path-switch cases of place, split and pairs in this process; every call of theirs is seen on its way
    to the Placer, and the largest lists more reads (those longer than DCN_PLACE_LANE_BASES) than four workgroups take at once"""
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    lane, listed = int(env["DCN_PLACE_LANE_BASES"]), []

    def seen(module, name, reads_at):
        f = getattr(module, name)

        def call(*args, **kw):
            listed.append(sum(len(r) > lane for r in args[reads_at]))
            return f(*args, **kw)
        monkeypatch.setattr(module, name, call)
    seen(PLW, "place", 2)        # place(dcn, amap, reads, O, ..)
    seen(PSW, "split", 2)        # split(dcn, amap, reads, O, ..)
    seen(PPW, "check_pairs", 4)  # check_pairs(dcn, O, model, amap, reads, ..)
    case(oracle, dcn)
    G.assert_listed(max(listed))


# ---- classify ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coverage", [False, True], ids=["plain", "coverage"])
def test_classify_workgroups_take_eleven_units_each(dcn, oracle, one_cu, coverage):
    """45 units of the workgroup kernel on four workgroups: units of three hash partitions in front of units that just pass
    the lane kernel's entry limit or its hit limit"""
    U = G.classify_case()
    reads, uid = U.batch()
    pairs = U.index_pairs(oracle, dcn, 31, np.random.default_rng(1932))
    s = dcn.IndexSet([g for _, g in pairs])
    if coverage:
        s.enable_coverage()
    try:
        for abs_t, rel_t in ((2, 0.01), (1, 0.5)):
            clf = dcn.Classifier(s, abs_threshold=abs_t, rel_threshold=rel_t, max_batch_bases=1 << 22, max_batch_reads=1 << 17)
            match, hits, total = classify_check(oracle, clf, [o for o, _ in pairs], reads, uid)
            want = U.expected(abs_t, rel_t)
            assert total.tolist() == want[2].tolist() and hits.tolist() == want[1].tolist() and match.tolist() == want[0].tolist()
            clf.close()
        if coverage:
            seen = {h for es in U.units for _, h in es if h is not None}
            for j, m in enumerate(U.members):
                assert set(s.observed_keys(j).tolist()) == seen & m, ("observed", j)
    finally:
        s.close()
        for _, g in pairs:
            g.close()


# ---- locate --------------------------------------------------------------------------------------------------------------------
def test_locate_waves_take_four_reads_each(dcn, oracle, one_cu):
    """120 reads of the wave kernel on 32 waves: a read whose last segment is open at its end in front of a read with no hit
    in its first 64 words"""
    plan = G.locate_plan()
    g = TL.Genome(oracle, TL.K, sum(ln for ln, _ in plan) + 64, 1941)
    assert g.distinct
    b = TL.Batch(oracle, g)
    for i, (ln, hits) in enumerate(plan):
        if i % 4 == 0:
            b.pad((1, 31, 0)[(i // 4) % 3])
        b.add(ln, hits)
    for max_gap, min_hits in ((0, 1), (40, 2), (2000, 1)):
        got = b.check(dcn, max_gap, min_hits)
        assert sum(len(x) for x in got) >= len(plan)


# ---- the thread-strided sweeps ---------------------------------------------------------------------------------------------
def test_set_algebra_sweeps_loop(dcn, one_cu):
    s, _ = TS.check_set(dcn, TS.plan3())
    assert s.memory // 12 > SWEEP_SLOTS
    TS.test_three_members_with_planned_overlaps(dcn)


def test_depth_sweeps_loop(dcn, oracle, one_cu):
    # (what tests/test_gpu_depth.py's fixtures genomes, members, batch and batch_model are: its `genomes` shares its name
    # with the coverage case's, so they are made here)
    genomes20 = TD.W.make_genomes()
    members = TD.W.build_members(oracle, dcn, genomes20, TD.K, TD.WIN)
    batch = TD.W.mixed_batch(genomes20)
    try:
        s = TD.new_set(dcn, members)
        assert s.memory // 12 > SWEEP_SLOTS
        s.close()
        TD.test_mixed_batch_is_exact(oracle, dcn, members, batch, TD.occurrences(oracle, batch, TD.K, TD.WIN))
    finally:
        for g in members[1]:
            g.close()


def test_builder_sweeps_loop(dcn, oracle, one_cu, reads_case):
    k, w = TB.KW[1]
    assert len(reads_case[1][(k, w)]) > SWEEP_ITEMS  # distinct keys counted, and the table has more slots than keys
    assert sum(len(r) for r in reads_case[0]) > SWEEP_ITEMS  # (the count kernel strides over bases)
    TB.test_reads_in_three_calls_and_finish_by_count(oracle, dcn, reads_case, k, w)


def test_coverage_count_loops(dcn, oracle, one_cu, genomes, members31):
    """coverage_count_kernel<true> strides over slots, <false> (the observed counts) and coverage_keys_kernel over bitmap
    words of 32 slots: the case's set has more than 2,048 of either"""
    s = dcn.IndexSet([g for _, g in members31])
    slots = s.memory // 12
    s.close()
    assert slots > SWEEP_ITEMS and slots // 32 > SWEEP_ITEMS, slots
    CC.test_marks_accumulate_reset_and_reenable(oracle, dcn, genomes, members31)


def test_track_pieces_loop(dcn, oracle, one_cu, edges_plan):
    p, _ = edges_plan
    bin_bases = TT.LANE_BASES + 1  # every read longer than the lane path's limit: a piece per bin, 8 x 4 waves under the hook
    assert sum(-(-len(r) // bin_bases) for r in p.reads if len(r) > TT.LANE_BASES) > G.sweep_blocks(H) * 4
    TT.test_bin_edges_and_the_path_switch(oracle, dcn, edges_plan, bin_bases)
    TT.test_many_reads_and_bins(oracle, dcn, edges_plan, 2049)

"""CPU: the cases of tests/test_gpu_grid_trips.py are not vacuous, by the models alone.  For every case: (a) its items exceed the
cap of the kernel's grid at the CU count the case runs under (1 under DCN_GRID_CUS, 256 at the full grid); (b) at that grid's
stride there are items r and r + stride of different shapes; (c) the item after a stateful one is a kind that would show a
leak.  The work lists of align, pileup and the insertion walk are the aligned rows in row order (align_api.hip); those of
place, classify and locate are written with atomics and taken here in read order (see tests/_grid_trip_cases.py)."""
import numpy as np
import pytest

import _grid_trip_cases as G
import _insertion_worker as IW

OVER, UNPLACED = G.OVER, G.UNPLACED
H, F = G.HOOK_CUS, G.FULL_CUS


def test_the_caps_at_one_cu_and_on_an_mi355x():
    assert (G.wave_rows(H), G.extend_rows(H), G.wave4_items(H), G.winner_positions(H), G.list_items(H), G.locate_reads(H)) == \
        (128, 256, 128, 8192, 4, 32)
    assert (G.wave_rows(F), G.extend_rows(F), G.wave4_items(F), G.winner_positions(F), G.list_items(F), G.locate_reads(F)) == \
        (32_768, 65_536, 32_768, 2_097_152, 1_024, 8_192)
    assert G.sweep_blocks(H) * G.SWEEP_THREADS == 2048 and G.sweep_blocks(F) == 2048
    assert G.trips(128, 128) == 1 and G.trips(129, 128) == 2 and G.stride(100, 128) == 100 and G.stride(600, 128) == 128


def pairs(items, step):
    """(r, r + step) over a list of items"""
    return [(items[i], items[i + step]) for i in range(len(items) - step)]


@pytest.fixture(scope="module")
def chain():
    records, reads, rows, kinds = G.chain_inputs()
    return records, reads, rows, kinds, G.chain_model()


def test_chain_exceeds_every_cap_three_times(chain):
    records, reads, rows, kinds, M = chain
    assert len(rows) == len(reads) == G.CHAIN_ROWS and len(records[0]) == G.LEN0 and G.LEN0 % 16 != 0
    assert G.trips(len(rows), G.wave_rows(H)) >= 3          # verify
    assert G.trips(len(rows), G.extend_rows(H)) >= 3        # extend
    assert G.trips(len(M["work"]), G.wave4_items(H)) >= 3   # align, its gather, pileup, the insertion walk
    assert G.trace_bytes(M["edits"]) <= G.ALIGN_TRACE_BYTES  # ... align in ONE trace group at the default budget
    assert M["n_added"] > G.wave4_items(H) and (M["edits"] == OVER).sum() > 20 and (M["edits"] == UNPLACED).sum() > 20


def test_chain_rows_of_one_wave_differ_and_would_show_a_leak(chain):
    records, reads, rows, kinds, M = chain
    ext_rows, edits, offs, cigar = M["ext_rows"], M["edits"], M["offs"], M["cigar"]
    shape = [G.row_shape(ext_rows, edits, offs, cigar, r, **G.CHAIN_KW) for r in range(len(rows))]
    # verify: a wave takes rows r, r + 128, ...
    g = G.stride(len(rows), G.wave_rows(H))
    assert sum(a != b for a, b in pairs(shape, g)) > 300
    e = edits.tolist()
    assert sum(30 <= a < OVER and b == 0 for a, b in pairs(e, g)) >= 3           # d = 0 behind a large d
    assert sum(a == OVER and b == 0 for a, b in pairs(e, g)) >= 3                # ... and behind a row that ran to E = 160
    assert sum(a < OVER and b == UNPLACED for a, b in pairs(e, g)) >= 3 and sum(a == UNPLACED and b < OVER for a, b in pairs(e, g)) >= 3
    # align, pileup, the walk: a wave takes work items w, w + 128, ...
    work = M["work"].tolist()
    gw = G.stride(len(work), G.wave4_items(H))
    n_runs = [G.n_runs_of(offs, cigar, r) for r in work]
    i_runs = [G.i_runs_of(offs, cigar, r) for r in work]
    n_ref = [int(ext_rows["ref_end"][r]) - int(ext_rows["ref_start"][r]) for r in work]
    assert sum(shape[a] != shape[b] for a, b in pairs(work, gw)) > 200
    assert sum(a >= 10 and b == 0 for a, b in pairs(i_runs, gw)) >= 3            # no I run behind a row with many
    assert sum(a > 64 and b <= 3 for a, b in pairs(n_runs, gw)) >= 3             # few runs behind more than a chunk of 64
    assert sum(a > 128 and b == 1 for a, b in pairs(n_runs, gw)) >= 1            # one run behind three chunks
    # a row that adds nothing (n = 0) between two adding ones of one wave
    assert sum(n_ref[w] > 0 and n_ref[w + gw] == 0 and n_ref[w + 2 * gw] > 0 for w in range(len(work) - 2 * gw)) >= 2
    # extend: a wave takes the flanks of rows r .. r + 1, then of r + 256 ..
    gx = G.stride(len(rows), G.extend_rows(H))
    ext = M["ext"]
    busy = ((ext["left_edits"] + ext["right_edits"]) > 0).tolist()
    gained = ((ext["read_end"].astype(np.int64) - ext["read_start"]) - (rows["read_end"].astype(np.int64) - rows["read_start"])).tolist()
    assert sum(a and not b for a, b in pairs(busy, gx)) >= 3 and sum(a > 0 and b == 0 for a, b in pairs(gained, gx)) >= 10
    assert sum(kinds[r] != "unplaced" and kinds[r + gx] == "unplaced" for r in range(len(rows) - gx)) >= 3


def test_chain_ledger_makes_the_range_kernels_loop(chain):
    records, reads, rows, kinds, M = chain
    r = G.N_ROW
    assert kinds[r] == "n_behind_each" and int(M["edits"][r]) == G.N_BASES
    assert G.n_runs_of(M["offs"], M["cigar"], r) == 2 * G.N_BASES and G.i_runs_of(M["offs"], M["cigar"], r) == G.N_BASES
    from _align_worker import cigar_text
    assert cigar_text(M["cigar"][int(M["offs"][r]):int(M["offs"][r + 1])]) == "1=1I" * G.N_BASES
    # nothing else lies on its interval: 150 events in one fetch and 150 called alleles in one call, more than 128 waves
    events = IW.fetch_range(M["ledger"][0], G.N_AT, G.N_BASES)
    assert len(events) == G.N_BASES > G.wave4_items(H) and [e[0] for e in events] == list(range(G.N_AT, G.N_AT + G.N_BASES))
    alleles = IW.call_range(M["counts"][0], M["ledger"][0], records[0], G.N_AT, G.N_BASES, 1, 0)
    assert len(alleles) == G.N_BASES > G.wave4_items(H)
    # the whole record in one range: more chunks of 64 positions than waves, called insertions on both sides of the seam
    assert G.trips(G.LEN0, G.winner_positions(H)) == 2
    called = [a[0] for a in IW.call_range(M["counts"][0], M["ledger"][0], records[0], 0, None, 1, 0)]
    seam = G.winner_positions(H)
    assert sum(p < seam for p in called) > 100 and sum(p >= seam for p in called) > 100
    assert len(M["ledger"][0]) > 10 * G.wave4_items(H)


@pytest.fixture(scope="module")
def full():
    return G.full_unique(), G.full_model(F)


def test_full_grid_exceeds_the_caps_of_an_mi355x(full):
    (records, reads, rows), M = full
    n = G.full_rows(F)
    assert n == 66_053 == len(M["draw"]) and len(rows) == G.FULL_UNIQUE and M["weight"].min() >= 1
    assert n > G.extend_rows(F) and G.trips(n, G.wave_rows(F)) >= 3 and G.trips(len(M["work"]), G.wave4_items(F)) >= 3
    assert M["n_added"] > 2 * G.wave4_items(F)
    assert G.trace_bytes(M["edits"]) <= G.ALIGN_TRACE_BYTES  # one trace group: align_kernel's grid strides over every row
    edits, offs, cigar, ext_rows = M["unique"]
    assert sorted(set(edits.tolist())) == list(range(9))
    m = ext_rows["read_end"].astype(np.int64) - ext_rows["read_start"]
    assert m.min() >= 40 and set(ext_rows["reverse"].tolist()) == {0, 1} and set(ext_rows["record"].tolist()) == {0, 1}
    assert sum(G.i_runs_of(offs, cigar, u) > 0 for u in range(G.FULL_UNIQUE)) > 40
    # no position receives more than about a thousand events: the winner pass is quadratic in them
    for R in range(2):
        per = np.bincount(np.array([e[0] for e in M["ledger"][R]], np.int64))
        assert 300 < per.max() <= 1000
    # a fetch takes one record: record 0 alone has more events than ins_gather_kernel's waves take in one trip.  (The called
    # alleles of a range stay far below that: ins_alleles_kernel, like the winner pass, does not loop at the full grid.)
    assert max(len(x) for x in M["ledger"]) == len(M["ledger"][0]) > G.wave4_items(F)
    assert len(IW.call_range(M["counts"][0], M["ledger"][0], records[0])) < G.wave4_items(F)


def test_full_grid_rows_of_one_wave_differ(full):
    (records, reads, rows), M = full
    edits, offs, cigar, ext_rows = M["unique"]
    shape = [G.row_shape(ext_rows, edits, offs, cigar, u, **G.FULL_KW) for u in range(G.FULL_UNIQUE)]
    draw = M["draw"].tolist()
    for g in (G.wave_rows(F), G.extend_rows(F)):
        assert sum(shape[a] != shape[b] for a, b in pairs(draw, g)) > 400
    i_runs = [G.i_runs_of(offs, cigar, u) for u in range(G.FULL_UNIQUE)]
    e = edits.tolist()
    g = G.wave4_items(F)  # (every row is aligned: the work list is the rows)
    assert len(M["work"]) == len(draw)
    assert sum(i_runs[a] >= 2 and i_runs[b] == 0 for a, b in pairs(draw, g)) > 100
    assert sum(e[a] >= 7 and e[b] == 0 for a, b in pairs(draw, g)) > 100


def test_place_reads_alternate_on_a_workgroup():
    records, model, reads = G.place_case()
    listed = [r for r in reads if len(r) > 0]  # DCN_PLACE_LANE_BASES = 0
    assert len(listed) == G.PLACE_READS >= 40 and G.trips(len(listed), G.list_items(H)) >= 10
    g = G.stride(len(listed), G.list_items(H))
    for W, slots in ((1, G.PLACE_CELLS), (64, G.PLACE_CELLS)):
        shape = [G.place_shape(model, r, W, slots) for r in listed]
        assert sum(a != b for a, b in pairs(shape, g)) > 20
        # a stitched read (many cells: it fills the set and sweeps in partitions) directly in front of a clean one
        assert sum(a[0] > 4 * slots and a[1] >= 4 and b[0] <= 4 and b[1] == 1 for a, b in pairs(shape, g)) >= 8
    shape = [G.place_shape(model, r, 256, 2048) for r in listed]  # the default set: no partitions, the cells differ
    assert sum(a[0] > 50 and b[0] <= 4 for a, b in pairs(shape, g)) >= 8
    want = model.place_all(listed, W=1)
    assert sum(w[0] != UNPLACED for w in want) > 30


def test_classify_units_alternate_on_a_workgroup():
    U = G.classify_case()
    match, hits, total = U.expected(2, 0.01)
    entries = [len(es) for es in U.units]
    distinct = hits.max(axis=1)
    big = [u for u in range(len(U.units)) if entries[u] > G.CLS_LANE_ENTRIES or distinct[u] > G.CLS_LANE_HITS]
    assert big == list(range(G.CLASSIFY_UNITS)) and len(big) >= 40 and G.trips(len(big), G.list_items(H)) >= 10
    parts = [(int(total[u]) + G.CLS_HALF - 1) // G.CLS_HALF for u in big]
    g = G.stride(len(big), G.list_items(H))
    assert sum(a >= 3 and b == 1 for a, b in pairs(parts, g)) >= 10                       # a lean unit behind one of three partitions
    assert sum(a >= 3 and entries[big[i + g]] <= 40 for i, a in enumerate(parts[:-g])) >= 3    # ... one that qualifies by its hits
    assert sum(entries[u] in (65, 66, 67) for u in big) >= 10 and sum(entries[u] == 40 and distinct[u] == 33 for u in big) >= 9
    assert len({int(t) for t in total}) > 20 and (total < np.array(entries)).any()        # (invalid entries among them)
    assert all(len(m) for m in U.members) and (hits > 0).any(axis=0).all() and (hits == 0).any()


def test_locate_reads_alternate_on_a_wave():
    plan = G.locate_plan()
    assert len(plan) == G.LOCATE_READS >= 100 and all(ln > G.LOC_LANE_BASES for ln, _ in plan)
    assert G.trips(len(plan), G.locate_reads(H)) >= 3
    g = G.stride(len(plan), G.locate_reads(H))
    open_at_end = [max(h) + G.LOC_K == ln for ln, h in plan]
    late = [min(h) >= G.LOC_ITER_BASES + 32 for ln, h in plan]  # no hit in the first 64 words wherever the read starts in a word
    assert sum(a and b for a, b in zip(open_at_end[:-g], late[g:])) >= 10
    assert sum(a != b for a, b in pairs([(ln, tuple(h)) for ln, h in plan], g)) == len(plan) - g
    assert all(0 <= p <= ln - G.LOC_K for ln, h in plan for p in h)


def test_locate_plan_gives_the_segments_it_is_for(oracle):
    import test_gpu_locate_seams as TL
    plan = G.locate_plan()
    g = TL.Genome(oracle, TL.K, sum(ln for ln, _ in plan) + 64, 1941)
    assert g.distinct
    b = TL.Batch(oracle, g)
    for ln, hits in plan:
        b.add(ln, hits)
    want = b.expect(0)  # (asserts that the reads' hits are the plan)
    assert all(len(w) >= 1 for w in want) and len({len(w) for w in want}) > 1
    assert sum(w[-1][1] == ln for w, (ln, h) in zip(want, plan)) >= 40  # the last segment ends with the read
    assert all(w[0][0] >= G.LOC_ITER_BASES + 32 for w, (ln, h) in zip(want, plan) if min(h) >= G.LOC_ITER_BASES + 32)
    assert all(len(w) >= 1 for w in b.expect(40, 2)) and {len(w) for w in b.expect(2000)} == {1}


@pytest.mark.parametrize("case", [c for c in G.SEAM_CASES if c[0] in G.CPU_PROVEN], ids=G.seam_id)
def test_seam_cases_taken_again_exceed_the_cap(oracle, dcn, case):
    """the seam cases of verify, align and extend that the hooked run takes, answered by the models: their largest call has
    more rows than one trip takes at one CU"""
    import importlib
    records = importlib.import_module(case[0]).make_records()
    counting = G.run_seam_case(case, (dcn, oracle, records, None), G.ModelPlacer(records))
    for name in case[3]:
        G.assert_looped(counting, name)

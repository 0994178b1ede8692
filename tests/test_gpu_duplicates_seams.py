"""The seams of duplicates.hip, on the smallest shapes at which it can go wrong, against the dict model of
tests/_duplicates_worker.py: two equal keys around the edges of a wave and of a workgroup of 256 units; a thousand copies of
one key racing for one slot among a thousand other keys; keys that differ in exactly one component; a negative pos5 at the
start of a record beside a read near the end of the record in front; a split read whose first row is unplaced; units without
a key; a duplicate of an earlier call; and a table that starts at 4 slots (DCN_DUPLICATE_TABLE_SLOTS), so that it grows
several times, its chains are full and wrap around its end.  No kernel has a capped grid: there is no second trip to test.
Every comparison is exact."""
import numpy as np
import pytest

import _duplicates_worker as DW

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shared_map(dcn, oracle):
    amap = DW.make_map(oracle, dcn, True)
    yield amap
    amap.close()


@pytest.fixture
def amap(shared_map):
    shared_map.duplicates_enable()
    shared_map.duplicates_reset()
    return shared_map


def distinct(u):
    """a row whose end no other u < 2050 has: forward at position u of record 0, from 900 on at position u - 900 of record 1"""
    return [(0, 0, 0, 50, u, u + 50)] if u < 900 else [(1, 0, 0, 50, u - 900, u - 850)]


@pytest.mark.parametrize("a,b", [(0, 1), (63, 64), (255, 256), (62, 63), (64, 65), (0, 599), (511, 512)])
def test_two_equal_keys_at_the_edges_of_a_wave_and_of_a_workgroup(dcn, amap, a, b):
    """600 units, all distinct but units a and b, which share a key that no other has: b is the duplicate, first(a) = first(b) = a"""
    rows = [distinct(u) for u in range(600)]
    rows[a] = rows[b] = [(1, 1, 2, 50, 700, 748)]
    dup, first = DW.check(dcn, amap, DW.Model(), DW.dtypes(dcn)[0], [50] * 600, rows)
    assert sum(dup) == 1 and dup[b] == 1 and first[b] == a and all(first[u] == u for u in range(600) if u != b)


def test_a_thousand_copies_of_one_key_among_a_thousand_others(dcn, amap):
    """one call: the copies race for one slot (compare-and-swap, then atomicMin); only the smallest ordinal stays"""
    rng = np.random.default_rng(8)
    where = set(int(x) for x in rng.choice(2000, 1000, replace=False))
    rows = [[(2, 1, u % 7, 50, 300, 350 - u % 7)] if u in where else distinct(u) for u in range(2000)]
    dup, first = DW.check(dcn, amap, DW.Model(), DW.dtypes(dcn)[1], [50] * 2000, rows)
    lowest = min(where)
    assert sum(dup) == 999 and all(first[u] == lowest for u in where) and all(first[u] == u for u in range(2000) if u not in where)
    assert amap.duplicates_info() == (2000, 2000, 1001)
    # ... and again in a second call: every copy now reports the first call's ordinal
    dup, first = DW.check(dcn, amap, _continue(amap, rows), DW.dtypes(dcn)[1], [50] * 2000, rows)
    assert sum(dup) == 2000 and all(first[u] == lowest for u in where) and all(first[u] == u for u in range(2000) if u not in where)


def _continue(amap, rows):
    """a model that has seen `rows` once as one call of reads of 50 bases"""
    m = DW.Model()
    m.mark([50] * len(rows), rows)
    assert m.info() == amap.duplicates_info()
    return m


def test_keys_that_differ_in_exactly_one_component(dcn, amap):
    dtype = DW.dtypes(dcn)[2]
    base = (0, 0, 0, 100, 100, 200)
    others = [(1, 0, 0, 100, 100, 200),   # record
              (0, 1, 0, 100, 0, 100),     # strand, at the same pos5 = 100
              (0, 0, 0, 100, 101, 201),   # pos5 by 1
              (0, 0, 0, 100, 99, 199)]
    for both_ends in (False, True):
        amap.duplicates_reset()
        model = DW.Model()
        rows = [[base]] + [[x] for x in others] + [[base]]
        dup, first = DW.check(dcn, amap, model, dtype, [100] * len(rows), rows, both_ends=both_ends)
        assert dup == [0] * 5 + [1] and first == [0, 1, 2, 3, 4, 0]
        # pos3 alone: one key without both_ends, two with
        amap.duplicates_reset()
        model = DW.Model()
        dup, _ = DW.check(dcn, amap, model, dtype, [100] * 2, [[base], [(0, 0, 0, 100, 100, 201)]], both_ends=both_ends)
        assert dup == ([0, 0] if both_ends else [0, 1])
    # the mode bits: the same rows handed in under another mode never match what is there
    amap.duplicates_reset()
    model = DW.Model()
    assert DW.check(dcn, amap, model, dtype, [100] * 2, [[base], [base]])[0] == [0, 1]
    assert DW.check(dcn, amap, model, dtype, [100] * 2, [[base], [base]], both_ends=True)[0] == [0, 1]
    assert DW.check(dcn, amap, model, dtype, [100] * 4, [[base], [None], [None], [base]], paired=True) == ([0, 1], [4, 4])
    assert DW.check(dcn, amap, model, dtype, [100] * 4, [[base], [None], [base], [None]], paired=True, both_ends=True) == ([0, 1], [6, 6])
    # one end against two, and the mate swap
    mate = (0, 1, 0, 100, 300, 400)
    dup, first = DW.check(dcn, amap, model, dtype, [100] * 8, [[base], [mate], [mate], [base], [base], [base], [mate], [None]], paired=True)
    assert dup == [0, 1, 0, 0] and first == [8, 8, 10, 11]
    assert amap.duplicates_info() == model.info() == (12, 12, 7)


def test_a_negative_pos5_at_a_record_start_beside_the_end_of_the_record_in_front(dcn, amap):
    """Record 0 has 1000 bases.  A forward read at the start of record 1, clipped by 5, has pos5 = -5; a coordinate over the
    concatenated records would put it at 995 of record 0, where another read begins.  A reverse read that hangs 5 over the
    end of record 0 has pos5 = 1005, against a read at 5 of record 1."""
    assert DW.REC_LENS[0] == 1000
    dtype = DW.dtypes(dcn)[0]
    rows = [[(1, 0, 5, 100, 0, 95)], [(0, 0, 0, 100, 995, 1000)], [(0, 1, 5, 100, 905, 1000)], [(1, 0, 0, 100, 5, 105)], [(1, 1, 5, 100, 0, 0)],
            [(1, 0, 9, 100, 4, 95)], [(0, 1, 1, 100, 905, 1000)]]
    dup, first = DW.check(dcn, amap, DW.Model(), dtype, [100] * len(rows), rows)
    assert dup == [0, 0, 0, 0, 0, 1, 0] and first == [0, 1, 2, 3, 4, 0, 6]


def test_a_split_read_whose_first_row_is_unplaced_takes_its_second(dcn, amap):
    dtype = DW.dtypes(dcn)[1]
    a, b = (0, 0, 0, 50, 100, 150), (1, 1, 0, 50, 400, 450)
    rows = [[a], [None, a, b], [None, None, b], [b, a], [None], [], [a, None]]
    dup, first = DW.check(dcn, amap, DW.Model(), dtype, [50] * len(rows), rows)
    assert dup == [0, 1, 0, 1, 0, 0, 1] and first == [0, 0, 2, 2, DW.NO_FIRST, DW.NO_FIRST, 0]


def test_units_without_a_key_consume_an_ordinal_and_earlier_calls_are_remembered(dcn, amap):
    dtype = DW.dtypes(dcn)[0]
    model = DW.Model()
    assert DW.check(dcn, amap, model, dtype, [50] * 4, [[None], [None], distinct(7), [None]]) == ([0, 0, 0, 0], [DW.NO_FIRST, DW.NO_FIRST, 2, DW.NO_FIRST])
    assert amap.duplicates_info() == (4, 1, 1)
    assert DW.check(dcn, amap, model, dtype, [50] * 3, [[None], distinct(8), distinct(7)]) == ([0, 0, 1], [DW.NO_FIRST, 5, 2])
    assert DW.check(dcn, amap, model, dtype, [50] * 4, [[None], [None], [None], [None]], paired=True) == ([0, 0], [DW.NO_FIRST] * 2)
    assert DW.check(dcn, amap, model, dtype, [50] * 2, [distinct(8), distinct(7)]) == ([1, 1], [5, 2])
    assert amap.duplicates_info() == (11, 5, 2)


def run_growth(dcn, amap):
    rng = np.random.default_rng(21)
    model = DW.Model()
    out = []
    for n, rate, paired in ((500, 0.3, False), (4, 0.0, False), (300, 0.5, True), (700, 0.2, False)):
        lengths, rows = DW.random_units(rng, n, rate, DW.REC_LENS, paired=paired)
        if out:  # half of the units repeat units of the first call
            keep = len(lengths) // 2 // 2 * 2
            lengths, rows = lengths[:keep] + out[0][2][:keep], rows[:keep] + out[0][3][:keep]
        got = DW.check(dcn, amap, model, DW.dtypes(dcn)[1], lengths, rows, paired, True)
        out.append((got, amap.duplicates_info(), lengths, rows))
    return [(x[0], x[1]) for x in out]


def test_a_table_that_starts_at_four_slots_grows_and_wraps(dcn, oracle, monkeypatch):
    """DCN_DUPLICATE_TABLE_SLOTS=4, read when a set first grows: a call of 500 units and three more behind it.  The table is
    rehashed from 4 slots to 1024, then 2048, ...; at two slots per key, chains run into one another and around the table's
    end.  The results equal the model's and those of a set that started at the default size."""
    results = []
    for slots in ("4", None):
        if slots:
            monkeypatch.setenv("DCN_DUPLICATE_TABLE_SLOTS", slots)
        else:
            monkeypatch.delenv("DCN_DUPLICATE_TABLE_SLOTS")
        amap = DW.make_map(oracle, dcn, False)
        try:
            amap.duplicates_enable()
            results.append(run_growth(dcn, amap))
        finally:
            amap.close()
    assert results[0] == results[1] and sum(results[0][0][0][0]) > 100 and sum(results[0][3][0][0]) > 300


def test_a_table_at_exactly_two_slots_per_key(dcn, oracle, monkeypatch):
    """all keys distinct and a power of two of them: the table is as full as it gets (slots = 2 x keys), call after call"""
    monkeypatch.setenv("DCN_DUPLICATE_TABLE_SLOTS", "2")
    amap = DW.make_map(oracle, dcn, False)
    try:
        amap.duplicates_enable()
        model = DW.Model()
        at = 0
        for n in (1, 1, 2, 4, 8, 240, 256, 512):  # keys so far + units = 1, 2, 4, 8, 16, 256, 512, 1024
            rows = [[(u % 3, (u // 3) % 2, 0, 50, 1000 + u, 1050 + u)] for u in range(at, at + n)]
            dup, first = DW.check(dcn, amap, model, DW.dtypes(dcn)[0], [50] * n, rows)
            assert sum(dup) == 0 and first == list(range(at, at + n))
            at += n
        rows = [[(u % 3, 0, 3, 50, 1003 + u, 1050 + u) if (u // 3) % 2 == 0 else (u % 3, 1, 3, 50, 1000 + u, 1047 + u)] for u in range(at)]  # again, clipped
        dup, first = DW.check(dcn, amap, model, DW.dtypes(dcn)[0], [50] * at, rows)
        assert sum(dup) == at and first == list(range(at)) and amap.duplicates_info() == (2 * at, 2 * at, at)
    finally:
        amap.close()

"""Set algebra on the GPU (dcn_index_set_select, dcn_index_set_overlap, dcn_index_intersect) against numpy set algebra over
the members' key arrays.  Index.from_keys takes arbitrary u64, so the members are mix64 keys (and key 0, put in directly)
with planned overlaps; no sequence and no oracle is needed except where a FilterProcessor reads the result."""
import ctypes as C
from functools import reduce

import numpy as np
import pytest

from conftest import mix64, random_reads

pytestmark = pytest.mark.gpu

K, W = 31, 15


def ids(lo, hi):
    return mix64(np.arange(lo, hi, dtype=np.uint64))


# ---- numpy truth ----------------------------------------------------------------------------------------------------
def masks_of(members):
    """(distinct keys of the union, sorted; u32 member mask of each)"""
    keys = np.unique(np.concatenate([np.asarray(m, np.uint64) for m in members]))
    mask = np.zeros(len(keys), np.uint32)
    for j, m in enumerate(members):
        mask[np.isin(keys, m)] |= np.uint32(1 << j)
    return keys, mask


def bits_of(mask, n):
    return ((mask[:, None] >> np.arange(n, dtype=np.uint32)[None, :]) & np.uint32(1)).astype(np.int64)


def select_truth(keys, mask, n, all_of=0, any_of=0, none_of=0, min_members=0, max_members=0):
    c = bits_of(mask, n).sum(1)
    ok = (mask & np.uint32(all_of)) == np.uint32(all_of)
    if any_of:
        ok &= (mask & np.uint32(any_of)) != 0
    ok &= (mask & np.uint32(none_of)) == 0
    ok &= (c >= max(min_members, 1)) & (c <= (max_members or 32))
    return keys[ok]  # sorted, as keys is


def overlap_truth(mask, n):
    b = bits_of(mask, n)
    c = b.sum(1)
    return b.T @ b, (b * (c == 1)[:, None]).sum(0), np.bincount(c, minlength=n + 1)[1:n + 1]


def default_preds(n):
    full = (1 << n) - 1
    preds = [dict(), dict(any_of=full), dict(all_of=1), dict(all_of=1, max_members=1), dict(min_members=2),
             dict(min_members=n), dict(max_members=1), dict(all_of=full), dict(any_of=1 | (1 << (n - 1))),
             dict(min_members=1, max_members=n), dict(all_of=1, none_of=1)]  # the last one: nothing can satisfy it
    if n >= 2:
        preds += [dict(all_of=1, none_of=2), dict(any_of=2, none_of=1, max_members=2), dict(all_of=3, none_of=1 << (n - 1))]
    return preds


def check_set(dcn, members, preds=None):
    """a set over `members` (key arrays): overlap and every predicate's selection against numpy; -> (set, indexes)"""
    n = len(members)
    idx = [dcn.Index.from_keys(m, K, W) for m in members]
    s = dcn.IndexSet(idx)
    keys, mask = masks_of(members)
    assert len(s) == len(keys)
    ov = s.overlap()
    shared, exclusive, by_count = overlap_truth(mask, n)
    assert np.array_equal(ov["shared"].astype(np.int64), shared), (ov["shared"], shared)
    assert np.array_equal(ov["shared"], ov["shared"].T)
    assert [int(x) for x in np.diag(ov["shared"])] == [len(i) for i in idx] == [len(np.unique(m)) for m in members]
    assert np.array_equal(ov["exclusive"].astype(np.int64), exclusive)
    assert np.array_equal(ov["by_count"].astype(np.int64), by_count)
    assert int(ov["by_count"].sum()) == len(s)
    probe = np.concatenate([keys[:256], ids(1 << 40, (1 << 40) + 64)])
    for pred in (default_preds(n) if preds is None else preds):
        want = select_truth(keys, mask, n, **pred)
        assert s.select(count_only=True, **pred) == len(want), pred
        got = s.select(**pred)
        assert len(got) == got.header()[2] == len(want), pred
        assert np.array_equal(np.sort(got.keys()), want), pred
        assert (got.kmer_length, got.window_size) == (K, W)
        assert np.array_equal(got.contains(probe), np.isin(probe, want)), pred
        got.close()
    return s, idx


def check_intersect(dcn, members):
    idx = [dcn.Index.from_keys(m, K, W) for m in members]
    got = dcn.Index.intersect(idx)
    want = reduce(np.intersect1d, [np.asarray(m, np.uint64) for m in members])
    assert len(got) == got.header()[2] == len(want)
    assert np.array_equal(np.sort(got.keys()), want)
    probe = np.concatenate([np.unique(np.concatenate(members))[:256], ids(1 << 40, (1 << 40) + 64)])
    assert np.array_equal(got.contains(probe), np.isin(probe, want))
    return got, idx


def plan3(zero_in=()):
    """3 members of ~2,000 keys: exclusive keys, every pairwise-only overlap, a triple overlap; key 0 where asked"""
    a = [ids(1, 1001), ids(3001, 3401), ids(3401, 3701), ids(4101, 4601)]
    b = [ids(1001, 2001), ids(3001, 3401), ids(3701, 4101), ids(4101, 4601)]
    c = [ids(2001, 3001), ids(3401, 3701), ids(3701, 4101), ids(4101, 4601)]
    members = [np.concatenate(m) for m in (a, b, c)]
    return [np.concatenate([m, np.zeros(1, np.uint64)]) if j in zero_in else m for j, m in enumerate(members)]


def small_processor(dcn, index, **kw):
    return dcn.FilterProcessor(index, max_batch_bases=1 << 20, max_batch_reads=1 << 12, **kw)


# ---- select / overlap / intersect against numpy ------------------------------------------------------------------------
def test_three_members_with_planned_overlaps(dcn):
    check_set(dcn, plan3())
    check_intersect(dcn, plan3())
    check_intersect(dcn, plan3()[:2])


def test_masks_as_iterables_and_ints_agree(dcn):
    members = plan3()
    s = dcn.IndexSet([dcn.Index.from_keys(m, K, W) for m in members])
    assert s.select(all_of=[0, 2], count_only=True) == s.select(all_of=5, count_only=True) == 800
    assert s.select(any_of={1}, none_of=(0,), count_only=True) == s.select(any_of=2, none_of=1, count_only=True) == 1400


def test_cross_checks_against_union_and_diff(dcn):
    members = plan3(zero_in=(0, 1))
    a, b, c = idx = [dcn.Index.from_keys(m, K, W) for m in members]
    s = dcn.IndexSet(idx)
    assert np.array_equal(np.sort(s.select(any_of=[0, 1, 2]).keys()), np.sort(dcn.Index.union(idx).keys()))
    assert np.array_equal(np.sort(s.select(all_of={0}, none_of={1}).keys()), np.sort(a.diff(b).keys()))
    assert np.array_equal(np.sort(dcn.Index.intersect([a, b]).keys()), np.sort(a.diff(a.diff(b)).keys()))
    assert np.array_equal(np.sort(dcn.Index.intersect([a]).keys()), np.sort(a.keys()))
    # a labelled set counts as the union of its members
    assert np.array_equal(np.sort(dcn.Index.intersect([s, c]).keys()), np.sort(c.keys()))


def test_intersect_of_33_indexes(dcn):
    core = ids(1, 11)
    members = [np.concatenate([core, ids(100 * (j + 1), 100 * (j + 1) + 40 + j)]) for j in range(33)]
    members[7] = np.concatenate([members[7], np.zeros(1, np.uint64)])  # key 0 in one input only: not in the result
    got, _ = check_intersect(dcn, members)
    assert len(got) == 10
    got, _ = check_intersect(dcn, [np.concatenate([m, np.zeros(1, np.uint64)]) for m in members])
    assert len(got) == 11


# ---- key 0 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zero_in", [(), (1,), (0, 2), (0, 1, 2)])
def test_key_zero_in_some_all_or_none_of_the_members(dcn, zero_in):
    members = plan3(zero_in)
    s, _ = check_set(dcn, members)
    keys, mask = masks_of(members)
    assert (0 in keys) == bool(zero_in)
    ov = s.overlap()
    for i in range(3):
        for j in range(3):  # key 0 is one of the keys behind each cell it belongs to
            without = len(np.intersect1d(members[i][members[i] != 0], members[j][members[j] != 0]))
            assert int(ov["shared"][i, j]) == without + (1 if i in zero_in and j in zero_in else 0)
    if zero_in:
        assert int(ov["by_count"][len(zero_in) - 1]) == int(overlap_truth(mask[keys != 0], 3)[2][len(zero_in) - 1]) + 1
        assert 0 in s.select(all_of=list(zero_in)).keys()
        assert 0 not in s.select(none_of=[zero_in[0]]).keys()
    got, _ = check_intersect(dcn, members)
    assert (0 in got.keys()) == (len(zero_in) == 3)


# ---- member limits --------------------------------------------------------------------------------------------------------
def test_one_member(dcn):
    m = np.concatenate([ids(1, 200), np.zeros(1, np.uint64)])
    s, _ = check_set(dcn, [m])
    ov = s.overlap()
    assert ov["shared"].shape == (1, 1) and int(ov["shared"][0, 0]) == int(ov["exclusive"][0]) == int(ov["by_count"][0]) == 200


@pytest.mark.parametrize("zero_in_all", [False, True])
def test_32_members(dcn, zero_in_all):
    everyone = ids(1, 2)            # label 0xFFFFFFFF
    all_but_last = ids(2, 4)        # 31 members
    members = []
    for j in range(32):
        m = [everyone, ids(1000 + 64 * j, 1000 + 64 * j + 56), ids(9000 + j, 9001 + j), ids(9000 + (j + 1) % 32, 9001 + (j + 1) % 32)]
        if j < 31:
            m.append(all_but_last)
        if zero_in_all:
            m.append(np.zeros(1, np.uint64))
        members.append(np.concatenate(m))
    last = 1 << 31
    preds = [dict(min_members=1, max_members=1), dict(min_members=31, max_members=31), dict(min_members=32, max_members=32),
             dict(min_members=32), dict(min_members=31), dict(max_members=31), dict(max_members=32), dict(min_members=2, max_members=31),
             dict(all_of=last, max_members=1), dict(all_of=0xFFFFFFFF), dict(none_of=last), dict(any_of=last | 1, min_members=2),
             dict(all_of=0x7FFFFFFF, none_of=last)]
    s, _ = check_set(dcn, members, preds)  # (the whole 32 x 32 shared matrix is compared in there)
    ov = s.overlap()
    assert int(ov["by_count"][31]) == (2 if zero_in_all else 1) and int(ov["by_count"][30]) == 2
    assert int(ov["exclusive"][31]) == 56 and int(ov["shared"][31, 0]) == 2 + (1 if zero_in_all else 0)
    assert s.select(all_of=last, max_members=1, count_only=True) == 56
    assert s.select(all_of=0xFFFFFFFF, count_only=True) == (2 if zero_in_all else 1)


# ---- table shapes ---------------------------------------------------------------------------------------------------------
SMALL_CASES = {
    "one key, one member": lambda: [ids(1, 2)],
    "one key, two members": lambda: [ids(1, 2), ids(1, 2)],
    "only key 0": lambda: [np.zeros(1, np.uint64), np.zeros(1, np.uint64)],
    "16 keys": lambda: [ids(1, 9), ids(5, 13), ids(9, 17)],
    # 60 keys over the members: with 2 slots per key the set's 128 slots hold 54 keys
    "60 keys": lambda: [ids(1, 25), ids(22, 42), ids(39, 55)],
    "planned": plan3,
}


@pytest.mark.parametrize("slots_per_key", [None, "2"])
@pytest.mark.parametrize("case", list(SMALL_CASES))
def test_small_tables(dcn, monkeypatch, case, slots_per_key):
    """a table smaller than a wave's quads; under DCN_TABLE_SLOTS_PER_KEY=2 second slots and displaced groups are occupied,
    in the set and in the selected index alike (it is built under the same setting)"""
    if slots_per_key:
        monkeypatch.setenv("DCN_TABLE_SLOTS_PER_KEY", slots_per_key)
    members = SMALL_CASES[case]()
    s, idx = check_set(dcn, members)
    if slots_per_key and case == "60 keys":
        assert s.memory == 128 * 12  # 64 groups of 2 slots (8 B) and masks (4 B): load 54 / 128
    check_intersect(dcn, members)


def test_grid_stride_loop_iterates(dcn):
    """~300,000 keys: 4 Mi slots = 1 Mi mask quads, more than the 256 threads x 8 workgroups per CU of the launch"""
    members = [ids(1, 200_001), ids(100_001, 300_001), ids(250_001, 300_101)]
    preds = [dict(), dict(all_of=1, max_members=1), dict(min_members=2), dict(all_of=7), dict(all_of=2, none_of=4)]
    s, _ = check_set(dcn, members, preds)
    assert s.memory >= (1 << 22) * 12
    check_intersect(dcn, members)
    check_intersect(dcn, members[:2])


# ---- empty results --------------------------------------------------------------------------------------------------------
def test_empty_results_are_valid_indexes(dcn):
    rng = np.random.default_rng(5)
    members = plan3()
    s = dcn.IndexSet([dcn.Index.from_keys(m, K, W) for m in members])
    nothing = s.select(all_of=[0], none_of=[0])
    disjoint = dcn.Index.intersect([dcn.Index.from_keys(ids(1, 500), K, W), dcn.Index.from_keys(ids(500, 900), K, W)])
    bases, offsets = dcn.concat_reads(random_reads(rng, 50, 150, 150))
    for e in (nothing, disjoint):
        assert len(e) == e.header()[2] == 0 and len(e.keys()) == 0
        assert not e.contains(np.concatenate([members[0][:300], np.zeros(1, np.uint64)])).any()
        keep, hits, total = small_processor(dcn, e).filter_batch(bases, offsets)
        assert not keep.any() and not hits.any() and total.all()


# ---- the result is an ordinary index ----------------------------------------------------------------------------------------
def test_selected_index_filters_like_one_built_from_the_truth(dcn, tmp_path):
    rng = np.random.default_rng(11)
    reads = random_reads(rng, 200, 150, 150)
    bases, offsets = dcn.concat_reads(reads)
    seed = dcn.Index.from_keys(ids(1, 10), K, W)
    _, hashes, _ = small_processor(dcn, seed).minimizer_hashes_batch(bases, offsets)
    h = np.unique(hashes)
    assert len(h) > 1000
    third = len(h) // 3
    members = [np.concatenate([h[:2 * third], ids(1, 300)]), np.concatenate([h[third:], ids(200, 500)]),
               np.concatenate([h[::2], ids(400, 700)])]
    keys, mask = masks_of(members)
    s = dcn.IndexSet([dcn.Index.from_keys(m, K, W) for m in members])
    for pred in (dict(min_members=2), dict(all_of=[0], max_members=1), dict(any_of=[1, 2], none_of=[0])):
        want = select_truth(keys, mask, 3, **{k: (s._mask(v) if k.endswith("_of") else v) for k, v in pred.items()})
        assert 0 < len(np.intersect1d(want, h)) < len(h)  # some of the reads' minimizers are selected, not all
        got, ref = s.select(**pred), dcn.Index.from_keys(want, K, W)
        a = small_processor(dcn, got).filter_batch(bases, offsets)
        b = small_processor(dcn, ref).filter_batch(bases, offsets)
        assert a[0].any() and a[1].any()
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        path = tmp_path / "selected.idx"
        got.write(path)
        back = dcn.Index.from_file(path)
        assert back.header() == got.header() == (K, W, len(want))
        assert np.array_equal(np.sort(back.keys()), want)


def test_k_w_and_minimizer_rule_are_inherited(dcn):
    a_keys, b_keys = ids(1, 300), ids(200, 500)
    default_rule = dcn.Index.from_keys(a_keys, 21, 11)
    dcn.set_minimizer_variant(7, 32, "xor")
    try:
        a, b = dcn.Index.from_keys(a_keys, 21, 11), dcn.Index.from_keys(b_keys, 21, 11)
        s = dcn.IndexSet([a, b])
    finally:
        dcn.set_minimizer_variant(1, 16, "add")
    sel, both = s.select(all_of=[0]), dcn.Index.intersect([a, b])  # made while the process-wide rule is the default again
    for r in (sel, both):
        assert (r.kmer_length, r.window_size) == (21, 11)
        assert len(dcn.Index.union([r, a])) == 299  # same rule as the members: accepted
        with pytest.raises(dcn.DeaconHipError) as e:
            dcn.Index.union([r, default_rule])
        assert e.value.code == dcn._native.DCN_ERR_ARG and "minimizer rules" in e.value.message


# ---- the set is left as it was ------------------------------------------------------------------------------------------------
def test_select_and_overlap_leave_the_set_and_its_coverage_alone(dcn):
    rng = np.random.default_rng(3)
    bases, offsets = dcn.concat_reads(random_reads(rng, 40, 150, 150))
    seed = dcn.Index.from_keys(ids(1, 10), K, W)
    _, hashes, _ = small_processor(dcn, seed).minimizer_hashes_batch(bases, offsets)
    h = np.unique(hashes)
    members = [np.concatenate([h[::2], ids(1, 300)]), np.concatenate([h[::3], ids(200, 500)])]
    s = dcn.IndexSet([dcn.Index.from_keys(m, K, W) for m in members])
    s.enable_coverage()
    cl = dcn.Classifier(s, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    cl.classify_batch(bases, offsets)
    observed, keys = s.coverage()
    assert observed.sum() > 0
    n_before = len(s)
    sel = s.select(all_of=[0, 1])
    s.overlap()
    s.select(min_members=1, count_only=True)
    after = s.coverage()
    assert np.array_equal(after[0], observed) and np.array_equal(after[1], keys)
    N = dcn._native
    info = [C.c_uint32(), C.c_uint8(), C.c_uint8(), C.c_uint64(), C.c_uint64()]
    assert N.lib().dcn_index_set_info(s._h, *[C.byref(x) for x in info]) == 0 and info[3].value == n_before == len(s)
    # the selected index is plain: no masks, no coverage
    assert N.lib().dcn_index_set_info(sel._h, *[C.byref(x) for x in info]) == N.DCN_ERR_ARG
    assert N.lib().dcn_index_set_coverage_enable(sel._h, 1) == N.DCN_ERR_ARG


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_argument_errors(dcn):
    N = dcn._native
    L = N.lib()
    plain = dcn.Index.from_keys(ids(1, 100), K, W)
    s = dcn.IndexSet([plain, dcn.Index.from_keys(ids(50, 150), K, W), dcn.Index.from_keys(ids(100, 200), K, W)])
    n, h = C.c_uint64(), C.c_void_p()
    out = np.zeros(9, np.uint64)
    p = out.ctypes.data_as(C.c_void_p)
    assert L.dcn_index_set_select(plain._h, 0, 0, 0, 0, 0, C.byref(n), C.byref(h)) == N.DCN_ERR_ARG
    assert b"not a labelled set" in L.dcn_last_error()
    assert L.dcn_index_set_overlap(plain._h, p, p, p) == N.DCN_ERR_ARG
    assert b"not a labelled set" in L.dcn_last_error()
    for pred in (dict(all_of=[3]), dict(any_of=8), dict(none_of=1 << 31), dict(min_members=3, max_members=2)):
        with pytest.raises(dcn.DeaconHipError) as e:
            s.select(count_only=True, **pred)
        assert e.value.code == N.DCN_ERR_ARG, pred
    assert s.select(min_members=4, count_only=True) == 0  # more members than the set has: well formed, nothing meets it
    assert L.dcn_index_set_select(s._h, 0, 0, 0, 0, 0, None, None) == N.DCN_ERR_ARG
    assert L.dcn_index_set_overlap(s._h, None, None, None) == N.DCN_ERR_ARG
    # any single output of overlap may be asked for alone
    assert L.dcn_index_set_overlap(s._h, None, None, p) == 0 and int(out[:3].sum()) == len(s)
    for other in (dcn.Index.from_keys(ids(1, 100), 21, 11), dcn.Index.from_keys(ids(1, 100), K, W + 2)):
        with pytest.raises(dcn.DeaconHipError) as e:
            dcn.Index.intersect([plain, other])
        assert e.value.code == N.DCN_ERR_ARG and "Incompatible headers" in e.value.message
    dcn.set_minimizer_variant(7, 32, "xor")
    try:
        other = dcn.Index.from_keys(ids(1, 100), K, W)
    finally:
        dcn.set_minimizer_variant(1, 16, "add")
    with pytest.raises(dcn.DeaconHipError) as e:
        dcn.Index.intersect([plain, other])
    assert e.value.code == N.DCN_ERR_ARG and "minimizer rules" in e.value.message

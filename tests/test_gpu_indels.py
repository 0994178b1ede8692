"""The deletion ledger and the indel genotype on the device, against the model of tests/_indel_worker.py: switching on, off
and reset, rule R1's refusal, both batch calls, rule R2's invariants from a fetch over every position, a second map without
the ledger, info and fetch, the capacity protocol of both calls, and a genotype call with one ledger, the other, both and
neither.  The two short records of tests/test_gpu_pileup_seams.py and rows written by hand.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import _indel_worker as DW
import _insertion_worker as IW
import _pileup_worker as PW
import _verify_worker as VW
from test_gpu_pileup_seams import LEN0, LEN1, Case, make_records, other

pytestmark = pytest.mark.gpu


def gapped_case(dcn, records, seed=70, copies=7):
    """`copies` reads over each of a few intervals of both records, on alternating strands: each interval's reads share a
    deletion (1 - 5 bases) and an insertion, about half of them carry a second deletion"""
    c = Case(dcn, records, seed)
    for R, a, d_at, d_len, i_at in ((0, 300, 40, 1, 90), (0, 900, 55, 3, 20), (1, 500, 33, 5, 100), (1, 1200, 64, 2, 10), (0, 2500, 100, 4, 50)):
        T = records[R][a:a + 160]
        for q in range(copies):
            s = [T[p:p + 1] for p in range(160)]
            for p in range(d_at, d_at + d_len):
                s[p] = b""
            s[i_at] += other(T[i_at:i_at + 1], T[i_at + 1:i_at + 2]) * (1 + q % 2)
            if q % 2:
                s[130] = s[131] = b""
            c.put(b"".join(s), R, a, a + 160, rev=q % 2)
    return c


def add(c, amap, placer, oracle, counts, ins, dels, quals=False, **kw):
    rows = np.concatenate(c.rows)
    b, o = oracle.concat_reads(c.reads)
    extra = dict(quals=np.full(len(b), 33 + 30, np.uint8)) if quals else {}
    edits, n_added = placer.pileup_batch(b, o, rows, **extra, **kw)
    want_edits, want_added = DW.pile_rows(counts, ins, dels, c.reads, c.records, rows, **kw)
    assert edits.tolist() == want_edits.tolist() and n_added == want_added
    return n_added


@pytest.fixture(scope="module")
def env(dcn, oracle):
    records = make_records()
    amap = VW.build_map(oracle, dcn, records)
    amap.pileup_enable()
    amap.pileup_keep_insertions()
    amap.pileup_keep_deletions()
    placer = dcn.Placer(amap, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    yield dcn, oracle, records, amap, placer
    placer.close()
    amap.close()


def test_both_batch_calls_append_and_r2_holds(env):
    """dcn_pileup_batch and dcn_pileup_batch_qual both append; DEL(q) is the number of events that cover q, and the sum of the
    lengths is the column's total, from a fetch over every position"""
    dcn, O, records, amap, placer = env
    c = gapped_case(dcn, records)
    for quals in (False, True):
        amap.pileup_reset()
        assert amap.deletions_info() == (0, 0)
        counts, ins, dels = PW.new_counts(records), IW.new_ledger(records), DW.new_ledger(records)
        assert add(c, amap, placer, O, counts, ins, dels, quals=quals) == 35
        PW.assert_counts(amap, records, counts)
        total = DW.assert_ledgers(amap, records, counts, ins, dels, settings=(DW.DEFAULTS, dict(min_depth=1, min_gq=0, min_qual=0, min_count=1)))
        assert total[0] >= 50 and total[1] == sum(int(x[:, PW.DEL].sum()) for x in counts)
        assert {e[2] for led in dels for e in led} == {0, 1} and {e[1] for led in dels for e in led} >= {1, 2, 3, 4}
        assert len(DW.sites_range(counts[0], ins[0], dels[0], 0, LEN0)) >= 5
    # a second call adds to the same ledger (rule R3: the same as both in one)
    add(c, amap, placer, O, counts, ins, dels)
    DW.assert_ledgers(amap, records, counts, ins, dels)


def test_a_map_without_the_ledger_has_the_same_counters_sums_and_insertions(env, dcn, oracle):
    dcn, O, records, amap, placer = env
    c = gapped_case(dcn, records, seed=71)
    rows = np.concatenate(c.rows)
    b, o = O.concat_reads(c.reads)
    quals = (33 + (np.arange(len(b)) * 7) % 41).astype(np.uint8)
    got = []
    for keep in (True, False):
        m = VW.build_map(oracle, dcn, records)
        m.pileup_enable()
        m.pileup_keep_insertions()
        m.pileup_keep_qualities()
        if keep:
            m.pileup_keep_deletions()
        p = dcn.Placer(m, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
        edits, n_added = p.pileup_batch(b, o, rows, quals=quals, min_base_qual=10)
        ev = [m.insertions_fetch(R) for R in range(2)]
        got.append((edits.tobytes(), n_added, [m.pileup_fetch(R).tobytes() for R in range(2)], [m.pileup_fetch_qualities(R).tobytes() for R in range(2)],
                    [(e.tobytes(), x) for e, x in ev], m.insertions_info()))
        if keep:
            assert m.deletions_info()[0] >= 50
        else:
            with pytest.raises(dcn.DeaconHipError) as e:
                m.deletions_info()
            assert e.value.code == dcn._native.DCN_ERR_ARG and "keeps no deletion ledger" in e.value.message
        p.close()
        m.close()
    assert got[0] == got[1] and got[0][1] == 35


def test_keep_reset_disable_clone_and_r1(env, dcn, oracle):
    dcn, O, records, amap, placer = env
    N = dcn._native
    L = N.lib()
    c = gapped_case(dcn, records, seed=72)
    rows = np.concatenate(c.rows)
    b, o = O.concat_reads(c.reads)
    m = VW.build_map(oracle, dcn, records)
    p = dcn.Placer(m, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    with pytest.raises(dcn.DeaconHipError) as e:
        m.pileup_keep_deletions()
    assert e.value.code == N.DCN_ERR_ARG and "no pileup" in e.value.message
    m.pileup_enable()
    for call in (m.deletions_info, lambda: m.deletions_fetch(0)):
        with pytest.raises(dcn.DeaconHipError) as e:
            call()
        assert e.value.code == N.DCN_ERR_ARG and "keeps no deletion ledger" in e.value.message
    with pytest.raises(dcn.DeaconHipError) as e:  # neither ledger
        m.indels_genotype(0)
    assert e.value.code == N.DCN_ERR_ARG and "keeps neither an insertion ledger nor a deletion ledger" in e.value.message
    m.pileup_keep_deletions(False)  # (nothing to drop)
    _, n_added = p.pileup_batch(b, o, rows)
    bare = [m.pileup_fetch(R).copy() for R in range(2)]
    with pytest.raises(dcn.DeaconHipError) as e:  # rule R1: a row has added
        m.pileup_keep_deletions()
    assert e.value.code == N.DCN_ERR_ARG and "%d rows have added" % n_added in e.value.message and "a ledger begins with the counters" in e.value.message
    m.pileup_reset()
    m.pileup_keep_deletions()  # fine after a reset
    m.pileup_keep_deletions()  # again: nothing changes
    assert m.deletions_info() == (0, 0) and len(m.deletions_fetch(0)) == 0 and len(m.indels_genotype(0)[0]) == 0
    p.pileup_batch(b, o, rows)
    assert all(np.array_equal(m.pileup_fetch(R), bare[R]) for R in range(2))  # the eight counters are what they are without a ledger
    info, held = m.deletions_info(), [m.deletions_fetch(R).tobytes() for R in range(2)]
    assert info[0] >= 50 and info[1] == sum(int(x[:, PW.DEL].sum()) for x in bare)
    # only the deletion ledger: deletion sites alone; then with the insertion ledger only
    only_del = [m.indels_genotype(R) for R in range(2)]
    assert all((s["flags"] & N.INDEL_DELETION).all() and x == b"" for s, x in only_del) and sum(len(s) for s, _ in only_del) >= 5
    clone = m.clone(0)  # an index without the ledger
    n1, n2 = C.c_uint64(), C.c_uint64()
    assert L.dcn_anchor_map_deletions_info(clone._h, C.byref(n1), C.byref(n2)) == N.DCN_ERR_ARG
    clone.close()
    m.pileup_keep_deletions(False)  # leaves the counters; keeping again is refused until a reset
    assert all(np.array_equal(m.pileup_fetch(R), bare[R]) for R in range(2))
    with pytest.raises(dcn.DeaconHipError):
        m.deletions_info()
    with pytest.raises(dcn.DeaconHipError):
        m.pileup_keep_deletions()
    m.pileup_reset()
    m.pileup_keep_insertions()
    p.pileup_batch(b, o, rows)
    only_ins = [m.indels_genotype(R) for R in range(2)]
    assert all(not (s["flags"] & N.INDEL_DELETION).any() for s, _ in only_ins) and sum(len(s) for s, _ in only_ins) >= 5
    m.pileup_reset()
    m.pileup_keep_deletions()
    p.pileup_batch(b, o, rows)
    assert [m.deletions_fetch(R).tobytes() for R in range(2)] == held and m.deletions_info() == info
    both = [m.indels_genotype(R) for R in range(2)]
    for R in range(2):  # both ledgers: the two kinds merged; each kind's sites are what the map with one ledger gave
        got = DW.device_sites(*both[R])
        assert [s for s in got if s[1] & DW.INDEL_DELETION] == DW.device_sites(*only_del[R])
        assert [s for s in got if not s[1] & DW.INDEL_DELETION] == DW.device_sites(*only_ins[R])
        assert both[R][1] == only_ins[R][1] and (np.diff(both[R][0]["pos"].astype(np.int64)) >= 0).all()
    # a refused call leaves counters and ledger alone
    bad = rows.copy()
    bad["ref_end"][3] = LEN0 + LEN1 + 5
    with pytest.raises(dcn.DeaconHipError) as e:
        p.pileup_batch(b, o, bad)
    assert e.value.code == N.DCN_ERR_ARG and "row 3" in e.value.message
    assert [m.deletions_fetch(R).tobytes() for R in range(2)] == held and all(np.array_equal(m.pileup_fetch(R), bare[R]) for R in range(2))
    m.pileup_disable()  # frees the ledger with the pileup; a new pileup has none
    m.pileup_enable()
    with pytest.raises(dcn.DeaconHipError) as e:
        m.deletions_info()
    assert "keeps no deletion ledger" in e.value.message
    p.close()
    m.close()


def test_fetch_ranges_and_errors(env):
    dcn, O, records, amap, placer = env
    N = dcn._native
    L = N.lib()
    c = gapped_case(dcn, records, seed=73)
    amap.pileup_reset()
    counts, ins, dels = PW.new_counts(records), IW.new_ledger(records), DW.new_ledger(records)
    add(c, amap, placer, O, counts, ins, dels)
    starts = sorted({e[0] for e in dels[1]})
    p0 = starts[0]
    for start, n in ((0, LEN1), (p0, 1), (p0 + 1, 1), (p0 - 1, 1), (0, p0), (0, p0 + 1), (p0 + 1, LEN1 - p0 - 1), (LEN1 - 1, 1), (7, 0), (LEN1, 0)):
        assert DW.deletions_as_tuples(amap.deletions_fetch(1, start, n)) == DW.fetch_range(dels[1], start, n), (start, n)
        DW.assert_sites(amap, counts[1], ins[1], dels[1], 1, start, n)
    n = C.c_uint64(5)
    assert L.dcn_anchor_map_deletions_fetch(amap._h, 1, 7, 0, None, 0, C.byref(n)) == 0 and n.value == 0
    assert L.dcn_anchor_map_deletions_fetch(amap._h, 1, 0, LEN1, None, 0, None) == N.DCN_ERR_ARG and b"n_events is NULL" in L.dcn_last_error()
    prm = N.IndelParams(2, 3, 20, 20, 2, 2000, 301, 0)
    m = C.c_uint64(5)
    for args, word in (((2, 0, 1), b"record 2 of 2 added"), ((1, LEN1, 1), b"past the record's"), ((1, 0, LEN1 + 1), b"past the record's")):
        assert L.dcn_anchor_map_deletions_fetch(amap._h, *args, None, 0, C.byref(n)) == N.DCN_ERR_ARG
        assert word in L.dcn_last_error() and b"deletions fetch" in L.dcn_last_error()
        assert L.dcn_anchor_map_indels_genotype(amap._h, C.byref(prm), *args, None, 0, None, 0, C.byref(n), C.byref(m)) == N.DCN_ERR_ARG
        assert word in L.dcn_last_error() and b"indels genotype" in L.dcn_last_error()
    # the parameter checks come first, in the struct's order, before the map is looked at
    for p, word in ((None, b"params is NULL"), (C.byref(N.IndelParams(3, 0, 100, 0, 0, 100001, 100001, 1)), b"params.reserved must be 0"),
                    (C.byref(N.IndelParams(3, 0, 100, 0, 0, 100001, 100001, 0)), b"params.ploidy must be 1 or 2"),
                    (C.byref(N.IndelParams(0, 0, 100, 0, 0, 100001, 100001, 0)), b"params.ploidy must be 1 or 2"),
                    (C.byref(N.IndelParams(1, 0, 100, 0, 0, 100001, 100001, 0)), b"params.min_gq must be 0..99"),
                    (C.byref(N.IndelParams(1, 0, 99, 0, 0, 100001, 100001, 0)), b"params.indel_centi must be 0..100000"),
                    (C.byref(N.IndelParams(1, 0, 99, 0, 0, 100000, 100001, 0)), b"params.het_centi must be 0..100000"),
                    (C.byref(N.IndelParams(1, 0, 99, 0, 0, 100000, 100000, 0)), b"map is NULL")):
        assert L.dcn_anchor_map_indels_genotype(None, p, 9, 0, 1, None, 0, None, 0, C.byref(n), C.byref(m)) == N.DCN_ERR_ARG
        assert word in L.dcn_last_error(), (word, L.dcn_last_error())
    assert L.dcn_anchor_map_indels_genotype(amap._h, C.byref(prm), 1, 0, LEN1, None, 0, None, 0, None, C.byref(m)) == N.DCN_ERR_ARG
    assert b"n_sites/n_inserted is NULL" in L.dcn_last_error()


def test_capacity_protocol(env):
    """NULLs with capacity 0, a capacity one too small, exact, more: the counts are always complete, and nothing else is
    written until the arrays fit"""
    dcn, O, records, amap, placer = env
    N = dcn._native
    L = N.lib()
    c = gapped_case(dcn, records, seed=74)
    amap.pileup_reset()
    counts, ins, dels = PW.new_counts(records), IW.new_ledger(records), DW.new_ledger(records)
    add(c, amap, placer, O, counts, ins, dels)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    want = DW.fetch_range(dels[0], 0, LEN0)
    total = len(want)
    assert total >= 20

    def fetch(cap, nulls=False):
        items = np.full(max(cap, 1) * 16, 0xAB, np.uint8)
        n = C.c_uint64(12345)
        rc = L.dcn_anchor_map_deletions_fetch(amap._h, 0, 0, LEN0, None if nulls else ptr(items), cap, C.byref(n))
        return rc, items, n.value

    rc, _, n = fetch(0, nulls=True)
    assert rc == N.DCN_ERR_CAPACITY and n == total and str(total).encode() in L.dcn_last_error()
    rc, items, n = fetch(total - 1)
    assert rc == N.DCN_ERR_CAPACITY and n == total and (items == 0xAB).all()
    for cap in (total, total + 3):
        rc, items, n = fetch(cap)
        assert rc == 0 and n == total and DW.deletions_as_tuples(items.view(dcn.DELETION_DTYPE)[:total]) == want
        assert (items[total * 16:] == 0xAB).all()
    rc, _, _ = fetch(total, nulls=True)
    assert rc == N.DCN_ERR_ARG and b"events is NULL" in L.dcn_last_error()

    prm = N.IndelParams(2, 3, 20, 20, 2, 2000, 301, 0)
    want = DW.sites_range(counts[0], ins[0], dels[0], 0, LEN0)
    total, total_bases = len(want), sum(s[2] for s in want if not s[1] & DW.INDEL_DELETION)
    assert total >= 5 and total_bases >= 3 and any(s[1] & DW.INDEL_DELETION for s in want)

    def geno(cap, base_cap, nulls=False, record=0, length=LEN0):
        items, bases = np.full(max(cap, 1) * 48, 0xAB, np.uint8), np.full(max(base_cap, 1), 0xAB, np.uint8)
        n, m = C.c_uint64(12345), C.c_uint64(12345)
        rc = L.dcn_anchor_map_indels_genotype(amap._h, C.byref(prm), record, 0, length, None if nulls else ptr(items), cap, None if nulls else ptr(bases),
                                              base_cap, C.byref(n), C.byref(m))
        return rc, items, bases, n.value, m.value

    rc, _, _, n, m = geno(0, 0, nulls=True)
    assert rc == N.DCN_ERR_CAPACITY and (n, m) == (total, total_bases) and str(total).encode() in L.dcn_last_error()
    for cap, base_cap in ((total - 1, total_bases), (total, total_bases - 1), (total - 1, total_bases - 1)):
        rc, items, bases, n, m = geno(cap, base_cap)
        assert rc == N.DCN_ERR_CAPACITY and (n, m) == (total, total_bases) and (items == 0xAB).all() and (bases == 0xAB).all()
    for cap, base_cap in ((total, total_bases), (total + 3, total_bases + 5)):
        rc, items, bases, n, m = geno(cap, base_cap)
        assert rc == 0 and (n, m) == (total, total_bases)
        assert DW.device_sites(items.view(dcn.INDEL_SITE_DTYPE)[:total], bases[:total_bases].tobytes()) == want
        assert (items[total * 48:] == 0xAB).all() and (bases[total_bases:] == 0xAB).all()
    rc, *_ = geno(total, total_bases, nulls=True)
    assert rc == N.DCN_ERR_ARG and b"is NULL" in L.dcn_last_error()
    # a range without a site: capacity 0 with NULLs succeeds
    amap.pileup_reset()
    rc, _, _, n, m = geno(0, 0, nulls=True)
    assert rc == 0 and (n, m) == (0, 0)

"""The seams of the strand planes (dcn_anchor_map_pileup_keep_strands / _fetch_strands, the strand forms of the pileup kernel in
pileup.hip) and the argument errors of dcn_anchor_map_strand_evidence and dcn_anchor_map_indels_strand that need a map, with
rows written by hand as tests/test_gpu_pileup_qual_seams.py writes its rows: two short records, the second starting mid-word
of the store and of every plane.  Every case runs through dcn_pileup_batch and through dcn_pileup_batch_qual; the counters and
the planes of both records, from their first base to their last, are compared with the models of tests/_pileup_worker.py,
tests/_quality_worker.py and tests/_strand_worker.py.  Every comparison is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _align_worker as AW
import _pileup_worker as PW
import _quality_worker as QW
import _strand_worker as SW
import _verify_worker as VW
from test_gpu_insertions_seams import behind, foreign
from test_gpu_pileup_qual_seams import HIGH, QCase, one_low
from test_gpu_pileup_seams import LEN0, LEN1, make_records, other

pytestmark = pytest.mark.gpu

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_strand_worker.py")
BOTH_CALLS = pytest.mark.parametrize("with_quals", [False, True], ids=["batch", "batch_qual"])


@pytest.fixture(scope="module")
def env(dcn, oracle):
    records = make_records()
    amap = VW.build_map(oracle, dcn, records)
    amap.pileup_enable()
    amap.pileup_keep_insertions()
    amap.pileup_keep_deletions()
    amap.pileup_keep_strands()
    placer = dcn.Placer(amap, max_batch_bases=1 << 21, max_batch_reads=1 << 12)
    yield dcn, oracle, records, amap, placer
    placer.close()
    amap.close()


def pile(c, placer, oracle, rows, reads, quals, with_quals, min_base_qual, **kw):
    if with_quals:
        b, o, q = QW.concat(oracle, reads, quals)
        return placer.pileup_batch(b, o, rows, quals=q, min_base_qual=min_base_qual, qual_offset=c.qual_offset, **kw)
    b, o = oracle.concat_reads(reads)
    return placer.pileup_batch(b, o, rows, **kw)


def run(c, amap, placer, oracle, with_quals, min_base_qual=0, **kw):
    """resets, adds the case's rows, compares the counters and the planes of both records with the models -> (counts, planes,
    [CIGAR text per row])"""
    rows = np.concatenate(c.rows)
    amap.pileup_reset()
    edits, n_added = pile(c, placer, oracle, rows, c.reads, c.quals, with_quals, min_base_qual, **kw)
    counts, planes = PW.new_counts(c.records), SW.new_planes(c.records)
    if with_quals:
        want = QW.pile_rows(counts, None, None, c.reads, c.quals, c.records, rows, min_base_qual=min_base_qual, qual_offset=c.qual_offset, **kw)
        assert SW.pile_planes(planes, c.reads, c.records, rows, quals=c.quals, min_base_qual=min_base_qual, qual_offset=c.qual_offset, **kw) == want[1]
    else:
        want = PW.pile_rows(counts, c.reads, c.records, rows, **kw)
        assert SW.pile_planes(planes, c.reads, c.records, rows, **kw) == want[1]
    assert edits.tolist() == want[0].tolist() and n_added == want[1]
    PW.assert_counts(amap, c.records, counts)
    SW.assert_planes(amap, c.records, planes, counts)
    _, offs, cigar = AW.align_rows(c.reads, c.records, rows, **kw)
    return counts, planes, [AW.cigar_text(cigar[int(offs[i]):int(offs[i + 1])]) for i in range(len(rows))]


@BOTH_CALLS
def test_a_reverse_row_and_a_forward_row_over_the_same_bases(env, with_quals):
    """64 bases with one substitution, forward and reverse, at four offsets of a word, on both records, at the last bases of
    record 0 and the first of record 1 as well: the reverse rows alone reach the planes, each base in its own column"""
    dcn, O, records, amap, placer = env
    c = QCase(dcn, records, 231)
    spots = [(0, 2000), (1, 1000), (0, LEN0 - 64), (1, 0)]
    for R, base in spots:
        for rev in (0, 1, 1):
            for pre in (0, 5, 16, 31):
                T = records[R][base:base + 64]
                c.put(T[:20] + other(T[20:21]) + T[21:], HIGH, R, base, base + 64, rev, pre=pre)
    counts, planes, cigars = run(c, amap, placer, O, with_quals)
    assert set(cigars[1:]) == {"20=1X43="}
    for R, base in spots:
        assert planes[R][base:base + 64].sum(axis=1).tolist() == [8] * 64 == counts[R][base:base + 64, PW.REV].tolist()
        assert counts[R][base:base + 64, :4].sum(axis=1).tolist() == [12] * 64
        x = PW.column(other(records[R][base + 20:base + 21])[0])
        assert int(planes[R][base + 20, x]) == 8 and int(counts[R][base + 20, x]) == 12
    assert sum(int(p.sum()) for p in planes) == 8 * 64 * len(spots)  # nothing anywhere else
    # the forward rows alone: not one add
    c = QCase(dcn, records, 232)
    for R, base in spots:
        c.put(records[R][base:base + 64], HIGH, R, base, base + 64, 0)
    counts, planes, _ = run(c, amap, placer, O, with_quals)
    assert not any(p.any() for p in planes) and not any(int(x[:, PW.REV].sum()) for x in counts)
    assert not amap.pileup_fetch_strands(0).any() and not amap.pileup_fetch_strands(1).any()


@BOTH_CALLS
def test_a_run_longer_than_the_lane_stride(env, with_quals):
    """X, one '=' run of 63, 64, 65 and 130 bases, X, on a reverse row: lane q of the run's second round adds at base 64 + q"""
    dcn, O, records, amap, placer = env
    c = QCase(dcn, records, 233)
    where = []
    for k, ln in enumerate((63, 64, 65, 130)):
        a = 300 + 150 * k
        T = records[1][a:a + ln + 2]
        c.put(other(T[:1]) + T[1:1 + ln] + other(T[1 + ln:]), HIGH, 1, a, a + ln + 2, 1)
        where.append((a, ln))
    counts, planes, cigars = run(c, amap, placer, O, with_quals, max_permille=1000)
    assert cigars[1:] == ["1X%d=1X" % ln for _, ln in where]
    for a, ln in where:
        assert planes[1][a:a + ln + 2].sum(axis=1).tolist() == [1] * (ln + 2)


def runs_row(T0, n_runs, first_x):
    """(S, bases of T) whose alignment has n_runs runs, '=' of three bases and X of one in turn, beginning with an X when
    first_x"""
    S, at = bytearray(), 0
    for r in range(n_runs):
        if (r % 2 == 1) != first_x:
            S += other(T0[at:at + 1])
            at += 1
        else:
            S += T0[at:at + 3]
            at += 3
    return bytes(S), at


@BOTH_CALLS
def test_more_runs_than_a_chunk(env, with_quals):
    """reverse rows of 63, 64, 65 and 129 runs: an X in run 63 (the last of the first chunk) and, in the rows that begin with
    an X, in run 64 (the first of the second chunk, whose (i, j) the first chunk hands on)"""
    dcn, O, records, amap, placer = env
    c = QCase(dcn, records, 234)
    shapes = []
    for n_runs in (63, 64, 65, 129):
        for first_x in (False, True):
            S, n = runs_row(records[0][1000:1400], n_runs, first_x)
            c.put(S, HIGH, 0, 1000, 1000 + n, 1)
            c.put(S, HIGH, 0, 1000, 1000 + n, 0)
            shapes.append((n_runs, first_x, n))
    counts, planes, cigars = run(c, amap, placer, O, with_quals, max_permille=1000)
    assert [len(AW.parse_cigar(x)) for x in cigars[1::2]] == [s[0] for s in shapes]
    for run_index in (63, 64):  # the X of that run, in every reverse row that has one there, is in the plane of the read's letter
        rows_with = 0
        for n_runs, first_x, n in shapes:
            if run_index >= n_runs or (run_index % 2 == 1) == first_x:
                continue
            j = sum(1 if (r % 2 == 1) != first_x else 3 for r in range(run_index))
            col = PW.column(other(records[0][1000 + j:1001 + j])[0])
            rows_with += 1
            assert int(planes[0][1000 + j, col]) >= 1 and int(planes[0][1000 + j, PW.column(records[0][1000 + j])]) < len(shapes)
        assert rows_with == (3 if run_index == 63 else 2)  # (rows of 64, 65 and 129 runs have a run 63; of 65 and 129 a run 64)
    assert planes[0][1000:1003].sum(axis=1).tolist() == [len(shapes)] * 3 == counts[0][1000:1003, PW.REV].tolist()


def test_what_adds_to_no_plane(env):
    """on a reverse row: a base under min_base_qual, an invalid base, a D run and an I run.  The planes do not move at any of
    them, and REV does"""
    dcn, O, records, amap, placer = env
    a = 2500
    T = records[0][a:a + 80]
    ins = foreign(T, 39, 2)
    cases = [(T, one_low(80, 40), "80=", [40]),                                     # a base under the threshold: N
             (T[:40] + b"N" + T[41:], [HIGH] * 80, "40=1X39=", [40]),               # an invalid base: N under X
             (T[:38] + T[40:], [HIGH] * 78, "38=2D40=", [38, 39]),                  # a D run of two
             (behind(T, 39, ins), [HIGH] * 40 + [HIGH, HIGH] + [HIGH] * 40, "40=2I40=", [])]  # an I run of two behind base 39
    for S, q, cigar, silent in cases:
        c = QCase(dcn, records, 235)
        c.put(S, q, 0, a, a + 80, 1)
        counts, planes, cigars = run(c, amap, placer, O, True, min_base_qual=20)
        assert cigars[1] == cigar
        assert counts[0][a:a + 80, PW.REV].tolist() == [1] * 80
        assert planes[0][a:a + 80].sum(axis=1).tolist() == [0 if p in silent else 1 for p in range(80)]
        assert int(planes[0].sum()) == 80 - len(silent) and not planes[1].any()
        if "I" in cigar:
            assert int(counts[0][a + 39, PW.INS]) == 1 and int(planes[0][a + 39].sum()) == 1  # the base in front is counted once
    # the same invalid base, D run and I run without qualities
    for S, q, cigar, silent in cases[1:]:
        c = QCase(dcn, records, 236)
        c.put(S, q, 0, a, a + 80, 1)
        counts, planes, _ = run(c, amap, placer, O, False)
        assert planes[0][a:a + 80].sum(axis=1).tolist() == [0 if p in silent else 1 for p in range(80)]


def mixed_case(dcn, records, seed, n_rows):
    """rows of both strands with substitutions, gaps, low qualities and N on both records"""
    c = QCase(dcn, records, seed)
    for q in range(n_rows):
        R = q % 2
        a = (37 * q) % ((LEN1 if R else LEN0) - 70)
        T = records[R][a:a + 60]
        kind = q % 5
        S = T if kind == 0 else T[:30] + other(T[30:31]) + T[31:] if kind == 1 else T[:20] + T[22:] if kind == 2 else \
            behind(T, 25, foreign(T, 25, 1 + q % 3)) if kind == 3 else T[:10] + b"N" + T[11:]
        c.put(S, c.rng.integers(0, 42, len(S)).tolist(), R, a, a + 60, rev=(q // 2) % 2)
    return c


@BOTH_CALLS
def test_one_batch_cut_into_calls(env, with_quals):
    """1, 2 and 7 calls over the same 140 rows: the same counters and the same planes"""
    dcn, O, records, amap, placer = env
    c = mixed_case(dcn, records, 237, 140)
    rows = np.concatenate(c.rows)
    texts = []
    for batches in (1, 2, 7):
        amap.pileup_reset()
        counts, planes = PW.new_counts(records), SW.new_planes(records)
        cuts = np.linspace(0, len(c.reads), batches + 1).astype(int)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            pile(c, placer, O, rows[lo:hi], c.reads[lo:hi], c.quals[lo:hi], with_quals, 20)
            if with_quals:
                QW.pile_rows(counts, None, None, c.reads[lo:hi], c.quals[lo:hi], records, rows[lo:hi], min_base_qual=20)
                SW.pile_planes(planes, c.reads[lo:hi], records, rows[lo:hi], quals=c.quals[lo:hi], min_base_qual=20)
            else:
                PW.pile_rows(counts, c.reads[lo:hi], records, rows[lo:hi])
                SW.pile_planes(planes, c.reads[lo:hi], records, rows[lo:hi])
        PW.assert_counts(amap, records, counts)
        SW.assert_planes(amap, records, planes, counts)
        texts.append(b"".join(amap.pileup_fetch_strands(R).tobytes() for R in (0, 1)))
    assert texts[0] == texts[1] == texts[2] and any(texts[0])
    # a range of a record, from a base that is no multiple of anything
    got = amap.pileup_fetch_strands(1, 33, 77)
    assert np.array_equal(got, PW.as_u32(planes[1][33:110])) and amap.pileup_fetch_strands(1, LEN1, 0).shape == (0, 4)


def test_the_second_trip_of_the_capped_grid():
    """DCN_GRID_CUS = 1 with 300 rows, in a process of its own: both strand forms of the kernel take the second trip of their
    work loop (tests/_strand_worker.py compares with the models there)"""
    env_ = {k: v for k, v in os.environ.items() if k != "DCN_GRID_CUS"}
    p = subprocess.run([sys.executable, WORKER, "grid"], capture_output=True, text=True, timeout=300, env=dict(env_, DCN_GRID_CUS="1"))
    assert p.returncode == 0, p.stderr[-2000:]
    line = [x for x in p.stdout.splitlines() if x.startswith("strand grid ")]
    assert len(line) == 1 and len(line[0]) > 1000


def test_the_switch_is_refused_once_a_row_has_added(env, dcn, oracle):
    """rule S1: DCN_ERR_ARG with the reset named once a row has added, accepted after a reset; keep(False) always; fetch is
    refused on a map without planes"""
    _, O, records, _, _ = env
    amap = VW.build_map(O, dcn, records)
    with pytest.raises(dcn.DeaconHipError, match="the map has no pileup"):
        amap.pileup_keep_strands()
    amap.pileup_enable()
    with pytest.raises(dcn.DeaconHipError, match=r"the map keeps no strand planes \(dcn_anchor_map_pileup_keep_strands\)"):
        amap.pileup_fetch_strands(0)
    placer = dcn.Placer(amap, max_batch_bases=1 << 18, max_batch_reads=1 << 10)
    c = QCase(dcn, records, 238)
    c.put(records[0][100:160], HIGH, 0, 100, 160, 1)
    rows = np.concatenate(c.rows)
    b, o = O.concat_reads(c.reads)
    amap.pileup_keep_strands()
    amap.pileup_keep_strands()  # (again: nothing changes)
    amap.pileup_keep_strands(False)
    assert placer.pileup_batch(b, o, rows)[1] == 1
    with pytest.raises(dcn.DeaconHipError, match=r"1 rows have added to the pileup since it was enabled or reset.*dcn_anchor_map_pileup_reset first"):
        amap.pileup_keep_strands()
    amap.pileup_keep_strands(False)  # (off stays allowed)
    amap.pileup_reset()
    amap.pileup_keep_strands()
    assert not amap.pileup_fetch_strands(0).any()
    assert placer.pileup_batch(b, o, rows)[1] == 1
    assert amap.pileup_fetch_strands(0, 100, 60).sum(axis=1).tolist() == [1] * 60
    amap.pileup_reset()  # zeroes the planes too
    assert not amap.pileup_fetch_strands(0).any() and not amap.pileup_fetch(0).any()
    amap.pileup_disable()  # frees them: a new pileup has none
    amap.pileup_enable()
    with pytest.raises(dcn.DeaconHipError, match="the map keeps no strand planes"):
        amap.pileup_fetch_strands(0)
    placer.close()
    amap.close()


def test_the_switch_off_changes_nothing(env, dcn, oracle):
    """a map that never heard of planes, one that switched them on and off again, and one that keeps them: the counters, the
    quality sums and both ledgers are the same bytes"""
    _, O, records, _, _ = env
    c = mixed_case(dcn, records, 239, 120)
    rows = np.concatenate(c.rows)
    b, o, q = QW.concat(O, c.reads, c.quals)
    texts = []
    for mode in ("never", "off again", "on"):
        amap = VW.build_map(O, dcn, records)
        amap.pileup_enable()
        amap.pileup_keep_insertions()
        amap.pileup_keep_deletions()
        amap.pileup_keep_qualities()
        if mode != "never":
            amap.pileup_keep_strands()
        if mode == "off again":
            amap.pileup_keep_strands(False)
        placer = dcn.Placer(amap, max_batch_bases=1 << 19, max_batch_reads=1 << 10)
        edits, n_added = placer.pileup_batch(b, o, rows, quals=q, min_base_qual=20)
        parts = [edits.tobytes(), str(n_added).encode()]
        for R in (0, 1):
            ev, eb = amap.insertions_fetch(R)
            parts += [amap.pileup_fetch(R).tobytes(), amap.pileup_fetch_qualities(R).tobytes(), ev.tobytes(), eb, amap.deletions_fetch(R).tobytes()]
        texts.append(b"|".join(parts))
        if mode == "on":
            assert amap.pileup_fetch_strands(0).any()
        placer.close()
        amap.close()
    assert texts[0] == texts[1] == texts[2] and len(texts[0]) > 100_000


# ---- the argument errors that need a map ---------------------------------------------------------------------------------
def test_strand_evidence_argument_errors_in_their_order(env, dcn, oracle):
    _, O, records, amap, _ = env
    N, L = dcn._native, dcn._native.lib()
    bare = VW.build_map(O, dcn, records)
    bare.pileup_enable()
    ok = N.StrandParams(1083, 1, 3, 0)
    Q = N.StrandQuery

    def call(m, p, record, queries, out=True):
        arr = (Q * max(len(queries), 1))(*queries)
        sites = (N.StrandSite * max(len(queries), 1))()
        rc = L.dcn_anchor_map_strand_evidence(m._h, None if p is None else C.byref(p), record, arr if queries else None, len(queries),
                                              sites if out else None)
        return rc, L.dcn_last_error() if rc else b""

    bad_q = Q(LEN0, 2, 4, 0, 1, 2, 0)  # (every field wrong: what comes first is told)
    for m, p, record, queries, word in (
            (bare, None, 9, [bad_q], b"params is NULL"),
            (bare, N.StrandParams(1083, 1, 3, 1), 9, [bad_q], b"params.reserved must be 0"),
            (bare, ok, 9, [bad_q], b"the map keeps no strand planes (dcn_anchor_map_pileup_keep_strands)"),
            (amap, ok, 2, [bad_q], b"strand evidence: record 2 of 2 added"),
            (amap, ok, 0, [Q(5, 0, 0, 2, 0, 0, 0), bad_q], b"query 1: pos %d is past the record's %d bases" % (LEN0, LEN0)),
            (amap, ok, 1, [Q(LEN1, 0, 0, 2, 0, 0, 0)], b"query 0: pos %d is past the record's %d bases" % (LEN1, LEN1)),
            (amap, ok, 0, [Q(5, 2, 4, 0, 1, 2, 0)], b"query 0: kind must be 0 or 1"),
            (amap, ok, 0, [Q(5, 0, 4, 0, 1, 2, 0)], b"query 0: ref_code must be 0..3"),
            (amap, ok, 0, [Q(5, 0, 3, 0, 1, 2, 0)], b"query 0: alt_mask is empty"),
            (amap, ok, 0, [Q(5, 0, 3, 16, 1, 2, 0)], b"query 0: alt_mask has bits above 3"),
            (amap, ok, 0, [Q(5, 0, 3, 9, 1, 2, 0)], b"query 0: alt_mask holds ref_code"),
            (amap, ok, 0, [Q(5, 0, 3, 7, 1, 2, 0)] * 3 + [Q(5, 1, 9, 99, 1, 2, 0)], b"query 3: count_reverse 2 is above count 1"),
            (amap, ok, 0, [Q(5, 1, 0, 0, 2, 2, 7)], b"query 0: reserved must be 0")):
        rc, msg = call(m, p, record, queries)
        assert rc == N.DCN_ERR_ARG and word in msg, (word, msg)
    assert call(amap, ok, 0, [Q(5, 0, 3, 7, 0, 0, 0)], out=False) == (N.DCN_ERR_ARG, b"queries/out is NULL")
    assert call(amap, ok, 0, [], out=False) == (0, b"")            # n_queries = 0: nothing to do
    assert call(amap, ok, 0, [Q(LEN0 - 1, 0, 3, 7, 9, 99, 0), Q(0, 1, 9, 99, 2, 2, 0)])[0] == 0  # (fields of the other kind are not looked at)
    with pytest.raises(dcn.DeaconHipError, match="the map has no pileup"):
        VW.build_map(O, dcn, records).strand_evidence(0, np.zeros(1, dcn.STRAND_QUERY_DTYPE))
    assert len(amap.strand_evidence(0, np.zeros(0, dcn.STRAND_QUERY_DTYPE))) == 0
    bare.close()


def test_indels_strand_argument_errors(env, dcn, oracle):
    _, O, records, amap, _ = env
    N = dcn._native
    site = np.zeros(3, dcn.INDEL_SITE_DTYPE)
    site["pos"], site["len"], site["flags"], site["bases_offset"] = [10, 10, 10], [2, 1, 3], [N.INDEL_FRONT, N.INDEL_DELETION, 0], [0, 2, 2]
    amap.pileup_reset()
    assert amap.indels_strand(0, site, b"ACGTA").tolist() == [0, 0, 0]  # an empty ledger: no event, and the order is I6's
    assert len(amap.indels_strand(0, site[:0])) == 0
    with pytest.raises(dcn.DeaconHipError, match="indels strand: record 2 of 2 added"):
        amap.indels_strand(2, site, b"ACGTA")
    with pytest.raises(dcn.DeaconHipError, match="site 1: the sites are not in rule I6's order"):
        amap.indels_strand(0, site[[1, 0, 2]], b"ACGTA")
    with pytest.raises(dcn.DeaconHipError, match="site 2: the sites are not in rule I6's order"):
        amap.indels_strand(0, site[[0, 1, 1]], b"AC")
    far = site.copy()
    far["pos"][2] = LEN0
    with pytest.raises(dcn.DeaconHipError, match="site 2: pos %d is past the record's %d bases" % (LEN0, LEN0)):
        amap.indels_strand(0, far, b"ACGTA")
    off = site.copy()
    off["bases_offset"][2] = 3
    with pytest.raises(dcn.DeaconHipError, match="site 2: bases_offset 3 is not the 2 inserted bases of the sites in front"):
        amap.indels_strand(0, off, b"ACGTAA")
    with pytest.raises(dcn.DeaconHipError, match="bases is NULL"):
        amap.indels_strand(0, site, b"")
    only_ins = VW.build_map(O, dcn, records)
    with pytest.raises(dcn.DeaconHipError, match="the map has no pileup"):
        only_ins.indels_strand(0, site, b"ACGTA")
    only_ins.pileup_enable()
    only_ins.pileup_keep_insertions()
    with pytest.raises(dcn.DeaconHipError, match=r"site 1: the map keeps no deletion ledger \(dcn_anchor_map_pileup_keep_deletions\)"):
        only_ins.indels_strand(0, site, b"ACGTA")
    assert only_ins.indels_strand(0, site[[0, 2]], b"ACGTA").tolist() == [0, 0]  # it needs no planes, and only the ledgers of its sites
    only_ins.pileup_keep_insertions(False)
    only_ins.pileup_keep_deletions()
    with pytest.raises(dcn.DeaconHipError, match=r"site 0: the map keeps no insertion ledger \(dcn_anchor_map_pileup_keep_insertions\)"):
        only_ins.indels_strand(0, site, b"ACGTA")
    only_ins.close()

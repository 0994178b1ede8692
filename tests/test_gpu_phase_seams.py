"""The seams of dcn_phase_batch, dcn_anchor_map_phase_links / _solve and their kernels (phase.hip), with rows and sites written
by hand as tests/test_gpu_pileup_seams.py writes its rows: the same two short records, the second starting mid-word of the
store.  Every case is a call of a few hundred rows (a thousand copies of one read in one case) whose links, every site of
the list, are compared bit for bit with the model of tests/_phase_worker.py, a walk over the runs one step at a time; the
solve is compared with rule H6 written as a loop.  What a case is about is asserted on the model, not on the device."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _align_worker as AW
import _phase_worker as HW
import _pileup_worker as PW
import _quality_worker as QW
import _verify_worker as VW
from test_gpu_insertions_seams import behind, foreign
from test_gpu_pileup_qual_seams import QCase, runs_row
from test_gpu_pileup_seams import LEN0, LEN1, Case, make_records, other

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_phase_worker.py")
SCAN_BLOCK = int(re.search(r"DCN_PHASE_SCAN_BLOCK = (\d+);", open(os.path.join(ROOT, "deacon-server_amd", "csrc", "dcn_phase.h")).read()).group(1))


@pytest.fixture(scope="module")
def env(dcn, oracle):
    records = make_records()
    amap = VW.build_map(oracle, dcn, records)
    amap.pileup_enable()  # (for the left-align switch, and to show that nothing of it is written)
    amap.pileup_keep_insertions()
    amap.pileup_keep_deletions()
    amap.pileup_keep_qualities()
    amap.pileup_keep_strands()
    placer = dcn.Placer(amap, max_batch_bases=1 << 21, max_batch_reads=1 << 12)
    yield dcn, oracle, records, amap, placer
    placer.close()
    amap.close()


def site(records, R, pos, alt=None):
    """(record, pos, a0, a1): a0 the record's base there, a1 another letter"""
    ref = records[R][pos:pos + 1]
    alt = other(ref) if alt is None else alt
    return (R, pos, PW.column(ref[0]), PW.column(alt[0]))


def alt_at(records, R, a, b, positions, what="alt"):
    """records[R][a:b] with the site's other allele ("alt"), or a letter that is neither ("third"), at the record positions given"""
    s = bytearray(records[R][a:b])
    for p in positions:
        ref = records[R][p:p + 1]
        s[p - a] = (other(ref) if what == "alt" else other(ref, other(ref)))[0]
    return bytes(s)


def run(c, entries, amap, placer, O, quals=False, left_align=False, set_sites=True, row_offsets=None, **kw):
    """sets the list, hands the case's rows in, compares every link and the info with the model -> (links, sites)"""
    dcn = c.dcn
    sites = HW.make_sites(dcn.PHASE_SITE_DTYPE, entries)
    rows = np.concatenate(c.rows)
    if set_sites:
        amap.phase_sites(sites)
    if quals:
        b, o, q = QW.concat(O, c.reads, c.quals)
        kw = dict(kw, quals=q, qual_offset=c.qual_offset)
        model_kw = dict(kw, quals=c.quals)
    else:
        b, o = O.concat_reads(c.reads)
        model_kw = kw
    edits, n_linking = placer.phase_batch(b, o, rows, row_offsets=row_offsets, **kw)
    links = np.zeros((len(sites), 4), np.int64)
    want = HW.link_rows(links, sites, c.reads, c.records, rows, row_offsets=row_offsets, left_align=left_align, **model_kw)
    assert edits.tolist() == want[0].tolist() and n_linking == want[1]
    HW.assert_links(amap, links)
    if set_sites:
        assert amap.phase_info() == (len(sites), want[2], want[1], want[3])
    return links, sites


def test_rows_with_no_one_and_two_sites_and_the_ends_of_the_interval(env):
    """sites at t_origin - 1, t_origin, the interval's last base and the base behind it: a row sees the two inside; rows that
    hold no site, one site, and two; both strands, both records"""
    dcn, O, records, amap, placer = env
    c = Case(dcn, records, 300)
    entries = []
    for R, a in ((0, 1000), (1, 500)):
        entries += [site(records, R, p) for p in (a - 1, a, a + 63, a + 64)]
        for rev in (0, 1):
            c.put(records[R][a:a + 64], R, a, a + 64, rev)                                        # ref, ref
            c.put(alt_at(records, R, a, a + 64, (a, a + 63)), R, a, a + 64, rev)                   # alt, alt
            c.put(alt_at(records, R, a, a + 64, (a + 63,)), R, a, a + 64, rev)                     # ref, alt
            c.put(records[R][a + 1:a + 63], R, a + 1, a + 63, rev)                                 # no site
            c.put(records[R][a:a + 63], R, a, a + 63, rev)                                         # one site
            c.put(records[R][a - 1:a + 1], R, a - 1, a + 1, rev)                                   # two sites, two bases
            c.put(alt_at(records, R, a + 63, a + 65, (a + 64,)), R, a + 63, a + 65, rev)
    links, _ = run(c, entries, amap, placer, O, max_permille=1000)  # (a row of two bases with a substitution)
    for k in (0, 4):  # (the four sites of a record: three links)
        assert links[k].tolist() == [2, 0, 0, 0] and links[k + 1].tolist() == [2, 2, 0, 2] and links[k + 2].tolist() == [0, 2, 0, 0]
    assert not links[3].any() and not links[7].any()  # record 0's last site has no link to record 1's first; the list's last has none


def test_every_run_kind_at_a_site(env):
    """a site on an X whose base is a1, on a base that is neither allele, under a D (no link on either side and no bridge), right
    behind an I, on the first and on the last base of a run"""
    dcn, O, records, amap, placer = env
    c = Case(dcn, records, 301)
    entries = []
    for R, a in ((0, 2500), (1, 600)):
        T = records[R][a:a + 80]
        entries += [site(records, R, p) for p in (a + 10, a + 39, a + 40, a + 41, a + 70)]
        for rev in (0, 1):
            c.put(T, R, a, a + 80, rev)
            c.put(alt_at(records, R, a, a + 80, (a + 40,)), R, a, a + 80, rev)                     # X with a1: the site is a run of its own
            c.put(alt_at(records, R, a, a + 80, (a + 40,), "third"), R, a, a + 80, rev)           # neither allele
            c.put(T[:40] + T[41:], R, a, a + 80, rev)                                              # D over the site
            c.put(behind(T, 39, foreign(T, 39, 2)), R, a, a + 80, rev)                             # the site right behind an I
            c.put(alt_at(records, R, a, a + 80, (a + 38, a + 42), "third"), R, a, a + 80, rev)    # 39 and 41: a run's first and last base
            c.put(alt_at(records, R, a, a + 80, (a + 39, a + 41)), R, a, a + 80, rev)
    links, sites = run(c, entries, amap, placer, O)
    _, offs, cigar = AW.align_rows(c.reads, c.records, np.concatenate(c.rows))
    texts = [AW.cigar_text(cigar[int(offs[i]):int(offs[i + 1])]) for i in range(1, 8)]
    assert texts == ["80=", "40=1X39=", "40=1X39=", "40=1D39=", "40=2I40=", "38=1X3=1X37=", "39=1X1=1X38="], texts
    assert links[0].sum() == links[3].sum() == links[5].sum() == links[8].sum() == 2 * 7  # seven rows a strand
    # record 0, whose runs are the ones above: the D row and the third-letter row link nothing at 40, on either side
    assert links[1].tolist() == [6, 2, 2, 0] and links[2].tolist() == [6, 2, 2, 0]


def test_strands_and_qualities(env):
    """forward and reverse rows with asymmetric qualities: the byte of S[i] on a reverse row is the read's from the other end;
    quality min - 1 and min at a site; no qualities at all"""
    dcn, O, records, amap, placer = env
    c = QCase(dcn, records, 302)
    entries = []
    for R, a in ((0, 500), (1, 300)):
        entries += [site(records, R, p) for p in (a + 5, a + 20, a + 50)]
        for rev in (0, 1):
            for q5, q20 in ((20, 20), (19, 20), (20, 19), (40, 0)):
                q = [35] * 60
                q[5], q[20] = q5, q20
                c.put(alt_at(records, R, a, a + 60, (a + 20,)), q, R, a, a + 60, rev)
            c.put(records[R][a:a + 60], list(range(60)), R, a, a + 60, rev)  # a ramp: a mirrored index would see site 50 low and site 5 high
    links, _ = run(c, entries, amap, placer, O, quals=True, min_base_qual=20)
    for k in (0, 3):
        assert links[k].tolist() == [0, 2, 0, 0] and links[k + 1].tolist() == [2, 0, 4, 0]  # (5, 20): one row a strand; (20, 50): q20 >= 20 three times, the ramp
    plain = Case(dcn, records, 303)
    plain.reads, plain.rows = c.reads, c.rows
    links, _ = run(plain, entries, amap, placer, O)
    for k in (0, 3):
        assert links[k].tolist() == [2, 8, 0, 0] and links[k + 1].tolist() == [2, 0, 8, 0]


def many_sites_row(records, n_sites, a=2000):
    """a row over record 0 with a site on every second base, the other allele at every third site: more runs than sites"""
    positions = [a + 2 * k for k in range(n_sites)]
    b = positions[-1] + 3
    return [site(records, 0, p) for p in positions], alt_at(records, 0, a, b, positions[::3]), a, b


@pytest.mark.parametrize("n_sites", [63, 64, 65, 129])
def test_the_lane_group_carry(env, n_sites):
    """63, 64, 65 and 129 sites in one row: the pair of sites 63 and 64 is the carry's, and with 129 that of 127 and 128 too"""
    dcn, O, records, amap, placer = env
    c = Case(dcn, records, 304)
    entries, S, a, b = many_sites_row(records, n_sites)
    for rev in (0, 1):
        c.put(S, 0, a, b, rev)
        c.put(records[0][a:b], 0, a, b, rev)
    links, _ = run(c, entries, amap, placer, O, max_permille=1000)
    assert links[:-1].sum(axis=1).tolist() == [4] * (n_sites - 1) and not links[-1].any()
    assert n_sites < 66 or links[62].tolist() != links[63].tolist() != links[64].tolist()  # (the alleles differ along the row: a shifted carry shows)


@pytest.mark.parametrize("n_runs", [63, 64, 65, 129])
def test_the_run_chunk_carry(env, n_runs):
    """rows of 63, 64, 65 and 129 runs with sites in runs 0, 1, 61, 62, 63, 64, 65 and the last (where the row has them): the
    pair of a site in run 63 and one in run 64 lies across two chunks of runs.  With 129 runs a site in every run: both carries"""
    dcn, O, records, amap, placer = env
    c = Case(dcn, records, 305)
    S, n = runs_row(records[0][1000:1400], n_runs)
    start = lambda r: 1000 + (r // 2) * 4 + (3 if r % 2 else 0)  # noqa: E731
    which = range(n_runs) if n_runs == 129 else sorted({r for r in (0, 1, 61, 62, 63, 64, 65, n_runs - 1) if r < n_runs})
    entries = []
    for r in which:
        p = start(r)
        if r % 2:  # an X run: S holds other(T) there; every second of them is a1, the others neither allele
            entries.append(site(records, 0, p, alt=S[p - 1000:p - 999] if r % 4 == 3 or r == 61 else other(records[0][p:p + 1], S[p - 1000:p - 999])))
        else:
            entries.append(site(records, 0, p))
    for rev in (0, 1):
        c.put(S, 0, 1000, 1000 + n, rev)
    links, sites = run(c, entries, amap, placer, O, max_permille=1000)
    _, offs, cigar = AW.align_rows(c.reads, c.records, np.concatenate(c.rows), max_permille=1000)
    assert int(offs[2] - offs[1]) == n_runs
    at = {r: k for k, r in enumerate(which)}
    assert links[at[61]].tolist() == [0, 0, 2, 0]  # runs 61 and 63 hold a1, runs 62 and 64 a0
    assert n_runs < 64 or links[at[62]].tolist() == [0, 2, 0, 0]
    assert n_runs < 65 or links[at[63]].tolist() == [0, 0, 2, 0]


def test_a_thousand_copies(env):
    """1,000 copies of one row: every counter it adds to is 1,000"""
    dcn, O, records, amap, placer = env
    c = Case(dcn, records, 306)
    entries = [site(records, 0, p) for p in (3000, 3050, 3100, 3149)]
    c.reads, c.rows = [alt_at(records, 0, 3000, 3150, (3050,))], [VW.make_row(c.dtype, 0, 0, 0, 150, 3000, 3150)] * 1000
    links, _ = run(c, entries, amap, placer, O, row_offsets=np.array([0, 1000], np.uint64))
    assert links.tolist() == [[0, 1000, 0, 0], [0, 0, 1000, 0], [1000, 0, 0, 0], [0, 0, 0, 0]]
    assert amap.phase_info() == (4, 1000, 1000, 3000)


def test_a_capped_grid_in_a_process_of_its_own(env):
    """DCN_GRID_CUS = 1 with 300 rows (the capped grid of the link kernel takes the second trip of its work loop) in a worker that
    compares with the model; the same links here, on the whole grid"""
    dcn, O, records, amap, placer = env
    env_ = {k: v for k, v in os.environ.items() if k != "DCN_GRID_CUS"}
    p = subprocess.run([sys.executable, WORKER, "grid"], capture_output=True, text=True, timeout=300, env=dict(env_, DCN_GRID_CUS="1"))
    assert p.returncode == 0, p.stderr[-2000:]
    line = [x for x in p.stdout.splitlines() if x.startswith("phase grid ")]
    assert len(line) == 1 and len(line[0]) > 1000
    _, sites, reads, rows = HW.grid_case(dcn)
    amap.phase_sites(sites)
    b, o = O.concat_reads(reads)
    placer.phase_batch(b, o, rows)
    assert "phase grid " + np.ascontiguousarray(amap.phase_links()).tobytes().hex() == line[0]


def test_records_do_not_link(env):
    """the last site of record 0 and the first of record 1, with rows over both ends: no link, and the solve starts a set"""
    dcn, O, records, amap, placer = env
    c = Case(dcn, records, 307)
    entries = [site(records, 0, LEN0 - 40), site(records, 0, LEN0 - 1), site(records, 1, 0), site(records, 1, 30)]
    for rev in (0, 1):
        for _ in range(2):
            c.put(records[0][LEN0 - 80:], 0, LEN0 - 80, LEN0, rev)
            c.put(alt_at(records, 1, 0, 80, (0, 30)), 1, 0, 80, rev)
    links, sites = run(c, entries, amap, placer, O)
    assert links.tolist() == [[4, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 4], [0, 0, 0, 0]]
    got = HW.assert_solve(amap, sites, links)
    assert got["flags"].tolist() == [HW.HEAD | HW.JOINED, 0, HW.HEAD | HW.JOINED, 0] and got["set_index"].tolist() == [0, 0, 1, 1]
    assert got["set_pos"].tolist() == [LEN0 - 40, LEN0 - 40, 0, 0]


def test_the_left_align_switch(env):
    """a site inside a homopolymer that a gap moves across: with the switch on the row's D lies on the repeat's first base, where
    the site is, and the row observes nothing there; with it off the gap lies at the far end and the row observes the base"""
    dcn, O, records, amap, placer = env
    c = Case(dcn, records, 308)
    a, b = 1260, 1410  # (A * 70 at 1300 .. 1370)
    T = records[0][a:b]
    first = 1300 if records[0][1299:1300] != b"A" else 1299
    while records[0][first - 1:first] == b"A":
        first -= 1
    entries = [site(records, 0, 1270), site(records, 0, first), site(records, 0, 1400)]
    for rev in (0, 1):
        c.put(T[:60] + T[61:], 0, a, b, rev)  # one A fewer
    seen = {}
    try:
        for on in (False, True):
            amap.pileup_reset()
            amap.pileup_left_align(on)
            seen[on], _ = run(c, entries, amap, placer, O, left_align=on)
    finally:
        amap.pileup_reset()
        amap.pileup_left_align(False)
    assert seen[False][:2].sum() == 4 and seen[True][:2].sum() == 0, (seen, first)


def test_replacing_the_list_batches_and_cuts(env):
    """replacing the list zeroes the links; two batches in either order and one batch cut in two give the same links"""
    dcn, O, records, amap, placer = env
    _, sites, reads, rows = HW.grid_case(dcn)
    links = np.zeros((len(sites), 4), np.int64)
    HW.link_rows(links, sites, reads, records, rows)

    def batch(lo, hi):
        b, o = O.concat_reads(reads[lo:hi])
        return placer.phase_batch(b, o, rows[lo:hi])[1]

    amap.phase_sites(sites)
    whole = batch(0, 300)
    HW.assert_links(amap, links)
    amap.phase_sites(sites)
    assert not amap.phase_links().any() and amap.phase_info() == (len(sites), 0, 0, 0)
    for order in (((0, 130), (130, 300)), ((130, 300), (0, 130)), ((0, 1), (1, 299), (299, 300))):
        amap.phase_sites(sites)
        assert sum(batch(lo, hi) for lo, hi in order) == whole
        HW.assert_links(amap, links)
    amap.phase_sites(sites[:1])  # a list of one site: nothing to link, nothing launched
    assert batch(0, 300) == 0 and amap.phase_links().tolist() == [[0, 0, 0, 0]]
    amap.phase_sites(None)
    assert amap.phase_info() == (0, 0, 0, 0)
    with pytest.raises(dcn.DeaconHipError, match="the map has no phase sites"):
        batch(0, 10)


def test_the_pileup_is_untouched(env):
    """counters, sums, planes and both ledgers before and after a phase_batch over the rows that filled them"""
    dcn, O, records, amap, placer = env
    _, sites, reads, rows = HW.grid_case(dcn)
    reads, rows = list(reads), rows.copy()
    for q in range(40):  # a base fewer or a base more in the first forty reads: both ledgers hold events
        reads[q] = reads[q][:20] + reads[q][21:] if q % 2 else reads[q][:20] + other(reads[q][19:20], reads[q][20:21]) + reads[q][20:]
        rows["read_end"][q] = len(reads[q])
    quals = QW.random_quals(np.random.default_rng(9), reads)
    b, o, q = QW.concat(O, reads, quals)
    amap.pileup_reset()
    placer.pileup_batch(b, o, rows, quals=q, min_base_qual=10)

    def state():
        return [np.ascontiguousarray(x).tobytes() for R in (0, 1) for x in (amap.pileup_fetch(R), amap.pileup_fetch_qualities(R), amap.pileup_fetch_strands(R))] + \
               [amap.insertions_info(), amap.insertions_fetch(0)[0].tobytes(), amap.insertions_fetch(0)[1], amap.pileup_left_align_info(),
                amap.deletions_info(), amap.deletions_fetch(0).tobytes()]

    before = state()
    assert amap.insertions_info()[0] >= 15 and amap.deletions_info()[0] >= 15
    amap.phase_sites(sites)
    _, n_linking = placer.phase_batch(b, o, rows, quals=q, min_base_qual=10)
    assert n_linking > 100 and state() == before
    amap.pileup_reset()


# ---- the solve ---------------------------------------------------------------------------------------------------------
STEP = 5


def solve_case(dcn, records, kinds):
    """sites every STEP bases of record 0 and, for link s, two rows over its two sites alone: kinds[s] = 0 none, 1 two rows in
    cis, 2 two in trans, 3 one of each (a tie: unjoined with counters), 4 four cis and one trans (joined, minor > 0)"""
    n = len(kinds) + 1
    pos = [10 + STEP * s for s in range(n)]
    assert pos[-1] + 8 < LEN0
    T = records[0]
    alt = [other(T[p:p + 1], T[p - 1:p], T[p + 1:p + 2]) for p in pos]  # (unlike both neighbours: no alignment can shift it)
    entries = [site(records, 0, p, alt=x) for p, x in zip(pos, alt)]
    c = Case(dcn, records, 400)
    for s, kind in enumerate(kinds):
        a, b = pos[s] - 4, pos[s] + STEP + 5  # (the sites in front and behind lie outside)
        trans = T[a:pos[s + 1]] + alt[s + 1] + T[pos[s + 1] + 1:b]
        cis = trans[:4] + alt[s] + trans[5:]
        for S in {0: [], 1: [cis, T[a:b]], 2: [trans, trans], 3: [cis, trans], 4: [cis] * 4 + [trans]}[kind]:
            c.put(S, 0, a, b, s % 2, pre=s % 7)
    return c, entries


def solved(env, kinds, ns):
    dcn, O, records, amap, placer = env
    c, entries = solve_case(dcn, records, kinds)
    rows = np.concatenate(c.rows)
    b, o = O.concat_reads(c.reads)
    all_sites = HW.make_sites(dcn.PHASE_SITE_DTYPE, entries)
    links = np.zeros((len(all_sites), 4), np.int64)
    HW.link_rows(links, all_sites, c.reads, c.records, rows, max_permille=1000)
    for s, kind in enumerate(kinds):  # the model shows what the case is about
        assert HW.decide(links[s]) == {0: (False, 0), 1: (True, 0), 2: (True, 1), 3: (False, 0), 4: (True, 0)}[kind], (s, kind, links[s])
    for n in ns:
        amap.phase_sites(all_sites[:n])
        placer.phase_batch(b, o, rows, max_permille=1000)
        mine = links[:n].copy()
        mine[n - 1] = 0  # (the list's last site has no link)
        HW.assert_links(amap, mine)
        for kw in (dict(), dict(min_reads=3), dict(min_reads=0, max_minor_permille=1000), dict(max_minor_permille=0)):
            HW.assert_solve(amap, all_sites[:n], mine, **kw)
    return links


def test_solve_sizes(env):
    """n = 1, 2, 64, 65, and the scan's workgroup size - 1, + 0 and + 1, over a pattern with every kind of link"""
    rng = np.random.default_rng(41)
    kinds = rng.choice([0, 1, 1, 2, 2, 3, 4], SCAN_BLOCK + 1).tolist()
    solved(env, kinds, (1, 2, 64, 65, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1))


def test_solve_heads_at_the_seams_of_waves_and_workgroups(env):
    """a head at the first and at the last lane of a wave and of a workgroup, in a list of three workgroups and a site"""
    n = 3 * SCAN_BLOCK + 1
    kinds = [1 + s % 2 for s in range(n - 1)]
    for head in (63, 64, 127, 128, SCAN_BLOCK - 1, SCAN_BLOCK, 2 * SCAN_BLOCK - 1, 2 * SCAN_BLOCK, 3 * SCAN_BLOCK):
        kinds[head - 1] = 3 if head % 2 else 0
    solved(env, kinds, (n,))


def test_solve_one_set_over_three_workgroups_all_joined_all_unjoined(env):
    """one set from the first site to the last with alternating relations; then no link joined at all"""
    n = 3 * SCAN_BLOCK + 1
    dcn, O, records, amap, placer = env
    solved(env, [1 + (s % 3 != 0) for s in range(n - 1)], (n,))
    got = amap.phase_solve()
    assert got["set_index"].max() == 0 and got["flags"][0] == HW.HEAD | HW.JOINED and not (got["flags"][1:] & HW.HEAD).any()
    assert 0 < got["hap"].sum() < n
    solved(env, [3 * (s % 2) for s in range(n - 1)], (n,))
    got = amap.phase_solve()
    assert got["set_index"].tolist() == list(range(n)) and (got["flags"] == HW.HEAD).all() and not got["hap"].any()

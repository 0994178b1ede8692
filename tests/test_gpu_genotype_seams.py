"""The seams of dcn_anchor_map_genotype and its kernel (genotype.hip), with rows and qualities written by hand as
tests/test_gpu_pileup_qual_seams.py writes them: whole-read forward and reverse rows of reads that differ from the reference
by isolated substitutions only (and, in one case, one deleted base), so the counters and the sums at every position are
chosen exactly.  Two records, the second beginning mid-word of the store.  What a case wants to hit is asserted on the model
(tests/_genotype_worker.py) first; then gt, gq and every site of both whole records are compared with it.  Exact throughout."""
import numpy as np
import pytest

import _genotype_worker as GW
import _pileup_worker as PW
import _quality_worker as QW
import _verify_worker as VW
from test_gpu_pileup_qual_seams import QCase, run
from test_gpu_pileup_seams import LEN0, LEN1, make_records

pytestmark = pytest.mark.gpu

HALF = 20  # a column's reads cover [p - HALF, p + HALF)
ZERO = dict(min_depth=0, min_gq=0, min_qual=0)


@pytest.fixture(scope="module")
def env(dcn, oracle):
    records = make_records()
    amap = VW.build_map(oracle, dcn, records)
    amap.pileup_enable()
    amap.pileup_keep_insertions()
    amap.pileup_keep_qualities()
    placer = dcn.Placer(amap, max_batch_bases=1 << 22, max_batch_reads=1 << 16)
    yield dcn, oracle, records, amap, placer
    placer.close()
    amap.close()


def alt(records, R, p, k=1):
    """the k-th letter after the reference's at p, cyclically in ACGT (an N counts as A)"""
    return b"ACGT"[(PW.column(records[R][p]) % 4 + k) % 4]


def column(c, R, p, obs, q_else=30):
    """one read per observation over [p - HALF, p + HALF): (k, q) shows the k-th other letter (0: the reference's own) at p
    with quality q; k = None deletes the base.  Strands alternate.  The bases beside p are the reference's at q_else."""
    rec = c.records[R]
    a, b = p - HALF, p + HALF
    for i, (k, q) in enumerate(obs):
        T = bytearray(rec[a:b].upper().replace(b"N", b"A"))
        if k is None:
            S, qs = bytes(T[:HALF] + T[HALF + 1:]), [q_else] * (2 * HALF - 1)
        else:
            T[HALF] = alt(c.records, R, p, k) if k else T[HALF]
            S, qs = bytes(T), [q_else] * HALF + [q] + [q_else] * (HALF - 1)
        c.put(S, qs, R, a, b, rev=i % 2)


def check(env, c, settings, **kw):
    """piles the case up, compares both whole records with the model under every setting -> (counts, sums, {setting index:
    per record (gt, gq, sites by position)})"""
    dcn, O, records, amap, placer = env
    counts, sums, _, _ = run(c, amap, placer, O, **kw)
    out = {}
    for i, s in enumerate(settings):
        out[i] = []
        for R in (0, 1):
            gt, gq, sites = GW.assert_range(amap, counts[R], sums[R], records[R], R, **s)
            out[i].append((gt, gq, {x[0]: x for x in sites}))
    return counts, sums, out


def find(records, R, letter, lo):
    """the first position from lo whose reference base is `letter`"""
    return lo + records[R][lo:].upper().index(letter)


def at(counts, sums, records, R, p, **params):
    return GW.decide(counts[R][p][:4], sums[R][p], PW.column(records[R][p]), **params)


def test_thresholds_of_the_rule(env):
    """D at min_depth and one below; min_depth = 0 at an empty position; GQ at min_gq and one below; QUAL at min_qual and one
    below; a tie for second; on both records"""
    dcn, O, records, amap, placer = env
    c = QCase(dcn, records, 190)
    spots = {}
    for R, base in ((0, 100), (1, 300)):
        spots[R] = dict(d3=base, gq30=base + 100, het=base + 200, empty=base + 300)
        column(c, R, base, [(0, 30)] * 3)
        column(c, R, base + 100, [(0, 30)] * 10)
        column(c, R, base + 200, [(0, 30)] * 5 + [(1, 30)] * 5)
    settings = [dict(min_depth=3, min_gq=0, min_qual=0), dict(min_depth=4, min_gq=0, min_qual=0), ZERO, dict(min_depth=0, min_gq=30, min_qual=0),
                dict(min_depth=0, min_gq=31, min_qual=0), dict(min_depth=0, min_gq=0, min_qual=143), dict(min_depth=0, min_gq=0, min_qual=144), dict(GW.DEFAULTS)]
    counts, sums, got = check(env, c, settings)
    for R in (0, 1):
        s = spots[R]
        assert counts[R][s["d3"]][:4].sum() == 3 and got[0][R][0][s["d3"]] != GW.NONE and got[1][R][0][s["d3"]] == GW.NONE
        assert not counts[R][s["empty"]].any() and got[2][R][0][s["empty"]] == GW.NONE and got[2][R][1][s["empty"]] == 0
        assert got[2][R][1][s["gq30"]] == 30
        assert got[3][R][0][s["gq30"]] != GW.NONE and got[4][R][0][s["gq30"]] == GW.NONE
        d = at(counts, sums, records, R, s["het"])
        assert d["qual"] == 143 and d["gq"] == 99 and sorted(d["costs"])[:3] == [3010, 17385, 17385]  # a tie for second
        assert s["het"] in got[5][R][2] and s["het"] not in got[6][R][2] and s["het"] in got[7][R][2]
        assert got[5][R][2][s["het"]][1] == 143 and got[5][R][2][s["het"]][2] == 10


def test_quotients_and_caps(env):
    """cost differences of 99, 100 and 101 hundredths; PL 254, 255 and capped; GQ 98, 99 and capped"""
    dcn, O, records, amap, placer = env
    c = QCase(dcn, records, 191)
    column(c, 0, 200, [(0, 30)], q_else=0)                 # one base: cost(het with it) = het_centi
    column(c, 0, 300, [(0, 127), (0, 127)], q_else=0)      # Q = 254, 255, 256 with err_centi = 0
    column(c, 0, 400, [(0, 127), (0, 128)], q_else=0)
    column(c, 0, 500, [(0, 128), (0, 128)], q_else=0)
    settings = [dict(ZERO, err_centi=100000, het_centi=h) for h in (99, 100, 101)] + [dict(ZERO, err_centi=0, het_centi=60000)] + \
               [dict(ZERO, err_centi=100000, het_centi=h) for h in (4900, 4950, 5000)]
    counts, sums, got = check(env, c, settings, min_base_qual=0)
    assert [int(got[i][0][1][200]) for i in (0, 1, 2)] == [0, 1, 1]
    hom = PW.column(records[0][200])
    hom = hom * (hom + 1) // 2 + hom
    for i, h in ((0, 0), (1, 1), (2, 1)):
        pl = at(counts, sums, records, 0, 200, **settings[i])["pl"]
        assert sorted(pl)[:4] == [0, h, h, h] and pl[hom] == 0
    assert [sorted(at(counts, sums, records, 0, p, **settings[3])["pl"])[1] for p in (300, 400, 500)] == [254, 255, 255]
    assert [sorted(at(counts, sums, records, 0, p, **settings[3])["costs"])[1] for p in (300, 400, 500)] == [25400, 25500, 25600]
    assert [int(got[i][0][1][300]) for i in (4, 5, 6)] == [98, 99, 99]


def test_ties_and_alleles(env):
    """a tie for best between a homozygote and a heterozygote, both ways round, and between two heterozygotes: the first in
    G3's order wins; three and four alleles; best a heterozygote of two non-reference bases; a reference N; positions that
    only low-quality bases or deletions cover"""
    dcn, O, records, amap, placer = env
    c = QCase(dcn, records, 192)
    tie_a, tie_t = find(records, 0, b"A", 180), find(records, 0, b"T", 230)
    assert tie_a < 225 < tie_t < 280
    column(c, 0, tie_a, [(0, 30)] * 2)                                  # het_centi = 0: x/x ties with every x/y; AA is first
    column(c, 0, tie_t, [(0, 30)] * 2)                                  # ... and AT is in front of TT
    column(c, 0, 300, [(0, 30), (1, 30), (2, 30)])                      # three alleles, one each: three heterozygotes tie
    column(c, 0, 400, [(0, 30), (1, 30), (2, 30), (3, 30)] * 2)         # four alleles
    column(c, 0, 500, [(1, 30)] * 5 + [(2, 30)] * 5)                    # 1/2
    column(c, 0, 600, [(0, 3)] * 4)                                     # low quality only: N
    column(c, 0, 700, [(None, 0)] * 4)                                  # deletions only
    column(c, 1, 101, [(0, 30)] * 6 + [(1, 30)] * 6)                    # over the reference's NNN (100 .. 102)
    settings = [dict(ZERO, het_centi=0), dict(ZERO), dict(GW.DEFAULTS), dict(GW.DEFAULTS, ploidy=1), dict(ZERO, ploidy=1)]
    counts, sums, got = check(env, c, settings)
    names = GW.names(2)
    for p, letter, want in ((tie_a, "A", "AA"), (tie_t, "T", "AT")):
        d = at(counts, sums, records, 0, p, **settings[0])
        assert d["costs"].count(0) == 4 and d["gq"] == 0  # x/x and the three heterozygotes with x
        assert names[d["best"]] == want and int(got[0][0][0][p]) == d["best"] == min(g for g, nm in enumerate(names) if letter in nm)
    d = at(counts, sums, records, 0, 300, **settings[1])
    assert sorted(d["costs"])[0] == sorted(d["costs"])[2] < sorted(d["costs"])[3] and d["gq"] == 0
    assert d["best"] == min(g for g, cost in enumerate(d["costs"]) if cost == min(d["costs"])) and len(set(names[d["best"]])) == 2
    assert (counts[0][300][:4] > 0).sum() == 3 and (counts[0][400][:4] > 0).sum() == 4
    s = got[2][0][2][500]
    assert len(set(names[s[4]])) == 2 and "ACGT"[s[6]] not in names[s[4]] and s[3][s[6]] == 0
    p_del = 680 + int(np.argmax(counts[0][680:720, PW.DEL]))  # (where the alignment puts the missing base of a run of equal ones)
    for p, col in ((600, PW.N), (p_del, PW.DEL)):
        assert counts[0][p][col] == 4 and counts[0][p][:4].sum() == 0
        assert all(got[i][0][0][p] == GW.NONE and got[i][0][1][p] == 0 for i in range(5))
    for p in (100, 101, 102):
        assert counts[1][p][:4].sum() == 12 and all(p not in got[i][1][2] for i in range(5))
        assert all(got[i][1][0][p] != GW.NONE for i in (0, 1, 2, 4))  # (settings[3]: six of each is a tie at ploidy 1, GQ 0)
    assert 103 not in got[1][1][2] and 99 not in got[1][1][2]


def dense(c, R, a, n_tiles, tile=50):
    """five reads per tile of `tile` bases, read i with a substitution at every fifth base from i: one read of five differs at
    every position, so with het_centi = 0 every position is a heterozygous site"""
    rec = c.records[R]
    for t in range(n_tiles):
        lo = a + t * tile
        for i in range(5):
            S = bytearray(rec[lo:lo + tile].upper().replace(b"N", b"A"))
            for p in range(i, tile, 5):
                S[p] = alt(c.records, R, lo + p)
            c.put(bytes(S), 30, R, lo, lo + tile, rev=(t + i) % 2)


def assert_slice(amap, whole, R, start, n, **params):
    """a range on the device against the slice of the model's whole record -> the device's sites"""
    gt, gq, by_pos = whole
    got_gt, got_gq, sites = amap.genotype(R, start, n, **params)
    assert np.array_equal(got_gt, gt[start:start + n]) and np.array_equal(got_gq, gq[start:start + n]), (R, start, n)
    got = GW.device_sites(sites)
    assert got == [by_pos[p] for p in range(start, start + n) if p in by_pos], (R, start, n)
    return got


LENGTHS = [1, 2, 3, 4, 5, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049]


def test_geometry_of_the_kernel(env):
    """a stretch in which every position is a site (capacity = n), beside stretches without one: ranges whose first store
    base is 0, 1, 2, 3 mod 4 on both records, lengths 1 .. 5 and around one and two workgroups' positions of either form of
    the kernel (256 and 1,024 per workgroup), so that sites lie on both sides of every lane group and workgroup; no site at
    all; the last positions of one record and the first of the next"""
    dcn, O, records, amap, placer = env
    c = QCase(dcn, records, 193)
    dense(c, 0, 1400, 50)               # [1400, 3900) of record 0, which begins at store base 0
    dense(c, 0, LEN0 - 50, 1)           # its last 50 bases
    dense(c, 1, 0, 31)                  # [0, 1550) of record 1, which begins at store base 3989 (1 mod 4), without its NNN stretch
    every = dict(ZERO, het_centi=0)
    counts, sums, got = check(env, c, [every, dict(GW.DEFAULTS, min_qual=10 ** 6)], max_permille=1000)
    # (all but a few: where two substitutions five bases apart align as well with a gap on each side, the alignment takes the gaps)
    planted = set(range(1400, 3900)) | set(range(LEN0 - 50, LEN0))
    assert set(got[0][0][2]) <= planted and len(planted - set(got[0][0][2])) <= 8 and not got[1][0][2] and not got[1][1][2]
    assert len(set(range(0, 1550)) - {100, 101, 102} - set(got[0][1][2])) <= 8
    run_start = run_len = 0  # the longest stretch of record 0 in which the model has a site at every position
    for p in sorted(got[0][0][2]):
        q = p
        while q + 1 in got[0][0][2]:
            q += 1
        if q - p + 1 > run_len:
            run_start, run_len = p, q - p + 1
    assert run_len >= 1030
    for n in (1023, 1024, 1025, run_len):
        for shift in range(4):
            if shift + n <= run_len:
                assert len(assert_slice(amap, got[0][0], 0, run_start + shift, n, **every)) == n  # every position of the range: capacity = n
    for R, first in ((0, 1400), (1, 0)):
        for shift in range(4):
            for n in LENGTHS:
                if first + shift + n <= len(records[R]):
                    assert_slice(amap, got[0][R], R, first + shift, n, **every)
    # ranges that begin in the stretch without sites and end in the dense one, and the other way round
    for start, n in ((1400 - 256, 512), (1400 - 1023, 1024), (1400 - 1024, 1025), (3900 - 5, 10), (3900 - 1024, 1030), (0, LEN0)):
        assert_slice(amap, got[0][0], 0, start, n, **every)
    # the last positions of record 0 and the first of record 1 do not see each other
    for n in (1, 2, 3, 4, 5):
        a, b = assert_slice(amap, got[0][0], 0, LEN0 - n, n, **every), assert_slice(amap, got[0][1], 1, 0, n, **every)
        assert len(a) >= n - 1 and len(b) >= n - 1
    assert LEN1 > 1550


def test_costs_past_32_bits_on_the_device(env):
    """50,000 copies of one 32-base read at q = 93 with err_centi = 100000: n * err_centi = 5 * 10^9 and 100 * Q = 4.65 * 10^8
    hundredths per column; the model just multiplies (Python integers)"""
    dcn, O, records, amap, placer = env
    T = bytearray(records[0][3000:3032])
    T[16] = alt(records, 0, 3016)
    copies = 50_000
    reads, quals = [bytes(T)], [bytes([126]) * 32]
    rows = np.concatenate([VW.make_row(dcn.filter.PLACEMENT_DTYPE, 0, 0, 0, 32, 3000, 3032)] * copies)
    b, o, q = QW.concat(O, reads, quals)
    amap.pileup_reset()
    edits, n_added = placer.pileup_batch(b, o, rows, row_offsets=np.array([0, copies], np.uint64), quals=q, min_base_qual=20)
    assert n_added == copies and (edits == 1).all()
    counts, sums = PW.new_counts(records), QW.new_sums(records)
    QW.pile_rows(counts, sums, None, reads, quals, records, rows[:1], min_base_qual=20)
    counts, sums = [x * copies for x in counts], [x * copies for x in sums]
    PW.assert_counts(amap, records, counts)
    QW.assert_sums(amap, records, sums)
    for ploidy in (1, 2):
        prm = dict(GW.DEFAULTS, ploidy=ploidy, err_centi=100000, het_centi=100000)
        _, _, sites = GW.assert_range(amap, counts[0], sums[0], records[0], 0, **prm)
        assert [s[0] for s in sites] == [3016] and sites[0][1] == (100 * 93 * copies + 100000 * copies) // 100 > 2 ** 25
        d = at(counts, sums, records, 0, 3016, **prm)
        assert max(d["costs"]) > 2 ** 32 and d["pl"].count(255) == len(d["costs"]) - 1 and d["gq"] == 99

"""Strand evidence against the model of tests/_strand_worker.py.

The random batch of tests/test_gpu_genotype_differential.py (a diploid sample, rows of both strands, qualities uniform in
0 .. 41 at min_base_qual 20): the planes, and dcn_anchor_map_strand_evidence at every genotype site at both ploidies.  A column
of 1,100 short rows at one position, nearly all of one strand, so that rule S5 shifts the table on the device, beside a small
balanced group.  The deletion and insertion sites of the indel seam cases (tests/test_gpu_indels_seams.py) with carriers of
both strands, of one strand, with a losing allele beside the winner and with two alleles of one length:
dcn_anchor_map_indels_strand and the evidence of every site.  Every comparison is exact.

What the inputs are good for is asserted from the model, so that a run cannot pass vacuously: the column holds a site with
both flags and one with DCN_STRAND_BIAS alone, the small group one with DCN_STRAND_ONE_SIDED alone and one with neither; the
random batch holds sites with neither; the indel cases hold a one-sided site and sites with neither."""
import numpy as np
import pytest

import _genotype_worker as GW
import _indel_worker as DW
import _insertion_worker as IW
import _pileup_worker as PW
import _quality_worker as QW
import _strand_worker as SW
import _verify_worker as VW
from conftest import revcomp
from test_gpu_genotype_differential import N_READS, make_sample
from test_gpu_indels_seams import LOOSE, genotype_case, one_run, without
from test_gpu_pileup_seams import LEN1, Case, make_records, other

pytestmark = pytest.mark.gpu

BIAS, ONE_SIDED = SW.STRAND_BIAS, SW.STRAND_ONE_SIDED
PARAMS = [dict(SW.DEFAULTS), dict(max_sb_centi=300, min_alt_strand=3, min_strand_depth=5), dict(max_sb_centi=0, min_alt_strand=0, min_strand_depth=0)]


def test_the_random_batch_of_the_genotype_test(dcn, oracle):
    record, reads, quals, rows = make_sample(1932, dcn.filter.PLACEMENT_DTYPE)
    assert 100 < int(rows["reverse"].sum()) < 300  # rows of both strands
    counts, sums, planes = PW.new_counts([record]), QW.new_sums([record]), SW.new_planes([record])
    want_edits, want_added = QW.pile_rows(counts, sums, None, reads, quals, [record], rows, min_base_qual=20)
    assert SW.pile_planes(planes, reads, [record], rows, quals=quals, min_base_qual=20) == want_added == N_READS
    assert int(planes[0].sum()) > 10_000 and int(counts[0][:, PW.N].sum()) > 10_000  # (bases under the threshold: in N, in no plane)
    amap = VW.build_map(oracle, dcn, [record])
    amap.pileup_enable()
    amap.pileup_keep_qualities()
    amap.pileup_keep_strands()
    placer = dcn.Placer(amap, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    try:
        for lo, hi in ((0, 37), (37, 290), (290, N_READS)):
            b, o, q = QW.concat(oracle, reads[lo:hi], quals[lo:hi])
            edits, n_added = placer.pileup_batch(b, o, rows[lo:hi], quals=q, min_base_qual=20)
            assert edits.tolist() == want_edits[lo:hi].tolist() and n_added == hi - lo
        PW.assert_counts(amap, [record], counts)
        QW.assert_sums(amap, [record], sums)
        SW.assert_planes(amap, [record], planes, counts)
        seen = set()
        for ploidy in (2, 1):
            _, _, sites = GW.genotype_range(counts[0], sums[0], record, **dict(GW.DEFAULTS, ploidy=ploidy))
            assert len(sites) >= 40
            queries = SW.genotype_queries([(s[0], s[4], s[6]) for s in sites], ploidy)
            for params in PARAMS:
                want = SW.assert_evidence(amap, 0, counts[0], planes[0], queries, **params)
                if params == SW.DEFAULTS:
                    seen |= {w[4] for w in want}
            # the convenience: genotype, the queries from gt and ref_code, the evidence
            gt, gq, dsites, ev = amap.genotype_strand(0, ploidy=ploidy)
            assert GW.device_sites(dsites) == sites and SW.device_evidence(ev) == SW.assert_evidence(amap, 0, counts[0], planes[0], queries)
            assert [tuple(int(x) for x in q) for q in amap.strand_queries_of_genotypes(dsites, ploidy)[["pos", "kind", "ref_code", "alt_mask", "count", "count_reverse"]].tolist()] == queries
        print("flags seen at the sample's sites:", sorted(seen))
        assert 0 in seen
    finally:
        placer.close()
        amap.close()


def test_a_column_of_1100_rows_shifts_the_table(dcn, oracle):
    """1,060 reverse and 40 forward rows over one 40-base interval, and 43 rows over another: tables with a cell above 1023
    (rule S5's shift on the device), and one site of each combination of the flags"""
    records = make_records()
    a, b = 3000, 3200
    T, U = records[0][a:a + 40], records[0][b:b + 30]

    def alt(X, *at):
        s = bytearray(X)
        for p in at:
            s[p] = other(X[p:p + 1])[0]
        return bytes(s)

    # (S, reverse, copies, first base, last base)
    groups = [(T, 1, 1030, a, a + 40), (alt(T, 12), 1, 30, a, a + 40), (alt(T, 5), 0, 30, a, a + 40), (alt(T, 5, 12), 0, 10, a, a + 40),
              (U, 0, 15, b, b + 30), (alt(U, 10), 0, 3, b, b + 30), (alt(U, 20), 0, 5, b, b + 30), (U, 1, 15, b, b + 30), (alt(U, 20), 1, 5, b, b + 30)]
    dtype = dcn.filter.PLACEMENT_DTYPE
    reads = [revcomp(S) if rev else S for S, rev, _, _, _ in groups]
    rows = np.concatenate([VW.make_row(dtype, 0, rev, 0, len(S), lo, hi) for S, rev, n, lo, hi in groups for _ in range(n)])
    row_offsets = np.concatenate([[0], np.cumsum([g[2] for g in groups])]).astype(np.uint64)
    assert len(rows) == 1100 + 43
    counts, planes = PW.new_counts(records), SW.new_planes(records)
    want_edits, want_added = PW.pile_rows(counts, reads, records, rows, row_offsets=row_offsets)
    assert SW.pile_planes(planes, reads, records, rows, row_offsets=row_offsets) == want_added == len(rows)

    def query(X, base, p):
        return (base + p, 0, PW.column(X[p]), 1 << PW.column(other(X[p:p + 1])[0]), 0, 0)
    queries = [query(T, a, 5), query(T, a, 12), query(U, b, 10), query(U, b, 20), query(T, a, 30)]
    want = [SW.evidence(counts[0], planes[0], q) for q in queries]
    # the tables, the scores and the flags as worked out by hand (tests/cpp/strand_rule_test.cpp's arithmetic):
    # (0, 1060, 40, 0) >> 1 = (0, 530, 20, 0): 100 * 550 = 55000; (30, 1030, 10, 30) >> 1 = (15, 515, 5, 15):
    # 100 * 550 * 2350^2 / (530 * 20 * 20 * 530) = 2703; (20, 20, 3, 0): 100 * 43 * 3600 / (40 * 3 * 23 * 20) = 280;
    # (18, 15, 5, 5): 100 * 43 * 225 / (33 * 10 * 23 * 20) = 6; no ALT read at all: score 0, and the allele is on neither strand
    assert [(w[2], w[3], w[4]) for w in want] == [([0, 1060, 40, 0], 55000, BIAS | ONE_SIDED), ([30, 1030, 10, 30], 2703, BIAS),
                                                  ([20, 20, 3, 0], 280, ONE_SIDED), ([18, 15, 5, 5], 6, 0), ([40, 1060, 0, 0], 0, ONE_SIDED)]
    amap = VW.build_map(oracle, dcn, records)
    amap.pileup_enable()
    amap.pileup_keep_strands()
    placer = dcn.Placer(amap, max_batch_bases=1 << 18, max_batch_reads=1 << 10)
    try:
        bb, oo = oracle.concat_reads(reads)
        edits, n_added = placer.pileup_batch(bb, oo, rows, row_offsets=row_offsets)
        assert edits.tolist() == want_edits.tolist() and n_added == want_added
        PW.assert_counts(amap, records, counts)
        SW.assert_planes(amap, records, planes, counts)
        for params in PARAMS + [dict(max_sb_centi=2703), dict(max_sb_centi=2704), dict(min_alt_strand=11), dict(min_strand_depth=41)]:
            got = SW.assert_evidence(amap, 0, counts[0], planes[0], queries, **params)
            if params == dict(max_sb_centi=2704):
                assert got[1][4] == 0
            if params == dict(min_strand_depth=41):
                assert got[0][4] == BIAS  # 40 forward reads no longer cover the site
        # every ALT set at one position, and a record whose planes lie behind record 0's
        assert len(SW.assert_evidence(amap, 0, counts[0], planes[0], [(a + 12, 0, r, m, 0, 0) for r in range(4) for m in range(1, 16) if not m & (1 << r)])) == 28
        assert SW.assert_evidence(amap, 1, counts[1], planes[1], [(LEN1 - 1, 0, 0, 14, 0, 0), (0, 1, 0, 0, 0, 0)])[0][2] == [0, 0, 0, 0]
    finally:
        placer.close()
        amap.close()


def indel_cases(env):
    """[(name, Case)] on the records of the seam tests"""
    dcn, O, records, amap, placer = env
    cases = [("both strands", genotype_case(env, 8, 4, 4))]  # carriers 0 .. 3, strands alternating: two of each
    T = records[1][:600]
    c = Case(dcn, records, 241)
    for q in range(12):  # a deletion carried by forward rows alone, an insertion by reverse rows alone, under two-stranded coverage
        s = [T[p:p + 1] for p in range(600)]
        if q in (0, 2, 4, 6):
            s[300] = s[301] = b""
        if q in (1, 3, 5):
            s[330] += other(T[330:331], T[331:332]) * 2
        c.put(b"".join(s), 1, 0, 600, rev=q % 2)
    cases.append(("one strand", c))
    c = Case(dcn, records, 242)  # two lengths at one start: only the winner's events count
    V = records[0][3000:3150]
    at = next(x for x in range(40, 110) if one_run(V, x, 2) and one_run(V, x, 3))
    for S, strands in ((without(V, at, 2), (0, 0, 0, 1, 1)), (without(V, at, 3), (0, 1, 1, 1))):
        for rev in strands:
            c.put(S, 0, 3000, 3150, rev=rev)
    cases.append(("two lengths", c))
    c = Case(dcn, records, 243)  # two insertions of one length behind one base: the bases tell the winner's events from the others
    W = records[0][3200:3300]
    x, y = other(W[50:51], W[51:52]), next(bytes([z]) for z in b"ACGT" if bytes([z]) not in (W[50:51].upper(), W[51:52].upper(), other(W[50:51], W[51:52])))
    for ins, strands in ((x * 2, (0, 0, 1, 1, 1)), (y * 2, (1, 1, 1, 1))):
        for rev in strands:
            c.put(W[:51] + ins + W[51:], 0, 3200, 3300, rev=rev)
    cases.append(("two alleles", c))
    c = Case(dcn, records, 244)  # a front insertion and one behind the first base, on both strands
    x, y = other(W[:1]), other(W[:1], W[1:2])
    for q in range(8):
        c.put(x * 2 + W[:1] + y + W[1:], 0, 3200, 3300, rev=(q % 4 == 0))
    cases.append(("front and behind", c))
    return cases


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


def test_the_indel_sites_of_the_seam_cases(env):
    dcn, O, records, amap, placer = env
    seen, reverse_counts = set(), {}
    for name, c in indel_cases(env):
        rows = np.concatenate(c.rows)
        bb, oo = O.concat_reads(c.reads)
        amap.pileup_reset()
        edits, n_added = placer.pileup_batch(bb, oo, rows, max_permille=1000)
        counts, ins, dels, planes = PW.new_counts(records), IW.new_ledger(records), DW.new_ledger(records), SW.new_planes(records)
        want_edits, want_added = DW.pile_rows(counts, ins, dels, c.reads, records, rows, max_permille=1000)
        assert edits.tolist() == want_edits.tolist() and n_added == want_added
        assert SW.pile_planes(planes, c.reads, records, rows, max_permille=1000) == want_added
        PW.assert_counts(amap, records, counts)
        SW.assert_planes(amap, records, planes, counts)
        for R in (0, 1):
            for settings in (DW.DEFAULTS, LOOSE):
                want_sites = DW.assert_sites(amap, counts[R], ins[R], dels[R], R, length=len(records[R]), **settings)
                sites, bases = amap.indels_genotype(R, **settings)
                got = amap.indels_strand(R, sites, bases)
                want = [SW.count_reverse(ins[R], dels[R], s) for s in want_sites]
                assert got.tolist() == want, (name, R, got.tolist(), want)
                queries = [(s[0], 1, 0, 0, s[6], r) for s, r in zip(want_sites, want)]
                ev = SW.assert_evidence(amap, R, counts[R], planes[R], queries)
                for params in PARAMS[1:]:
                    SW.assert_evidence(amap, R, counts[R], planes[R], queries, **params)
                for s, r, e in zip(want_sites, want, ev):
                    assert e[0] == e[1] == [0] * 4 and e[2][2] + e[2][3] == s[6] and e[2][3] == r
                    assert e[2][0] + e[2][1] == s[5] - s[6]  # the first row: every read there that does not carry the allele (I2's o)
                if settings is LOOSE:
                    reverse_counts[name] = reverse_counts.get(name, []) + [(s[0], s[1], s[2], s[6], r) for s, r in zip(want_sites, want)]
                    seen |= {e[4] for e in ev}
                    dsites, dbases, dev = amap.indels_genotype_strand(R, **settings)
                    assert dsites.tobytes() == sites.tobytes() and dbases == bases and SW.device_evidence(dev) == ev
    # the inputs, from the model: carriers of both strands, of one strand, a loser beside the winner, two alleles of one length
    assert reverse_counts["both strands"] == [(300, DW.INDEL_DELETION, 2, 4, 2), (330, 0, 2, 4, 2)]
    assert reverse_counts["one strand"] == [(300, DW.INDEL_DELETION, 2, 4, 0), (330, 0, 2, 3, 3)]
    assert [x[2:] for x in reverse_counts["two lengths"]] == [(2, 5, 2)]       # (the 3-base allele's three reverse events are not counted)
    assert [x[1:] for x in reverse_counts["two alleles"]] == [(0, 2, 5, 3)]    # (nor the other insertion's four)
    assert [x[1:] for x in reverse_counts["front and behind"]] == [(0, 1, 8, 2)]
    print("flags seen at the indel sites:", sorted(seen))
    assert 0 in seen and any(f & ONE_SIDED for f in seen)

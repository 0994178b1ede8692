"""dcn_anchor_map_genotype / AnchorMap.genotype on the rows the placement calls return, against the model of
tests/_genotype_worker.py (a loop over genotypes and a loop over columns per cost, on the counts and sums of the CPU pile-up of
tests/_quality_worker.py, never the device's): a diploid sample over two records at (k, w) = (31, 15) and (31, 1).  Two
haplotypes per record differ from the reference by planted substitutions, some on both and some on one; one haplotype has a
deletion, and the second record a run of N.  The reads are drawn half and half with random qualities, placed by place_batch,
carried over the flanks by extend_batch and piled up by pileup_batch(quals=...).  gt, gq and every field of every site, over
whole records, sub-ranges and n = 0, both ploidies, three parameter sets; how batches are cut; reset and refill; the capacity
protocol; the errors that need a device; optional outputs; and that nothing else moves.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import _genotype_worker as GW
import _insertion_worker as IW
import _pileup_worker as PW
import _quality_worker as QW
import _verify_worker as VW
from conftest import random_reads, revcomp

pytestmark = pytest.mark.gpu

CASES = [(31, 15), (31, 1)]
PARAMS = [dict(GW.DEFAULTS), dict(min_depth=0, min_gq=0, min_qual=0, err_centi=477, het_centi=301),
          dict(min_depth=8, min_gq=45, min_qual=60, err_centi=1000, het_centi=150)]
BOTH = {0: (97, 211, 380, 522), 1: (60, 333)}      # substitutions on both haplotypes, per record
ONE = {0: (40, 150, 290, 451, 600), 1: (120, 250, 410)}  # ... on one, alternating between the two
MIN_BASE_QUAL = 20


def other(base):
    return next(x for x in b"ACGT" if x != base)


def make_sample():
    rng = np.random.default_rng(1901)
    records = [random_reads(rng, 1, 701, 701)[0], bytearray(random_reads(rng, 1, 523, 523)[0])]
    records[1][200:205] = b"NNNNN"
    records[1] = bytes(records[1])
    haps = []
    for R, rec in enumerate(records):
        pair = [bytearray(rec.replace(b"N", b"A")), bytearray(rec.replace(b"N", b"A"))]
        for p in BOTH[R]:
            pair[0][p] = pair[1][p] = other(rec[p])
        for i, p in enumerate(ONE[R]):
            pair[i % 2][p] = other(rec[p])
        a = bytes(pair[0])
        haps.append((a[:560] + a[562:] if R == 0 else a, bytes(pair[1])))  # a deletion of two bases on one haplotype of record 0
    reads = []
    for R in range(2):
        for i in range(140 if R == 0 else 110):
            h = haps[R][i % 2]
            s = int(rng.integers(0, len(h) - 150))
            reads.append(revcomp(h[s:s + 150]) if rng.random() < 0.5 else h[s:s + 150])
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    return records, reads, QW.random_quals(rng, reads, lo=5, hi=41)


@pytest.fixture(scope="module")
def built(dcn, oracle):
    records, reads, quals = make_sample()
    b, o, q = QW.concat(oracle, reads, quals)
    out = {}
    for k, w in CASES:
        amap = VW.build_map(oracle, dcn, records, k, w)
        amap.pileup_enable()
        amap.pileup_keep_insertions()
        amap.pileup_keep_qualities()
        placer = dcn.Placer(amap, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
        rows, _ = placer.extend_batch(b, o, placer.place_batch(b, o))
        edits, n_added = placer.pileup_batch(b, o, rows, quals=q, min_base_qual=MIN_BASE_QUAL)
        counts, sums = PW.new_counts(records), QW.new_sums(records)
        want_edits, want_added = QW.pile_rows(counts, sums, None, reads, quals, records, rows, min_base_qual=MIN_BASE_QUAL)
        assert edits.tolist() == want_edits.tolist() and n_added == want_added > 200
        out[(k, w)] = (amap, placer, rows, counts, sums)
    yield records, reads, quals, (b, o, q), out
    for amap, placer, *_ in out.values():
        placer.close()
        amap.close()


@pytest.mark.parametrize("ploidy", [2, 1])
@pytest.mark.parametrize("k,w", CASES)
def test_whole_records_and_ranges_against_the_model(built, k, w, ploidy):
    records, _, _, _, maps = built
    amap, _, _, counts, sums = maps[(k, w)]
    seen = set()
    for i, params in enumerate(PARAMS):
        for R, rec in enumerate(records):
            gt, gq, sites = GW.assert_range(amap, counts[R], sums[R], rec, R, ploidy=ploidy, **{k_: v for k_, v in params.items() if k_ != "ploidy"})
            if i == 0:  # the model alone finds what was planted: the test would show nothing on an empty pile-up
                at = {s[0]: s for s in sites}
                found_both, found_one = [p for p in BOTH[R] if p in at], [p for p in ONE[R] if p in at]
                assert len(found_both) >= len(BOTH[R]) - 1 and (ploidy == 1 or len(found_one) >= len(ONE[R]) - 2), (R, sorted(at))  # (a haploid rule calls no heterozygote)
                if ploidy == 2:
                    names = GW.names(2)
                    assert all(len(set(names[at[p][4]])) == 1 for p in found_both) and all(len(set(names[at[p][4]])) == 2 for p in found_one)
                assert (gt != GW.NONE).sum() > len(rec) // 2 and (gq >= 30).any() and (gq < 20).any()
                if R == 1:
                    assert all(not (200 <= s[0] < 205) for s in sites)  # the reference's N: genotyped, never a site
            seen.update(int(x) for x in gt)
    assert len(seen) >= (6 if ploidy == 2 else 4)
    p = {k_: v for k_, v in PARAMS[1].items()}
    for R, start, n in ((0, 1, 700), (0, 3, 5), (0, 255, 258), (0, 700, 1), (1, 0, 1), (1, 198, 9), (1, 2, 511), (1, 7, 0), (0, 701, 0), (1, 523, 0)):
        gt, gq, sites = GW.assert_range(amap, counts[R], sums[R], records[R], R, start, n, ploidy=ploidy, **p)
        assert len(gt) == n and all(start <= s[0] < start + n for s in sites)


def genotype_bytes(amap, n_records=2):
    out = []
    for R in range(n_records):
        for ploidy in (1, 2):
            gt, gq, sites = amap.genotype(R, ploidy=ploidy)
            out.append((gt.tobytes(), gq.tobytes(), sites.tobytes()))
    return out


def test_cuts_and_a_refill_do_not_matter(built, dcn, oracle):
    records, reads, quals, (b, o, q), maps = built
    amap, placer, rows, counts, sums = maps[(31, 15)]
    whole = genotype_bytes(amap)
    assert sum(len(x[2]) for x in whole) > 8 * 48
    for cuts in ((0, 1, 50, len(reads)), (0, 33, 34, len(reads)), (0, 170, 249, len(reads))):
        amap.pileup_reset()
        gt, gq, sites = amap.genotype(0)
        assert (gt == GW.NONE).all() and not gq.any() and len(sites) == 0  # an empty pile-up calls nothing
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            cb, co, cq = QW.concat(oracle, reads[lo:hi], quals[lo:hi])
            placer.pileup_batch(cb, co, rows[lo:hi], quals=cq, min_base_qual=MIN_BASE_QUAL)
        assert genotype_bytes(amap) == whole


def raw_call(dcn, amap, R, start, n, gt, gq, sites, capacity, n_sites, **params):
    N = dcn._native
    prm = dict(GW.DEFAULTS, **params)
    p = N.GenotypeParams(prm["ploidy"], prm["min_depth"], prm["min_gq"], prm["min_qual"], prm["err_centi"], prm["het_centi"], (C.c_uint32 * 2)(0, 0))
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = N.lib().dcn_anchor_map_genotype(amap._h, C.byref(p), R, start, n, ptr(gt), ptr(gq), ptr(sites), capacity, n_sites)
    return rc, (N.lib().dcn_last_error() or b"").decode()


def test_capacity_protocol_and_optional_outputs(built, dcn):
    records, _, _, _, maps = built
    amap, _, _, counts, sums = maps[(31, 15)]
    N = dcn._native
    want_gt, want_gq, want_sites = GW.genotype_range(counts[0], sums[0], records[0], **GW.DEFAULTS)
    total = len(want_sites)
    assert total > 4
    n = len(records[0])
    n_sites = C.c_uint64(12345)
    # NULL with capacity 0 asks for the count: gt and gq are complete
    gt, gq = np.full(n, 7, np.uint8), np.full(n, 7, np.uint8)
    rc, msg = raw_call(dcn, amap, 0, 0, n, gt, gq, None, 0, C.byref(n_sites))
    assert rc == N.DCN_ERR_CAPACITY and n_sites.value == total and "call again with that capacity" in msg
    assert np.array_equal(gt, want_gt) and np.array_equal(gq, want_gq)
    # one short: the same, and the guard-filled site buffer is untouched
    gt[:], gq[:] = 7, 7
    sites = np.full(total * 48 + 48, 0xEE, np.uint8)
    rc, msg = raw_call(dcn, amap, 0, 0, n, gt, gq, sites, total - 1, C.byref(n_sites))
    assert rc == N.DCN_ERR_CAPACITY and n_sites.value == total and (sites == 0xEE).all()
    assert np.array_equal(gt, want_gt) and np.array_equal(gq, want_gq)
    # exactly enough: the sites, and nothing behind them
    rc, msg = raw_call(dcn, amap, 0, 0, n, gt, gq, sites, total, C.byref(n_sites))
    assert rc == N.DCN_OK and n_sites.value == total and (sites[total * 48:] == 0xEE).all()
    assert GW.device_sites(sites[:total * 48].view(dcn.GENOTYPE_SITE_DTYPE)) == want_sites
    # gt or gq NULL, or both
    for use_gt, use_gq in ((True, False), (False, True), (False, False)):
        gt[:], gq[:], sites[:] = 7, 7, 0xEE
        rc, msg = raw_call(dcn, amap, 0, 0, n, gt if use_gt else None, gq if use_gq else None, sites, total, C.byref(n_sites))
        assert rc == N.DCN_OK and n_sites.value == total, msg
        assert np.array_equal(gt, want_gt) == use_gt and np.array_equal(gq, want_gq) == use_gq
        assert (gt == 7).all() != use_gt and (gq == 7).all() != use_gq
        assert GW.device_sites(sites[:total * 48].view(dcn.GENOTYPE_SITE_DTYPE)) == want_sites
    # a range without a site takes NULL sites; n = 0 writes n_sites = 0 and nothing else
    rc, msg = raw_call(dcn, amap, 0, 0, 30, None, None, None, 0, C.byref(n_sites))
    assert rc == N.DCN_OK and n_sites.value == 0 and not any(s[0] < 30 for s in want_sites)
    n_sites.value = 99
    gt[:] = 7
    rc, msg = raw_call(dcn, amap, 0, 5, 0, gt, None, None, 0, C.byref(n_sites))
    assert rc == N.DCN_OK and n_sites.value == 0 and (gt == 7).all()
    # sites there are, capacity enough, and no buffer
    rc, msg = raw_call(dcn, amap, 0, 0, n, None, None, None, total, C.byref(n_sites))
    assert rc == N.DCN_ERR_ARG and "sites is NULL" in msg


def test_errors_that_need_a_device(built, dcn, oracle):
    records, _, _, _, maps = built
    amap = maps[(31, 15)][0]
    N = dcn._native
    n_sites = C.c_uint64(77)
    bare = VW.build_map(oracle, dcn, records)
    rc, msg = raw_call(dcn, bare, 0, 0, 10, None, None, None, 0, C.byref(n_sites))
    assert rc == N.DCN_ERR_ARG and "the map has no pileup (dcn_anchor_map_pileup_enable)" in msg
    bare.pileup_enable()
    rc, msg = raw_call(dcn, bare, 0, 0, 10, None, None, None, 0, C.byref(n_sites))
    assert rc == N.DCN_ERR_ARG and "the map keeps no quality sums (dcn_anchor_map_pileup_keep_qualities)" in msg
    with pytest.raises(dcn.DeaconHipError) as e:
        bare.genotype(0)
    assert e.value.code == N.DCN_ERR_ARG and "keeps no quality sums" in e.value.message
    # the parameter checks come before the map's
    rc, msg = raw_call(dcn, bare, 0, 0, 10, None, None, None, 0, C.byref(n_sites), ploidy=3)
    assert rc == N.DCN_ERR_ARG and "params.ploidy must be 1 or 2" in msg
    bare.close()
    # the range, with dcn_anchor_map_fetch's words
    for R, start, n in ((2, 0, 1), (0, 702, 0), (0, 0, 702), (1, 500, 24), (0, 700, 2)):
        rc, msg = raw_call(dcn, amap, R, start, n, None, None, None, 0, C.byref(n_sites))
        with pytest.raises(dcn.DeaconHipError) as e:
            amap.fetch(R, start, n)
        assert rc == N.DCN_ERR_ARG and msg.split(": ", 1)[1] == e.value.message.split(": ", 1)[1] and msg.startswith("genotype: "), (msg, e.value.message)
    assert n_sites.value == 77  # (nothing is written by a refused call)
    rc, msg = raw_call(dcn, amap, 0, 0, 10, None, None, None, 0, None)
    assert rc == N.DCN_ERR_ARG and "n_sites is NULL" in msg
    rc, msg = raw_call(dcn, amap, 0, 0, 0, None, None, None, 0, None)  # (behind the range, in front of n = 0)
    assert rc == N.DCN_ERR_ARG and "n_sites is NULL" in msg


def test_nothing_else_moves(built, dcn):
    records, _, _, _, maps = built
    amap = maps[(31, 1)][0]

    def everything():
        out = []
        for R in range(2):
            calls, pos, info = amap.pileup_call(R)
            alleles, ins = amap.insertions_call(R)
            out += [calls, pos.tobytes(), info.tobytes(), alleles.tobytes(), ins, amap.consensus(R), amap.consensus(R, fill_ref=True),
                    amap.pileup_fetch(R).tobytes(), amap.pileup_fetch_qualities(R).tobytes(), amap.insertions_fetch(R)[0].tobytes()]
        return out

    before = everything()
    for R in range(2):
        for ploidy in (1, 2):
            amap.genotype(R, ploidy=ploidy)
            amap.genotype(R, 3, 100, ploidy=ploidy, min_depth=0, min_gq=0, min_qual=0)
    assert everything() == before

"""Phase against the model of tests/_phase_worker.py and against the truth, on rows that the placement calls return: a small
diploid, two haplotypes of one 20 kbp reference that differ at 60 SNVs, read at 150 and at 2,000 bases with substitutions and
indels on both strands, through Placer (place_split_batch, extend_batch, the quality pile-up), AnchorMap.genotype for the
heterozygous SNV sites, then phase_sites, phase_batch over the same rows and phase_solve.  The links are the model's bit for
bit, the solve is rule H6 written as a loop, and every set's hap vector is the truth or its complement.

What the input is good for is asserted on the model, computed on the CPU, so that a run cannot pass vacuously: a set of at
least three sites, an unjoined link (the SNVs leave 3,000 bases free in the middle, which no read spans) and a link with
minor > 0 (one read switches haplotype between two sites, among a dozen that do not)."""
import numpy as np
import pytest

import _phase_worker as HW
import _pileup_worker as PW
import _quality_worker as QW
import _verify_worker as VW
from conftest import random_reads, revcomp

pytestmark = pytest.mark.gpu

LEN, N_SNV, SEED = 20_000, 60, 2501
LETTERS = b"ACGT"


def diploid():
    """-> (reference, [(pos, ref column, alt column, which haplotype carries alt)], the two haplotypes)"""
    rng = np.random.default_rng(SEED)
    ref = random_reads(rng, 1, LEN, LEN)[0]
    pos = set()
    while len(pos) < N_SNV:
        p = int(rng.integers(200, LEN - 200))
        if not 8500 <= p < 11500 and all(abs(p - q) >= 25 for q in pos):
            pos.add(p)
    snvs, haps = [], [bytearray(ref), bytearray(ref)]
    for p in sorted(pos):
        r = PW.column(ref[p])
        a = (r + int(rng.integers(1, 4))) % 4
        h = int(rng.integers(0, 2))
        haps[h][p] = LETTERS[a]
        snvs.append((p, r, a, h))
    return ref, snvs, [bytes(h) for h in haps]


def sample(haps, snvs):
    rng = np.random.default_rng(SEED + 1)
    reads = []
    for ln, count, rate in ((2000, 70, 0.003), (150, 700, 0.003)):
        for q in range(count):
            at = int(rng.integers(0, LEN - ln))
            s = VW.mutate_mixed(rng, haps[q % 2][at:at + ln], rate)
            reads.append(revcomp(s) if (q // 2) % 2 else s)
    # a dozen clean reads of each haplotype over the first two SNVs, and one that begins on haplotype 0 and ends on haplotype 1
    a, b = snvs[0][0], snvs[1][0]
    lo, mid = max(0, a - 600), (a + b) // 2
    for q in range(12):
        reads.append(haps[q % 2][lo + 10 * q:b + 400 + 10 * q])
    reads.append(haps[0][lo:mid] + haps[1][mid:b + 500])
    return reads


@pytest.fixture(scope="module")
def phased(dcn, oracle):
    ref, snvs, haps = diploid()
    reads = sample(haps, snvs)
    quals = QW.random_quals(np.random.default_rng(SEED + 2), reads, lo=15, hi=41)
    amap = VW.build_map(oracle, dcn, [ref])
    amap.pileup_enable()
    amap.pileup_keep_qualities()
    placer = dcn.Placer(amap, max_batch_bases=1 << 21, max_batch_reads=1 << 12)
    b, o, q = QW.concat(oracle, reads, quals)
    po, srows, _ = placer.place_split_batch(b, o, max_placements=2)
    xrows, _ = placer.extend_batch(b, o, srows, row_offsets=po)
    _, n_added = placer.pileup_batch(b, o, xrows, row_offsets=po, quals=q, min_base_qual=20)
    assert n_added > 600
    _, _, gsites = amap.genotype(0)
    het = [(0, int(s["pos"]), a0, a1) for s in gsites for a0, a1 in [tuple(PW.column(x) for x in dcn.GENOTYPES[int(s["gt"])].encode())] if a0 != a1]
    sites = HW.make_sites(dcn.PHASE_SITE_DTYPE, het)
    amap.phase_sites(sites)
    edits, n_linking = placer.phase_batch(b, o, xrows, row_offsets=po, quals=q, min_base_qual=20)
    links = np.zeros((len(sites), 4), np.int64)
    want = HW.link_rows(links, sites, reads, [ref], xrows, row_offsets=po, quals=quals, min_base_qual=20)
    yield dcn, amap, snvs, sites, links, (edits, n_linking), want
    placer.close()
    amap.close()


def test_the_genotype_finds_the_sites(phased):
    dcn, amap, snvs, sites, links, got, want = phased
    truth = {p: (min(r, a), max(r, a)) for p, r, a, _ in snvs}
    found = {int(s["pos"]): (int(s["a0"]), int(s["a1"])) for s in sites}
    assert len(set(found) & set(truth)) >= 50 and all(found[p] == truth[p] for p in found if p in truth)
    # (a false heterozygous site, from read errors that agree, splits a set and no more, rule H10: the truth check below looks
    # at the true sites of every set; how many there are is no property of the phase)
    print("true sites found", len(set(found) & set(truth)), "of", len(truth), "false sites", len(set(found) - set(truth)))


def test_links_equal_the_model(phased):
    dcn, amap, snvs, sites, links, got, want = phased
    assert got[0].tolist() == want[0].tolist() and got[1] == want[1] >= 13  # (the thirteen reads built over the first two SNVs link, at the least)
    HW.assert_links(amap, links)
    assert amap.phase_info() == (len(sites), want[2], want[1], want[3])


def test_sets_equal_the_model_and_the_truth(phased):
    dcn, amap, snvs, sites, links, got, want = phased
    model = HW.solve(sites, links)
    minor = [min(int(n[0]) + int(n[3]), int(n[1]) + int(n[2])) for n in links]
    sizes = np.bincount([m[1] for m in model])
    # what the committed seed is good for, on the model
    assert sizes.max() >= 3 and any(not m[3] & HW.JOINED for m in model[:-1]) and any(x > 0 and m[3] & HW.JOINED for x, m in zip(minor, model))
    print("sites", len(sites), "sets of two or more", int((sizes >= 2).sum()), "largest", int(sizes.max()), "links with minor > 0", sum(x > 0 for x in minor))
    res = HW.assert_solve(amap, sites, links)
    carrier = {p: (r, a, h) for p, r, a, h in snvs}
    checked = 0
    for k in range(len(sizes)):
        members = [s for s in range(len(sites)) if int(res["set_index"][s]) == k and int(sites["pos"][s]) in carrier]
        if sizes[k] < 2 or len(members) < 2:
            continue
        # the allele index (0: a0, 1: a1) that haplotype 0 of the truth carries at each site of the set
        t = []
        for s in members:
            r, a, h = carrier[int(sites["pos"][s])]
            on_hap0 = a if h == 0 else r
            t.append(0 if on_hap0 == int(sites["a0"][s]) else 1)
        hap = [int(res["hap"][s]) for s in members]
        assert hap == t or hap == [1 - x for x in t], (k, hap, t)
        checked += len(members)
    assert checked >= 40
    for kw in (dict(min_reads=1, max_minor_permille=1000), dict(min_reads=5, max_minor_permille=50)):
        HW.assert_solve(amap, sites, links, **kw)

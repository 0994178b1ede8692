"""The model of tests/test_genotype_abi.py and tests/test_gpu_genotype*.py.

THE DEFINITION OF A GENOTYPE (include/deacon_hip.h), written as it reads: a loop over the genotypes of rule G3 and, per
cost, a loop over the four columns that asks whether the column is one of the genotype's alleles.  Python integers, so
nothing can overflow; no total-minus-own shortcut, no ten named scalars.  Nothing here is shared with csrc/dcn_genotype.h.
The counts and sums it is given come from the CPU pile-up of tests/_pileup_worker.py and tests/_quality_worker.py, never from
the device."""
import numpy as np

import _pileup_worker as PW

NONE = 255
DEFAULTS = dict(ploidy=2, min_depth=3, min_gq=20, min_qual=20, err_centi=477, het_centi=301)
LETTERS = "ACGT"


def genotypes(ploidy):
    """rule G3's order: index y (y + 1) / 2 + x at ploidy 2"""
    if ploidy == 1:
        return [(x,) for x in range(4)]
    out = [(x, y) for y in range(4) for x in range(y + 1)]
    assert all(out[y * (y + 1) // 2 + x] == (x, y) for x, y in out)
    return out


def names(ploidy):
    return ["".join(LETTERS[a] for a in g) for g in genotypes(ploidy)]


def costs(n, Q, ploidy=2, err_centi=477, het_centi=301):
    """rules G2 and G3"""
    M = [100 * int(Q[c]) + err_centi * int(n[c]) for c in range(4)]
    out = []
    for g in genotypes(ploidy):
        cost = 0
        for c in range(4):
            if c not in g:
                cost += M[c]
        if len(set(g)) == 2:
            cost += het_centi * (int(n[g[0]]) + int(n[g[1]]))
        out.append(cost)
    return out


def decide(n, Q, ref_column, ploidy=2, min_depth=3, min_gq=20, min_qual=20, err_centi=477, het_centi=301):
    """rules G4 - G7 at one position; ref_column above 3: an invalid reference base
    -> dict(best, gt, gq, qual, site, pl (ten entries), costs)"""
    cost = costs(n, Q, ploidy, err_centi, het_centi)
    best = min(range(len(cost)), key=lambda g: (cost[g], g))
    second = min(cost[g] for g in range(len(cost)) if g != best)
    gq = min(99, (second - cost[best]) // 100)
    pl = [min(255, (c - cost[best]) // 100) for c in cost] + [0] * (10 - len(cost))
    ref_valid = ref_column <= 3
    ref_gt = genotypes(ploidy).index((ref_column,) * ploidy) if ref_valid else None
    qual = min(2 ** 32 - 1, (cost[ref_gt] - cost[best]) // 100) if ref_valid else 0
    D = sum(int(x) for x in n[:4])
    called = D >= max(1, min_depth) and gq >= min_gq
    site = called and ref_valid and best != ref_gt and qual >= min_qual
    return dict(best=best, gt=best if called else NONE, gq=gq, qual=qual, site=bool(site), pl=pl, costs=cost)


def site_tuple(pos, d, counts8, ref_column):
    """a site as plain Python: (pos, qual, depth, ad, gt, gq, ref_code, pl)"""
    return (int(pos), d["qual"], sum(int(x) for x in counts8[:6]) & 0xFFFFFFFF, tuple(int(x) for x in counts8[:4]), d["gt"], d["gq"],
            int(ref_column), tuple(d["pl"]))


def genotype_range(counts, sums, record, start=0, n=None, **params):
    """counts[len(record), 8] and sums[len(record), 4] of one record -> (gt uint8[n], gq uint8[n], [site tuples])"""
    n = len(record) - start if n is None else n
    gt, gq, sites = np.zeros(n, np.uint8), np.zeros(n, np.uint8), []
    for q in range(n):
        p = start + q
        ref_column = PW.column(record[p])
        d = decide(counts[p][:4], sums[p], ref_column, **params)
        gt[q], gq[q] = d["gt"], d["gq"]
        if d["site"]:
            sites.append(site_tuple(p, d, counts[p], ref_column))
    return gt, gq, sites


def device_sites(sites):
    """the structured array of AnchorMap.genotype as site tuples; the reserved bytes must be 0"""
    assert not sites["reserved0"].any() and not sites["reserved1"].any()
    return [(int(s["pos"]), int(s["qual"]), int(s["depth"]), tuple(int(x) for x in s["ad"]), int(s["gt"]), int(s["gq"]), int(s["ref_code"]),
             tuple(int(x) for x in s["pl"])) for s in sites]


def assert_range(amap, counts, sums, record_bytes, R, start=0, n=None, **params):
    """AnchorMap.genotype over a range against the model, the first difference named -> the model's (gt, gq, sites)"""
    want = genotype_range(counts, sums, record_bytes, start, n, **params)
    gt, gq, sites = amap.genotype(R, start, n, **params)
    assert gt.dtype == gq.dtype == np.uint8 and len(gt) == len(gq) == len(want[0])
    for name, g, w in (("gt", gt, want[0]), ("gq", gq, want[1])):
        if not np.array_equal(g, w):
            q = int(np.flatnonzero(g != w)[0])
            raise AssertionError((name, "record", R, "position", start + q, "got", int(g[q]), "want", int(w[q]), params))
    got = device_sites(sites)
    if got != want[2]:
        k = next((i for i, (a, b) in enumerate(zip(got, want[2])) if a != b), min(len(got), len(want[2])))
        raise AssertionError(("site", k, "of", len(got), len(want[2]), "got", got[k:k + 1], "want", want[2][k:k + 1], params))
    return want


# ---- VCF ---------------------------------------------------------------------------------------------------------------
VCF_FIXED = ['##INFO=<ID=DP,Number=1,Type=Integer,Description="Depth: reads with a base, an N or a deletion at the position">',
             '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
             '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype quality: phred gap to the second best genotype, at most 99">',
             '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Bases A, C, G, T of at least the minimum base quality">',
             '##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Such bases per allele">',
             '##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Phred-scaled genotype likelihoods, at most 255">']


def vcf_header(version, contigs, sample="sample"):
    """contigs: [(name, length)] in the reference's order"""
    lines = ["##fileformat=VCFv4.2", "##source=deacon-hip " + version]
    lines += ["##contig=<ID=%s,length=%d>" % (name, length) for name, length in contigs]
    lines += VCF_FIXED
    lines.append("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + sample)
    return lines


def vcf_line(name, site, ploidy):
    pos, qual, depth, ad, gt, gq, ref_code, pl = site
    g = genotypes(ploidy)[gt]
    alleles = [ref_code] + sorted(set(g) - {ref_code})
    index = sorted(alleles.index(a) for a in g)
    if ploidy == 1:
        pls = [pl[a] for a in alleles]
    else:
        order = genotypes(2)
        pls = [pl[order.index(tuple(sorted((alleles[i], alleles[j]))))] for j in range(len(alleles)) for i in range(j + 1)]
    sample = ":".join(["/".join(map(str, index)), str(gq), str(sum(ad)), ",".join(str(ad[a]) for a in alleles), ",".join(map(str, pls))])
    return "\t".join([name, str(pos + 1), ".", LETTERS[ref_code], ",".join(LETTERS[a] for a in alleles[1:]), str(qual), "PASS", "DP=%d" % depth,
                      "GT:GQ:DP:AD:PL", sample])


def vcf_text(version, names_, records, sites_per_record, ploidy=2, sample="sample"):
    """the whole file: header, then one line per site in record order and position order"""
    lines = vcf_header(version, [(nm, len(rec)) for nm, rec in zip(names_, records)], sample)
    for nm, sites in zip(names_, sites_per_record):
        lines += [vcf_line(nm, s, ploidy) for s in sites]
    return "\n".join(lines) + "\n"

// dcn_genotype.h -- what the host and the device share of a genotype (THE DEFINITION OF A GENOTYPE, include/deacon_hip.h):
// the costs of rules G2 and G3 and the decision of rules G4 - G7 at one position, from the four base counters and the
// four quality sums (kernel in genotype.hip, the C ABI in genotype_api.hip).  Plain integer arithmetic, no floating point,
// no division but the quotients by 100 of G4 and G5: compiles for the host alone (tests/cpp/genotype_rule_test.cpp), as
// dcn_pileup.h does.  Nothing here is indexed by a runtime value: the ten costs are ten scalars and every pl[] index is a
// constant, so that a lane keeps them in registers.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DCN_GENO_FN __host__ __device__ inline
#else
#define DCN_GENO_FN inline
#endif

constexpr uint32_t DCN_GENO_NONE = 255;       // DCN_GENOTYPE_NONE of the public header, which tests/cpp does not include
constexpr uint32_t DCN_GENO_REF_INVALID = 4;  // any reference column above T (dcn_pile_column gives DCN_PILE_N = 4)
constexpr uint32_t DCN_GENO_GENOTYPES = 10;

// the fields of dcn_genotype_params that the rule reads (the API has checked them)
struct dcn_geno_params {
    uint32_t ploidy, min_depth, min_gq, min_qual, err_centi, het_centi;
};

struct dcn_geno_result {
    uint32_t gt;   // G6: the best genotype's index in G3's order, or DCN_GENO_NONE when the position is not called
    uint32_t gq;   // G4, called or not
    uint32_t qual; // G5
    uint32_t site; // G7: 0 or 1
    uint32_t best; // G4's best, called or not (a site's gt equals it)
};

// one step of the search for the smallest and the second smallest cost, in G3's order: the first smallest wins
#define DCN_GENO_STEP(G, COST)              \
    if ((COST) < best_cost) {               \
        second = best_cost;                 \
        best_cost = (COST);                 \
        best = (G);                         \
    } else if ((COST) < second) {           \
        second = (COST);                    \
    }

// min(cap, diff / 100) for cap < 2^32 / 100, with a 32-bit quotient: diff / 100 >= cap exactly when diff >= 100 cap
DCN_GENO_FN uint32_t dcn_geno_centi_capped(uint64_t diff, uint32_t cap) {
    const uint64_t top = (uint64_t)cap * 100u + 99u;
    return (uint32_t)(diff < top ? diff : top) / 100u;
}

// n[A..T], Q[A..T], ref_column = the column of the record's base (above T: invalid) -> the result and pl[0 .. 10)
DCN_GENO_FN dcn_geno_result dcn_genotype_decide(const uint32_t *n, const uint32_t *Q, uint32_t ref_column, const dcn_geno_params &p,
                                                uint8_t *pl) {
    // G2 (widening multiplies: 100 Q + err n < 2^32 * 100100 fits easily)
    const uint64_t mA = 100ull * Q[0] + (uint64_t)p.err_centi * n[0], mC = 100ull * Q[1] + (uint64_t)p.err_centi * n[1];
    const uint64_t mG = 100ull * Q[2] + (uint64_t)p.err_centi * n[2], mT = 100ull * Q[3] + (uint64_t)p.err_centi * n[3];
    const uint64_t all = mA + mC + mG + mT;
    // G3: a homozygote pays for every other column, a heterozygote for the other two and het_centi per base of its own
    const uint64_t hA = all - mA, hC = all - mC, hG = all - mG, hT = all - mT;
    const uint64_t het = p.het_centi;
    const bool diploid = p.ploidy == 2;
    const uint64_t absent = UINT64_MAX; // a genotype the ploidy does not have: never the best, never the second
    uint64_t c0, c1, c2, c3, c4, c5, c6, c7, c8, c9;
    if (diploid) {
        c0 = hA;
        c1 = hA - mC + het * ((uint64_t)n[0] + n[1]); // AC
        c2 = hC;
        c3 = hA - mG + het * ((uint64_t)n[0] + n[2]); // AG
        c4 = hC - mG + het * ((uint64_t)n[1] + n[2]); // CG
        c5 = hG;
        c6 = hA - mT + het * ((uint64_t)n[0] + n[3]); // AT
        c7 = hC - mT + het * ((uint64_t)n[1] + n[3]); // CT
        c8 = hG - mT + het * ((uint64_t)n[2] + n[3]); // GT
        c9 = hT;
    } else {
        c0 = hA, c1 = hC, c2 = hG, c3 = hT;
        c4 = c5 = c6 = c7 = c8 = c9 = absent;
    }
    // G4
    uint64_t best_cost = c0, second = absent;
    uint32_t best = 0;
    DCN_GENO_STEP(1u, c1)
    DCN_GENO_STEP(2u, c2)
    DCN_GENO_STEP(3u, c3)
    DCN_GENO_STEP(4u, c4)
    DCN_GENO_STEP(5u, c5)
    DCN_GENO_STEP(6u, c6)
    DCN_GENO_STEP(7u, c7)
    DCN_GENO_STEP(8u, c8)
    DCN_GENO_STEP(9u, c9)
    dcn_geno_result r;
    r.best = best;
    r.gq = dcn_geno_centi_capped(second - best_cost, 99u);
    pl[0] = (uint8_t)dcn_geno_centi_capped(c0 - best_cost, 255u);
    pl[1] = (uint8_t)dcn_geno_centi_capped(c1 - best_cost, 255u);
    pl[2] = (uint8_t)dcn_geno_centi_capped(c2 - best_cost, 255u);
    pl[3] = (uint8_t)dcn_geno_centi_capped(c3 - best_cost, 255u);
    pl[4] = diploid ? (uint8_t)dcn_geno_centi_capped(c4 - best_cost, 255u) : (uint8_t)0;
    pl[5] = diploid ? (uint8_t)dcn_geno_centi_capped(c5 - best_cost, 255u) : (uint8_t)0;
    pl[6] = diploid ? (uint8_t)dcn_geno_centi_capped(c6 - best_cost, 255u) : (uint8_t)0;
    pl[7] = diploid ? (uint8_t)dcn_geno_centi_capped(c7 - best_cost, 255u) : (uint8_t)0;
    pl[8] = diploid ? (uint8_t)dcn_geno_centi_capped(c8 - best_cost, 255u) : (uint8_t)0;
    pl[9] = diploid ? (uint8_t)dcn_geno_centi_capped(c9 - best_cost, 255u) : (uint8_t)0;
    // G5: the homozygote of the record's base is a homozygote's cost at either ploidy
    const bool ref_valid = ref_column <= 3u;
    const uint64_t ref_cost = ref_column == 0 ? hA : ref_column == 1 ? hC : ref_column == 2 ? hG : hT;
    const uint32_t ref_hom = ref_column == 0 ? 0u : ref_column == 1 ? 2u : ref_column == 2 ? 5u : 9u; // x (x + 1) / 2 + x
    const uint32_t ref_gt = diploid ? ref_hom : ref_column;
    const uint64_t qual64 = ref_valid ? (ref_cost - best_cost) / 100u : 0u;
    r.qual = qual64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)qual64;
    // G6, G7
    const uint64_t D = (uint64_t)n[0] + n[1] + n[2] + n[3];
    const bool called = D >= (p.min_depth > 1u ? p.min_depth : 1u) && r.gq >= p.min_gq;
    r.gt = called ? best : DCN_GENO_NONE;
    r.site = called && ref_valid && best != ref_gt && r.qual >= p.min_qual ? 1u : 0u;
    return r;
}

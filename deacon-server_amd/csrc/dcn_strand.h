// dcn_strand.h -- what the host and the device share of strand evidence (THE DEFINITION OF STRAND EVIDENCE, include/deacon_hip.h):
// the tables of rules S3 and S4, the score of rule S5 and the flags of rule S6, from the counters, the reverse planes and a
// ledger's counts (kernels in strand.hip, the C ABI in strand_api.hip; the add of rule S2 is dcn_pileup.h's).  Plain integer
// arithmetic, one 64-bit quotient: compiles for the host alone (tests/cpp/strand_rule_test.cpp), as dcn_genotype.h does.
// Nothing here is indexed by a runtime value: the four columns are four scalars, so that a lane keeps them in registers.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DCN_STRAND_FN __host__ __device__ inline
#else
#define DCN_STRAND_FN inline
#endif

// DCN_STRAND_* of the public header, which tests/cpp does not include
constexpr uint32_t DCN_STRAND_FLAG_BIAS = 1, DCN_STRAND_FLAG_ONE_SIDED = 2;
constexpr uint32_t DCN_STRAND_SB_CAP = 65535;

// the 2 x 2 table: a, b = the reference row forward and reverse; c, d = the allele's row
struct dcn_strand_table {
    uint32_t a, b, c, d;
};

// the fields of dcn_strand_params that the rule reads
struct dcn_strand_prm {
    uint32_t max_sb_centi, min_alt_strand, min_strand_depth;
};

// rule S2: F[c] = n[c] - R[c] (R[c] <= n[c] while nothing has wrapped; 0 otherwise, so that the rule is total)
DCN_STRAND_FN uint32_t dcn_strand_forward(uint32_t n, uint32_t r) { return n >= r ? n - r : 0u; }

// rule S3: n[A..T] and R[A..T] of a position, ref = the record's base (0 .. 3), alt_mask = the set ALT (bits 0 .. 3, not ref's).
// c and d wrap as the counters do.
DCN_STRAND_FN dcn_strand_table dcn_strand_base_table(uint32_t n0, uint32_t n1, uint32_t n2, uint32_t n3, uint32_t r0, uint32_t r1,
                                                     uint32_t r2, uint32_t r3, uint32_t ref, uint32_t alt_mask) {
    const uint32_t f0 = dcn_strand_forward(n0, r0), f1 = dcn_strand_forward(n1, r1), f2 = dcn_strand_forward(n2, r2),
                   f3 = dcn_strand_forward(n3, r3);
    dcn_strand_table t;
    t.a = ref == 0 ? f0 : ref == 1 ? f1 : ref == 2 ? f2 : f3;
    t.b = ref == 0 ? r0 : ref == 1 ? r1 : ref == 2 ? r2 : r3;
    t.c = ((alt_mask & 1u) ? f0 : 0u) + ((alt_mask & 2u) ? f1 : 0u) + ((alt_mask & 4u) ? f2 : 0u) + ((alt_mask & 8u) ? f3 : 0u);
    t.d = ((alt_mask & 1u) ? r0 : 0u) + ((alt_mask & 2u) ? r1 : 0u) + ((alt_mask & 4u) ? r2 : 0u) + ((alt_mask & 8u) ? r3 : 0u);
    return t;
}

// rule S4: depth = P4's depth(p), rev = REV(p), a_all = the winner's count, a_rev = its events with reverse = 1 (<= a_all)
DCN_STRAND_FN dcn_strand_table dcn_strand_indel_table(uint32_t depth, uint32_t rev, uint32_t a_all, uint32_t a_rev) {
    dcn_strand_table t;
    t.d = a_rev;
    t.c = a_all - a_rev;
    t.b = rev >= t.d ? rev - t.d : 0u;
    const uint32_t fwd = depth >= rev ? depth - rev : 0u;
    t.a = fwd >= t.c ? fwd - t.c : 0u;
    return t;
}

// rule S5: hundredths of a chi-square with one degree of freedom.  Each entry is below 2^10 behind the shift, so N < 2^12,
// |ad - bc| < 2^20, and the numerator 100 N (ad - bc)^2 < 2^7 * 2^12 * 2^40 = 2^59; the denominator is below 2^44.
DCN_STRAND_FN uint32_t dcn_strand_score(const dcn_strand_table &t) {
    uint32_t m = t.a > t.b ? t.a : t.b;
    m = t.c > m ? t.c : m;
    m = t.d > m ? t.d : m;
    uint32_t s = 0;
    while ((m >> s) >= 1024u) ++s; // the bit length of m, less 10
    const uint64_t a = t.a >> s, b = t.b >> s, c = t.c >> s, d = t.d >> s;
    const uint64_t N = a + b + c + d, r1 = a + b, r2 = c + d, c1 = a + c, c2 = b + d;
    const uint64_t den = r1 * r2 * c1 * c2;
    if (den == 0) return 0u;
    const uint64_t ad = a * d, bc = b * c, diff = ad >= bc ? ad - bc : bc - ad;
    const uint64_t sb = 100u * N * diff * diff / den;
    return sb < DCN_STRAND_SB_CAP ? (uint32_t)sb : DCN_STRAND_SB_CAP;
}

// rule S6, on the unshifted table
DCN_STRAND_FN uint32_t dcn_strand_flags(const dcn_strand_table &t, uint32_t sb_centi, const dcn_strand_prm &p) {
    uint32_t flags = 0;
    if (p.max_sb_centi > 0 && sb_centi >= p.max_sb_centi) flags |= DCN_STRAND_FLAG_BIAS;
    const uint32_t least = t.c < t.d ? t.c : t.d;
    if (least < p.min_alt_strand && (uint64_t)t.a + t.c >= p.min_strand_depth && (uint64_t)t.b + t.d >= p.min_strand_depth)
        flags |= DCN_STRAND_FLAG_ONE_SIDED;
    return flags;
}

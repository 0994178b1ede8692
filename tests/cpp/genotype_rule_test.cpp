// genotype_rule_test.cpp -- dcn_genotype.h's dcn_genotype_decide on the host against a second formulation of rules G2 - G7
// (tests/test_genotype_abi.py compiles this with g++ -fsanitize=address,undefined and runs it).
//   small:  every count vector with D <= 6, each column expanded into its n[c] observations, each observation with a quality
//           of its own from a small set and a cost of its own under every genotype; Q[c] is the sum of the column's
//           qualities.  Both ploidies, three parameter sets, every reference column and the invalid one.
//   large:  100,000 random vectors with counters and sums up to 2^32 - 1 and both centi parameters up to 100000; a column is
//           then n[c] observations of which only the total quality is known, and its cost is taken in 128 bits and must fit
//           64.  QUAL's saturation is forced.
// pl is written into exactly ten bytes between guard bytes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "dcn_genotype.h"

typedef unsigned __int128 u128;

static const int GT2[10][2] = {{0, 0}, {0, 1}, {1, 1}, {0, 2}, {1, 2}, {2, 2}, {0, 3}, {1, 3}, {2, 3}, {3, 3}};

static long checked = 0;
static bool saturated = false;

static void fail(const char *what, const uint32_t *n, const uint32_t *Q, uint32_t ref, const dcn_geno_params &p, long got, long want) {
    printf("FAIL %s: n=%u,%u,%u,%u Q=%u,%u,%u,%u ref=%u ploidy=%u err=%u het=%u got %ld want %ld\n", what, n[0], n[1], n[2], n[3], Q[0], Q[1],
           Q[2], Q[3], ref, p.ploidy, p.err_centi, p.het_centi, got, want);
    exit(1);
}

// the costs come from the caller's formulation; the decision is restated here with a loop over the genotypes
static void compare(const uint32_t *n, const uint32_t *Q, uint32_t ref, const dcn_geno_params &p, const std::vector<u128> &cost) {
    const size_t G = cost.size();
    for (u128 c : cost)
        if (c >> 64) fail("a cost does not fit 64 bits", n, Q, ref, p, 0, 0);
    size_t best = 0;
    for (size_t g = 1; g < G; ++g)
        if (cost[g] < cost[best]) best = g;
    u128 second = ~(u128)0;
    for (size_t g = 0; g < G; ++g)
        if (g != best && cost[g] < second) second = cost[g];
    const u128 gq128 = (second - cost[best]) / 100;
    const uint32_t gq = gq128 > 99 ? 99u : (uint32_t)gq128;
    uint32_t pl[10] = {};
    for (size_t g = 0; g < G; ++g) {
        const u128 x = (cost[g] - cost[best]) / 100;
        pl[g] = x > 255 ? 255u : (uint32_t)x;
    }
    const bool ref_valid = ref <= 3;
    size_t ref_gt = 0;
    for (size_t g = 0; g < G; ++g)
        if (p.ploidy == 1 ? g == ref : (GT2[g][0] == (int)ref && GT2[g][1] == (int)ref)) ref_gt = g;
    u128 qual128 = ref_valid ? (cost[ref_gt] - cost[best]) / 100 : 0;
    if (qual128 > 0xFFFFFFFFull) qual128 = 0xFFFFFFFFull, saturated = true;
    const uint64_t D = (uint64_t)n[0] + n[1] + n[2] + n[3];
    const bool called = D >= (p.min_depth > 1 ? p.min_depth : 1) && gq >= p.min_gq;
    const bool site = called && ref_valid && best != ref_gt && (uint32_t)qual128 >= p.min_qual;

    struct {
        uint8_t front[16], pl[10], back[16];
    } box;
    for (int i = 0; i < 16; ++i) box.front[i] = box.back[i] = 0xA5;
    for (int i = 0; i < 10; ++i) box.pl[i] = 0x5A;
    const dcn_geno_result r = dcn_genotype_decide(n, Q, ref, p, box.pl);
    for (int i = 0; i < 16; ++i)
        if (box.front[i] != 0xA5 || box.back[i] != 0xA5) fail("a guard byte", n, Q, ref, p, i, 0);
    if (r.best != best) fail("best", n, Q, ref, p, r.best, (long)best);
    if (r.gt != (called ? best : DCN_GENO_NONE)) fail("gt", n, Q, ref, p, r.gt, called ? (long)best : 255);
    if (r.gq != gq) fail("gq", n, Q, ref, p, r.gq, gq);
    if (r.qual != (uint32_t)qual128) fail("qual", n, Q, ref, p, r.qual, (long)(uint32_t)qual128);
    if (r.site != (site ? 1u : 0u)) fail("site", n, Q, ref, p, r.site, site);
    for (int g = 0; g < 10; ++g)
        if (box.pl[g] != pl[g]) fail("pl", n, Q, ref, p, box.pl[g], pl[g]);
    ++checked;
}

// one observation (base c, quality q) under a genotype of `alleles` distinct alleles a0, a1
static u128 observation_cost(uint32_t c, uint32_t q, int a0, int a1, const dcn_geno_params &p) {
    if ((int)c != a0 && (int)c != a1) return (u128)100 * q + p.err_centi; // an error
    return a0 != a1 ? p.het_centi : 0;                                     // a match: half of the chromosomes carry it, or all
}

static void small_case(const uint32_t *n, const std::vector<uint32_t> *quals, uint32_t ref, const dcn_geno_params &p) {
    uint32_t Q[4];
    for (int c = 0; c < 4; ++c) {
        Q[c] = 0;
        for (uint32_t q : quals[c]) Q[c] += q;
    }
    std::vector<u128> cost;
    const int G = p.ploidy == 2 ? 10 : 4;
    for (int g = 0; g < G; ++g) {
        const int a0 = p.ploidy == 2 ? GT2[g][0] : g, a1 = p.ploidy == 2 ? GT2[g][1] : g;
        u128 sum = 0;
        for (uint32_t c = 0; c < 4; ++c)
            for (uint32_t q : quals[c]) sum += observation_cost(c, q, a0, a1, p);
        cost.push_back(sum);
    }
    compare(n, Q, ref, p, cost);
}

static void large_case(const uint32_t *n, const uint32_t *Q, uint32_t ref, const dcn_geno_params &p) {
    std::vector<u128> cost;
    const int G = p.ploidy == 2 ? 10 : 4;
    for (int g = 0; g < G; ++g) {
        const int a0 = p.ploidy == 2 ? GT2[g][0] : g, a1 = p.ploidy == 2 ? GT2[g][1] : g;
        u128 sum = 0;
        for (int c = 0; c < 4; ++c) { // n[c] observations whose qualities sum to Q[c]
            if (c != a0 && c != a1) sum += (u128)100 * Q[c] + (u128)p.err_centi * n[c];
            else if (a0 != a1) sum += (u128)p.het_centi * n[c];
        }
        cost.push_back(sum);
    }
    compare(n, Q, ref, p, cost);
}

int main() {
    std::mt19937_64 rng(1919);
    const uint32_t qset[] = {0, 1, 7, 20, 30, 41, 93};
    const dcn_geno_params sets[] = {{2, 3, 20, 20, 477, 301}, {2, 0, 0, 0, 477, 301}, {2, 1, 4, 50, 0, 0}, {2, 6, 99, 1, 1000, 100}};
    long vectors = 0;
    for (uint32_t a = 0; a <= 6; ++a)
        for (uint32_t c = 0; a + c <= 6; ++c)
            for (uint32_t g = 0; a + c + g <= 6; ++g)
                for (uint32_t t = 0; a + c + g + t <= 6; ++t) {
                    const uint32_t n[4] = {a, c, g, t};
                    ++vectors;
                    for (int rep = 0; rep < 6; ++rep) {
                        std::vector<uint32_t> quals[4];
                        for (int col = 0; col < 4; ++col)
                            for (uint32_t i = 0; i < n[col]; ++i) quals[col].push_back(rep == 0 ? 30u : qset[rng() % 7]);
                        for (const dcn_geno_params &s : sets)
                            for (uint32_t ploidy = 1; ploidy <= 2; ++ploidy)
                                for (uint32_t ref = 0; ref <= 4; ++ref) {
                                    dcn_geno_params p = s;
                                    p.ploidy = ploidy;
                                    small_case(n, quals, ref, p);
                                }
                    }
                }
    const long small = checked;
    for (int i = 0; i < 100000; ++i) {
        uint32_t n[4], Q[4];
        for (int c = 0; c < 4; ++c) {
            const int kind = (int)(rng() % 4); // all magnitudes, and the ends of the range
            n[c] = kind == 0 ? 0xFFFFFFFFu : kind == 1 ? (uint32_t)(rng() % 50) : (uint32_t)rng() >> (rng() % 32);
            const int kq = (int)(rng() % 4);
            Q[c] = kq == 0 ? 0xFFFFFFFFu : kq == 1 ? (uint32_t)(rng() % 2000) : (uint32_t)rng() >> (rng() % 32);
        }
        dcn_geno_params p;
        p.ploidy = 1 + (uint32_t)(rng() % 2);
        p.min_depth = (uint32_t)(rng() % 3 == 0 ? rng() : rng() % 40);
        p.min_gq = (uint32_t)(rng() % 100);
        p.min_qual = (uint32_t)(rng() % 2 ? rng() % 100 : rng());
        p.err_centi = (uint32_t)(rng() % 3 == 0 ? 100000 : rng() % 100001);
        p.het_centi = (uint32_t)(rng() % 3 == 0 ? 100000 : rng() % 100001);
        large_case(n, Q, (uint32_t)(rng() % 5), p);
    }
    { // QUAL saturates: every read shows C at full quality on a reference A
        const uint32_t n[4] = {0, 0xFFFFFFFFu, 0, 0}, Q[4] = {0, 0xFFFFFFFFu, 0, 0};
        saturated = false;
        for (uint32_t ploidy = 1; ploidy <= 2; ++ploidy) large_case(n, Q, 0, {ploidy, 3, 20, 20, 100000, 100000});
        if (!saturated) {
            printf("FAIL: QUAL did not saturate\n");
            return 1;
        }
    }
    printf("genotype rule ok: %ld count vectors, %ld small cases, %ld large cases, QUAL saturated\n", vectors, small, checked - small);
    return 0;
}

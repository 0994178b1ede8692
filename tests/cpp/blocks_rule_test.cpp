// blocks_rule_test.cpp -- csrc/dcn_blocks.h compiled for the host alone: rule B2's class at every boundary of the rule, and
// rules B6 / B7, against a brute force that is written from the definition (include/deacon_hip_blocks.h) and shares nothing
// with the header but dcn_genotype_decide's result.  A program of its own, so that it runs under the address and
// undefined-behaviour sanitizers without anything preloaded:
//   g++ -O1 -std=c++17 -Wall -Werror -fsanitize=address,undefined -I deacon-server_amd/csrc tests/cpp/blocks_rule_test.cpp
// It prints one line per checked position of its hand-written part (tests/test_blocks_abi.py reads them through the Python
// model) and a last line "blocks rule ok: ...".
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "dcn_blocks.h"

namespace {

int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);            \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

const dcn_geno_params DEFAULTS = {2, 3, 20, 20, 477, 301};

struct position {
    uint32_t n[4], Q[4], n_n, n_del, ref_column;
};

// rule B2 as the definition reads, the edges in a plain array
uint32_t brute_class(const position &p, const dcn_geno_params &prm, const std::vector<uint8_t> &edges, uint32_t *gq) {
    uint8_t pl[DCN_GENO_GENOTYPES];
    const dcn_geno_result r = dcn_genotype_decide(p.n, p.Q, p.ref_column, prm, pl);
    *gq = r.gq;
    if (r.site) return 255;
    uint64_t depth = (uint64_t)p.n_n + p.n_del;
    for (int c = 0; c < 4; ++c) depth += p.n[c];
    if (depth == 0) return 0;
    const bool ref_valid = p.ref_column <= 3;
    uint32_t ref_gt = p.ref_column;
    if (prm.ploidy == 2) ref_gt = p.ref_column * (p.ref_column + 1) / 2 + p.ref_column;
    if (r.gt != DCN_GENO_NONE && ref_valid && r.best == ref_gt) {
        uint32_t b = 0;
        for (uint8_t e : edges) b += e <= r.gq;
        return 2 + b;
    }
    return 1;
}

dcn_blk_edges pack(const std::vector<uint8_t> &edges) {
    uint8_t raw[16] = {};
    for (size_t i = 0; i < edges.size(); ++i) raw[i] = edges[i];
    return dcn_blocks_pack_edges(raw, (uint32_t)edges.size());
}

uint64_t checked = 0;
uint32_t check_position(const position &p, const dcn_geno_params &prm, const std::vector<uint8_t> &edges, bool print = false) {
    uint32_t gq = 0;
    const uint32_t want = brute_class(p, prm, edges, &gq);
    const dcn_blk_position got = dcn_blocks_classify(p.n, p.Q, p.n_n, p.n_del, p.ref_column, prm, pack(edges));
    CHECK(got.cls == want);
    CHECK(got.gq == gq);
    CHECK(got.depth == p.n[0] + p.n[1] + p.n[2] + p.n[3]);
    ++checked;
    if (print) {
        std::printf("row %u %u %u %u  %u %u %u %u  %u %u %u  %u %u %u %u %u %u  %zu", p.n[0], p.n[1], p.n[2], p.n[3], p.Q[0], p.Q[1], p.Q[2], p.Q[3], p.n_n,
                    p.n_del, p.ref_column, prm.ploidy, prm.min_depth, prm.min_gq, prm.min_qual, prm.err_centi, prm.het_centi, edges.size());
        for (uint8_t e : edges) std::printf(" %u", e);
        std::printf("  -> %u %u %u\n", got.cls, got.gq, got.depth);
    }
    return got.cls;
}

// the blocks of per-position classes, by a plain loop (rules B3 - B5)
struct pos_info {
    uint32_t cls, gq, depth;
};
std::vector<dcn_blk_block> blocks_of(const std::vector<pos_info> &v, uint64_t from, uint64_t to) {
    std::vector<dcn_blk_block> out;
    for (uint64_t q = from; q < to;) {
        if (v[q].cls == 255) {
            ++q;
            continue;
        }
        dcn_blk_block b = {q, 0, 0, 0xFFFFFFFFu, 0, 0xFFFFFFFFu, v[q].cls, 0};
        for (; q < to && v[q].cls == b.cls; ++q) {
            b.len += 1, b.sum_depth += v[q].depth;
            b.min_depth = v[q].depth < b.min_depth ? v[q].depth : b.min_depth;
            b.max_depth = v[q].depth > b.max_depth ? v[q].depth : b.max_depth;
            b.min_gq = v[q].gq < b.min_gq ? v[q].gq : b.min_gq;
        }
        out.push_back(b);
    }
    return out;
}

std::vector<dcn_blk_block> merged(std::vector<dcn_blk_block> v) { // rule B6, with the header's two functions
    std::vector<dcn_blk_block> out;
    for (const dcn_blk_block &b : v) {
        if (!out.empty() && dcn_blocks_mergeable(out.back(), b)) dcn_blocks_merge_into(out.back(), b);
        else out.push_back(b);
    }
    return out;
}

bool same(const std::vector<dcn_blk_block> &a, const std::vector<dcn_blk_block> &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i].pos != b[i].pos || a[i].len != b[i].len || a[i].cls != b[i].cls || a[i].min_gq != b[i].min_gq || a[i].min_depth != b[i].min_depth ||
            a[i].max_depth != b[i].max_depth || a[i].sum_depth != b[i].sum_depth || a[i].reserved != b[i].reserved)
            return false;
    return true;
}

} // namespace

int main() {
    const std::vector<uint8_t> five = {20, 40, 60, 80, 99};
    // ---- rule B2 at its boundaries, by hand (reference base A = column 0 unless said) ----------------------------------
    const auto ref_reads = [](uint32_t k, uint32_t q) { return position{{k, 0, 0, 0}, {k * q, 0, 0, 0}, 0, 0, 0}; };
    CHECK(check_position(position{{0, 0, 0, 0}, {0, 0, 0, 0}, 0, 0, 0}, DEFAULTS, five, true) == 0);          // nothing at all
    CHECK(check_position(position{{0, 0, 0, 0}, {0, 0, 0, 0}, 4, 0, 0}, DEFAULTS, five, true) == 1);          // N only
    CHECK(check_position(position{{0, 0, 0, 0}, {0, 0, 0, 0}, 0, 4, 0}, DEFAULTS, five, true) == 1);          // DEL only
    CHECK(check_position(position{{0, 0, 0, 0}, {0, 0, 0, 0}, 0, 0, 4}, DEFAULTS, five, true) == 0);          // an invalid base, uncovered
    CHECK(check_position(position{{8, 0, 0, 0}, {240, 0, 0, 0}, 0, 0, 4}, DEFAULTS, five, true) == 1);        // an invalid base, covered
    CHECK(check_position(ref_reads(2, 30), DEFAULTS, five, true) == 1);                                       // D under min_depth
    CHECK(check_position(ref_reads(3, 30), DEFAULTS, five, true) == 1);                                       // D = min_depth, GQ 9 under min_gq
    CHECK(check_position(ref_reads(6, 30), DEFAULTS, five, true) == 1);                                       // GQ 18
    CHECK(check_position(ref_reads(7, 30), DEFAULTS, five, true) == 3);                                       // GQ 21: called, band 1
    CHECK(check_position(ref_reads(10, 30), DEFAULTS, {29}, true) == 3);                                      // GQ 30 over, at and under an edge
    CHECK(check_position(ref_reads(10, 30), DEFAULTS, {30}, true) == 3);
    CHECK(check_position(ref_reads(10, 30), DEFAULTS, {31}, true) == 2);
    CHECK(check_position(ref_reads(10, 30), DEFAULTS, {}, true) == 2);                                        // no edge
    CHECK(check_position(ref_reads(40, 30), DEFAULTS, {99}, true) == 3);                                      // GQ 99 at edge 99
    CHECK(check_position(ref_reads(40, 30), DEFAULTS, {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 99}, true) == 17);  // fifteen edges, all reached
    CHECK(check_position(ref_reads(10, 30), DEFAULTS, {6, 12, 18, 24, 30, 36, 42, 48, 54, 60, 66, 72, 78, 84, 90}, true) == 7);
    CHECK(check_position(ref_reads(3, 30), dcn_geno_params{1, 3, 20, 20, 477, 301}, five, true) == 7);        // ploidy 1: GQ 99 from three reads
    const position het = {{5, 5, 0, 0}, {150, 150, 0, 0}, 0, 0, 0};                                           // QUAL 143
    CHECK(check_position(het, dcn_geno_params{2, 3, 20, 143, 477, 301}, five, true) == 255);                  // a site
    CHECK(check_position(het, dcn_geno_params{2, 3, 20, 144, 477, 301}, five, true) == 1);                    // called, not the reference's, under min_qual
    CHECK(check_position(het, dcn_geno_params{1, 3, 20, 20, 477, 301}, five, true) == 1);                     // ploidy 1: a tie, GQ 0
    const position hom_alt = {{0, 9, 0, 0}, {0, 270, 0, 0}, 0, 0, 0};
    CHECK(check_position(hom_alt, DEFAULTS, five, true) == 255);
    CHECK(check_position(position{{0, 9, 0, 0}, {0, 270, 0, 0}, 0, 0, 1}, DEFAULTS, five, true) == 3);        // the same reads on a reference C
    CHECK(check_position(position{{0, 0, 0, 9}, {0, 0, 0, 270}, 0, 0, 3}, DEFAULTS, five, true) == 3);        // ... and T / T (genotype 9)
    CHECK(check_position(position{{0, 9, 0, 0}, {0, 270, 0, 0}, 3, 2, 4}, DEFAULTS, five, true) == 1);        // called, the reference base invalid
    CHECK(check_position(ref_reads(0xFFFFFFFFu / 93, 93), dcn_geno_params{2, 3, 20, 20, 100000, 100000}, five, true) == 7);  // costs past 32 bits
    // the band counts every edge at or under GQ and none behind the list
    for (uint32_t gq = 0; gq <= 99; ++gq)
        for (const std::vector<uint8_t> &edges : {std::vector<uint8_t>{}, std::vector<uint8_t>{1}, std::vector<uint8_t>{99}, five,
                                                  std::vector<uint8_t>{1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}}) {
            uint32_t want = 0;
            for (uint8_t e : edges) want += e <= gq;
            CHECK(dcn_blocks_band(gq, pack(edges)) == want);
        }

    // ---- random counters against the brute force, then B3 - B7 over random records ---------------------------------------
    std::mt19937_64 rng(2401);
    const auto pick = [&rng](uint32_t n) { return (uint32_t)(rng() % n); };
    uint64_t seen[256] = {}, cuts = 0, n_blocks = 0;
    for (int round = 0; round < 250; ++round) {
        dcn_geno_params prm = {1 + pick(2), pick(6), pick(3) ? pick(40) : 0u, pick(3) ? pick(200) : 0u, pick(2) ? 477u : pick(2000), pick(2) ? 301u : pick(1000)};
        std::vector<uint8_t> edges;
        for (uint32_t e = 1 + pick(30); e <= 99 && edges.size() < 15; e += 1 + pick(30)) edges.push_back((uint8_t)e);
        if (pick(8) == 0) edges.clear();
        const uint64_t len = 1 + pick(300);
        std::vector<pos_info> v(len);
        uint32_t mode = 0, depth = 0;
        for (uint64_t q = 0; q < len; ++q) {
            if (pick(12) == 0) mode = pick(6), depth = pick(2) ? pick(6) : pick(40);  // stretches of one kind, so that blocks have lengths
            position p = {{0, 0, 0, 0}, {0, 0, 0, 0}, 0, 0, pick(20) ? pick(4) : 4u};
            const uint32_t ref = p.ref_column & 3u;
            if (mode <= 2) p.n[ref] = depth + (mode == 2 ? pick(3) : 0u);
            if (mode == 3) p.n[ref] = depth, p.n[(ref + 1) & 3u] = pick(2) ? depth : pick(4);
            if (mode == 4) p.n_n = depth, p.n_del = pick(3);
            if (mode == 5)
                for (int c = 0; c < 4; ++c) p.n[c] = pick(12);
            for (int c = 0; c < 4; ++c) p.Q[c] = p.n[c] * (pick(4) ? 30u : pick(42));
            const uint32_t cls = check_position(p, prm, edges);
            uint32_t gq = 0;
            brute_class(p, prm, edges, &gq);
            v[q] = {pick(40) == 0 ? 255u : cls, gq, p.n[0] + p.n[1] + p.n[2] + p.n[3]};  // (a break now and then)
            ++seen[v[q].cls];
        }
        const std::vector<dcn_blk_block> whole = blocks_of(v, 0, len);
        n_blocks += whole.size();
        CHECK(same(merged(whole), whole));  // maximal runs: nothing left to merge
        for (size_t i = 1; i < whole.size(); ++i) CHECK(whole[i - 1].pos + whole[i - 1].len <= whole[i].pos);
        for (uint64_t m = 0; m <= len; ++m) {  // rule B7 at every cut, and at two cuts
            std::vector<dcn_blk_block> halves = blocks_of(v, 0, m), back = blocks_of(v, m, len);
            halves.insert(halves.end(), back.begin(), back.end());
            CHECK(same(merged(halves), whole));
            ++cuts;
            const uint64_t m2 = m + pick((uint32_t)(len - m + 1));
            std::vector<dcn_blk_block> three = blocks_of(v, 0, m), mid = blocks_of(v, m, m2), last = blocks_of(v, m2, len);
            three.insert(three.end(), mid.begin(), mid.end());
            three.insert(three.end(), last.begin(), last.end());
            CHECK(same(merged(three), whole));
        }
    }
    CHECK(seen[0] > 100 && seen[1] > 1000 && seen[255] > 100);
    uint32_t bands_seen = 0;
    for (uint32_t c = 2; c <= 17; ++c) bands_seen += seen[c] > 0;
    CHECK(bands_seen >= 10);
    // rule B6 by hand: touching blocks of one class merge, others do not
    dcn_blk_block a = {10, 70, 5, 3, 9, 12, 3, 0}, b = {15, 11, 2, 1, 20, 30, 3, 0};
    CHECK(dcn_blocks_mergeable(a, b));
    dcn_blk_block gap = b, other = b;
    gap.pos = 16, other.cls = 4;
    CHECK(!dcn_blocks_mergeable(a, gap) && !dcn_blocks_mergeable(a, other) && !dcn_blocks_mergeable(b, a));
    dcn_blocks_merge_into(a, b);
    CHECK(a.pos == 10 && a.len == 7 && a.sum_depth == 81 && a.min_depth == 1 && a.max_depth == 20 && a.min_gq == 12 && a.cls == 3);
    if (failures) {
        std::printf("blocks rule FAILED: %d checks\n", failures);
        return 1;
    }
    std::printf("blocks rule ok: %llu positions, %llu blocks, %llu cuts\n", (unsigned long long)checked, (unsigned long long)n_blocks, (unsigned long long)cuts);
    return 0;
}

// indel_rule_test.cpp -- the rules of csrc/dcn_indels.h (R2, R5 and I1 - I5 of include/deacon_hip.h) on the host alone:
// the decision against a brute-force table, written here with an array of costs, a loop over the genotypes and 128-bit
// sums, over small a and o and every parameter boundary; the extremes (counts of 2^32 - 1, centi of 100000); the event
// positions of hand-written run lists, with a leading and a trailing D run; the winner of hand-written buckets.  Built
// with -fsanitize=address,undefined by tests/test_indels_abi.py and run as a child process.
#include "dcn_indels.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

static int failures = 0;
static long checks = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        ++checks;                                                    \
        if (!(cond)) {                                               \
            ++failures;                                              \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);    \
        }                                                            \
    } while (0)

typedef unsigned __int128 u128;

struct expect {
    uint32_t gt, gq, qual, site, pl[3];
};

// rules I2 - I5 as they read
static expect brute(uint32_t a, uint32_t depth, const dcn_indel_prm &p) {
    const u128 A = a, O = depth >= a ? depth - a : 0;
    std::vector<u128> cost;
    if (p.ploidy == 2) cost = {(u128)p.indel_centi * A, (u128)p.het_centi * (A + O), (u128)p.indel_centi * O};
    else cost = {(u128)p.indel_centi * A, (u128)p.indel_centi * O};
    size_t best = 0;
    for (size_t g = 1; g < cost.size(); ++g)
        if (cost[g] < cost[best]) best = g;
    bool have = false;
    u128 second = 0;
    for (size_t g = 0; g < cost.size(); ++g)
        if (g != best && (!have || cost[g] < second)) second = cost[g], have = true;
    expect e = {};
    e.gt = (uint32_t)best;
    const u128 gq = (second - cost[best]) / 100;
    e.gq = gq > 99 ? 99u : (uint32_t)gq;
    for (size_t g = 0; g < cost.size(); ++g) {
        const u128 v = (cost[g] - cost[best]) / 100;
        e.pl[g] = v > 255 ? 255u : (uint32_t)v;
    }
    const u128 qual = (cost[0] - cost[best]) / 100;
    e.qual = qual > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)qual;
    const bool called = depth >= (p.min_depth > 1 ? p.min_depth : 1) && e.gq >= p.min_gq;
    e.site = called && best != 0 && e.qual >= p.min_qual;
    return e;
}

static void compare(uint32_t a, uint32_t depth, const dcn_indel_prm &p) {
    uint8_t pl[3] = {7, 7, 7};
    const dcn_indel_result r = dcn_indel_decide(a, depth, p, pl);
    const expect e = brute(a, depth, p);
    CHECK(r.gt == e.gt && r.gq == e.gq && r.qual == e.qual && r.site == e.site);
    CHECK(pl[0] == e.pl[0] && pl[1] == e.pl[1] && pl[2] == e.pl[2]);
}

int main() {
    // ---- I3 - I5 against the table: small a and o, every parameter boundary ----
    const uint32_t centis[] = {0, 1, 99, 100, 301, 2000, 100000};
    for (uint32_t ploidy = 1; ploidy <= 2; ++ploidy)
        for (uint32_t ic : centis)
            for (uint32_t hc : centis)
                for (uint32_t min_depth : {0u, 1u, 3u, 12u})
                    for (uint32_t min_gq : {0u, 1u, 20u, 99u})
                        for (uint32_t min_qual : {0u, 1u, 20u, 400u}) {
                            const dcn_indel_prm p = {ploidy, min_depth, min_gq, min_qual, 2, ic, hc};
                            for (uint32_t a = 0; a <= 12; ++a)
                                for (uint32_t o = 0; o <= 12; ++o) compare(a, a + o, p);
                        }
    // written out: three of six reads at the defaults is a heterozygote, six of six a homozygote
    {
        const dcn_indel_prm p = {2, 3, 20, 20, 2, 2000, 301};
        uint8_t pl[3];
        dcn_indel_result r = dcn_indel_decide(3, 6, p, pl);
        CHECK(r.gt == 1 && r.gq == 41 && r.qual == 41 && r.site == 1 && pl[0] == 41 && pl[1] == 0 && pl[2] == 41); // 6000 - 1806 = 4194
        r = dcn_indel_decide(6, 6, p, pl);
        CHECK(r.gt == 2 && r.gq == 18 && r.qual == 120 && r.site == 0 && pl[0] == 120 && pl[1] == 18 && pl[2] == 0); // 1806 / 100: under min_gq
        r = dcn_indel_decide(0, 6, p, pl);
        CHECK(r.gt == 0 && r.site == 0 && r.qual == 0);
        // equal costs: the first in order wins
        const dcn_indel_prm q = {2, 1, 0, 0, 1, 100, 100};
        r = dcn_indel_decide(1, 1, q, pl); // 100, 100, 0
        CHECK(r.gt == 2);
        r = dcn_indel_decide(1, 2, q, pl); // 100, 200, 100: R/R before V/V
        CHECK(r.gt == 0 && r.gq == 0 && r.site == 0);
        // a > depth (a wrapped counter): o is 0, nothing underflows
        r = dcn_indel_decide(9, 4, p, pl);
        CHECK(r.gt == 2 && pl[2] == 0);
    }
    // PL at 255 and 256, GQ at 99 and 100
    {
        uint8_t pl[3];
        dcn_indel_prm p = {1, 1, 0, 0, 1, 100, 0};
        CHECK(dcn_indel_decide(255, 255, p, pl).gq == 99 && pl[0] == 255);
        dcn_indel_decide(254, 254, p, pl);
        CHECK(pl[0] == 254);
        dcn_indel_decide(256, 256, p, pl);
        CHECK(pl[0] == 255);
        CHECK(dcn_indel_decide(99, 99, p, pl).gq == 99 && dcn_indel_decide(98, 98, p, pl).gq == 98 && dcn_indel_decide(100, 100, p, pl).gq == 99);
    }
    // ---- the extremes ----
    for (uint32_t ploidy = 1; ploidy <= 2; ++ploidy)
        for (uint32_t ic : {0u, 1u, 100000u})
            for (uint32_t hc : {0u, 1u, 100000u})
                for (uint32_t a : {0u, 1u, 0x7FFFFFFFu, 0xFFFFFFFEu, 0xFFFFFFFFu})
                    for (uint32_t depth : {0u, 1u, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu}) {
                        const dcn_indel_prm p = {ploidy, 3, 20, 20, 2, ic, hc};
                        compare(a, depth, p);
                    }
    {
        const dcn_indel_prm p = {1, 0, 0, 0, 0, 100000, 100000};
        uint8_t pl[3];
        const dcn_indel_result r = dcn_indel_decide(0xFFFFFFFFu, 0xFFFFFFFFu, p, pl);
        CHECK(r.gt == 1 && r.qual == 0xFFFFFFFFu && r.gq == 99 && pl[0] == 255 && pl[1] == 0 && pl[2] == 0); // 100000 (2^32 - 1) / 100 saturates
    }
    // ---- I1 ----
    CHECK(dcn_indel_candidate(1, 0) && dcn_indel_candidate(1, 1) && !dcn_indel_candidate(1, 2) && dcn_indel_candidate(2, 2) && !dcn_indel_candidate(0, 0));
    CHECK(dcn_indel_candidate(0xFFFFFFFFu, 0xFFFFFFFFu) && !dcn_indel_candidate(0xFFFFFFFEu, 0xFFFFFFFFu));
    // ---- R2: the events of hand-written run lists ----
    {
        const auto run = [](uint32_t len, uint32_t op) { return len << 4 | op; };
        // 3D 10= 2I 1X 4D 5= 1D: a D run first and a D run last
        const std::vector<uint32_t> runs = {run(3, DCN_ALN_D), run(10, DCN_ALN_EQ), run(2, DCN_ALN_I), run(1, DCN_ALN_X),
                                            run(4, DCN_ALN_D), run(5, DCN_ALN_EQ), run(1, DCN_ALN_D)};
        std::vector<dcn_del_event> got;
        uint32_t j = 0, events = 0;
        for (uint32_t r : runs) {
            events += dcn_del_run_events(r);
            if (dcn_del_run_events(r)) got.push_back(dcn_del_event_of(r, j, 1, 1000));
            j += dcn_pile_step_t(r);
        }
        CHECK(events == 3 && got.size() == 3 && j == 24);
        CHECK(got[0].base == 1000 && got[0].len == 3 && got[0].flags == DCN_DEL_REVERSE);
        CHECK(got[1].base == 1014 && got[1].len == 4);
        CHECK(got[2].base == 1023 && got[2].len == 1);
        CHECK(dcn_del_event_of(run(7, DCN_ALN_D), 0, 0, 5).flags == 0 && dcn_del_run_events(run(7, DCN_ALN_I)) == 0 &&
              dcn_del_run_events(run(7, DCN_ALN_EQ)) == 0 && dcn_del_run_events(run(7, DCN_ALN_X)) == 0);
        // a position of the store past 2^32
        CHECK(dcn_del_event_of(run(2, DCN_ALN_D), 0xFFFFFFF0u, 0, 0x100000000ull).base == 0x1FFFFFFF0ull);
    }
    // ---- R5: the winner of a bucket, over every number of lanes ----
    {
        const uint32_t lens[] = {3, 1, 3, 2, 2, 1, 3, 2}; // 3 x3, 2 x3, 1 x2: a 3 : 3 tie goes to the shorter
        std::vector<dcn_del_event> events(8);
        std::vector<uint64_t> slots(8);
        for (uint32_t k = 0; k < 8; ++k) events[k] = {100, lens[k], 0}, slots[k] = 7 - k;
        for (uint32_t lanes : {1u, 2u, 3u, 8u, 64u}) {
            uint32_t best_len = 0, best_count = 0;
            for (uint32_t lane = 0; lane < lanes; ++lane) {
                uint32_t c = 0;
                const uint32_t len = dcn_del_lane_winner(slots.data(), 8, lane, lanes, events.data(), &c);
                if (c != 0 && (best_count == 0 || dcn_del_beats(c, len, best_count, best_len))) best_len = len, best_count = c;
            }
            CHECK(best_len == 2 && best_count == 3);
        }
        events[1].len = 3; // 3 x4
        uint32_t c = 0;
        CHECK(dcn_del_lane_winner(slots.data(), 8, 0, 1, events.data(), &c) == 3 && c == 4);
        CHECK(dcn_del_lane_winner(slots.data(), 0, 0, 1, events.data(), &c) == 0 && c == 0);
        CHECK(dcn_del_beats(4, 9, 3, 1) && !dcn_del_beats(3, 1, 4, 9) && dcn_del_beats(3, 1, 3, 2) && !dcn_del_beats(3, 2, 3, 2));
    }
    if (failures) {
        std::printf("%d of %ld checks FAILED\n", failures, checks);
        return 1;
    }
    std::printf("indel rule ok: %ld checks\n", checks);
    return 0;
}

// insertion_walk_test.cpp -- the counting and the writing walk of the insertion ledger (dcn_insertions.h) on the host, under
// the address and undefined-behaviour sanitizers (tests/test_insertions_abi.py builds and runs it).  The kernel's shape is
// kept: the counting pass sums dcn_ins_run_events / _bases over the runs as 64 lanes stride over them; the writing pass takes
// the runs in chunks of 64, each I run's (i, j) and its event and base offsets from the prefix sums of the chunk (emulated
// serially here) on top of where the chunk begins, then dcn_ins_write_run by each of 64 lanes.  Events and bases go into
// arrays of exactly the counted size between guard words and are compared with a walk step by step by rule L2.  The winner
// rule (dcn_ins_lane_winner over 64 lanes, reduced with dcn_ins_beats) is compared with a sort and count by rule L5.
#include "dcn_insertions.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <tuple>
#include <vector>

namespace {

constexpr uint8_t GUARD_BYTE = 0xA5;
constexpr size_t GUARD = 32;

int fail(const char *what, size_t list) {
    std::fprintf(stderr, "run list %zu: %s\n", list, what);
    return 1;
}

struct plain_event {
    uint64_t base;
    uint32_t front, len, reverse;
    std::string bases;
};

// rule L2 step by step
std::vector<plain_event> step_walk(const std::vector<uint32_t> &runs, const std::string &s, uint32_t reverse, uint64_t t0) {
    std::vector<plain_event> out;
    uint32_t i = 0, j = 0;
    for (const uint32_t run : runs) {
        const uint32_t op = run & 15u, len = run >> 4;
        if (op == DCN_ALN_I) {
            out.push_back({t0 + (j > 0 ? j - 1 : 0), j == 0 ? 1u : 0u, len, reverse, s.substr(i, len)});
            i += len;
        } else if (op == DCN_ALN_D) {
            j += len;
        } else {
            i += len;
            j += len;
        }
    }
    return out;
}

// a list of `count` runs with no equal neighbours, with n > 0; i_at >= 0: run i_at is an I run of i_len bases
std::vector<uint32_t> make_runs(std::mt19937 &rng, uint32_t count, int first_op, int last_op, int i_at, uint32_t i_len) {
    const uint32_t ops[4] = {DCN_ALN_EQ, DCN_ALN_X, DCN_ALN_I, DCN_ALN_D};
    std::vector<uint32_t> runs;
    uint32_t prev = 99;
    for (uint32_t r = 0; r < count; ++r) {
        uint32_t op;
        do op = ops[rng() % 4];
        while (op == prev);
        if (r == 0 && first_op >= 0) op = (uint32_t)first_op;
        if (r == count - 1 && last_op >= 0 && (uint32_t)last_op != prev) op = (uint32_t)last_op;
        if ((int)r + 1 == i_at && op == DCN_ALN_I) op = prev == DCN_ALN_EQ ? DCN_ALN_X : DCN_ALN_EQ; // (no I run in front of the planted one)
        if ((int)r == i_at) op = DCN_ALN_I;
        if (op == prev) op = op == DCN_ALN_EQ ? DCN_ALN_X : DCN_ALN_EQ;
        uint32_t len = 1 + (rng() % 8 == 0 ? rng() % 130 : rng() % 5);
        if ((int)r == i_at && op == DCN_ALN_I) len = i_len;
        runs.push_back(len << 4 | op);
        prev = op;
    }
    bool any_t = false;
    for (const uint32_t x : runs) any_t = any_t || dcn_pile_step_t(x) > 0;
    if (!any_t) runs.push_back(3u << 4 | ((runs.back() & 15u) == DCN_ALN_EQ ? DCN_ALN_D : DCN_ALN_EQ));
    return runs;
}

int winner_checks(std::mt19937 &rng) {
    const char letters[5] = {'A', 'C', 'G', 'N', 'T'};
    for (int round = 0; round < 400; ++round) {
        const uint32_t sizes[8] = {1, 2, 63, 64, 65, 130, 3, 7};
        const uint32_t count = sizes[round % 8];
        const uint32_t kinds = 1 + rng() % 4; // few alleles: ties are common
        std::vector<dcn_ins_event> events;
        std::vector<uint8_t> bases;
        std::vector<std::tuple<uint32_t, uint32_t, std::string>> pool;
        for (uint32_t k = 0; k < kinds; ++k) {
            std::string b;
            const uint32_t len = 1 + rng() % 3;
            for (uint32_t q = 0; q < len; ++q) b.push_back(letters[rng() % 5]);
            pool.emplace_back(rng() % 2, len, b);
        }
        std::map<std::tuple<uint32_t, uint32_t, std::string>, uint32_t> tally;
        for (uint32_t e = 0; e < count; ++e) {
            const auto &a = pool[rng() % kinds];
            dcn_ins_event ev;
            ev.base = 5;
            ev.bases_offset = bases.size();
            ev.len = std::get<1>(a);
            ev.flags = std::get<0>(a) | (rng() % 2 ? DCN_INS_REVERSE : 0u);
            for (const char c : std::get<2>(a)) bases.push_back((uint8_t)c);
            events.push_back(ev);
            ++tally[a];
        }
        std::vector<uint64_t> slots(count);
        for (uint32_t e = 0; e < count; ++e) slots[e] = e;
        std::shuffle(slots.begin(), slots.end(), rng);
        // rule L5 by sort and count: the map is in L4's order of alleles (front, len, bytes); the first largest wins
        std::tuple<uint32_t, uint32_t, std::string> want;
        uint32_t want_count = 0;
        for (const auto &kv : tally)
            if (kv.second > want_count) want = kv.first, want_count = kv.second;
        uint32_t best = UINT32_MAX, best_count = 0;
        for (uint32_t lane = 0; lane < 64; ++lane) { // the lanes' own winners, reduced as the wave does
            uint32_t c = 0;
            const uint32_t k = dcn_ins_lane_winner(slots.data(), count, lane, 64u, events.data(), bases.data(), &c);
            if (k == UINT32_MAX) continue;
            if (k >= count) return fail("a lane's winner is outside the bucket", (size_t)round);
            if (best == UINT32_MAX || dcn_ins_beats(c, events[slots[k]], best_count, events[slots[best]], bases.data())) best = k, best_count = c;
        }
        if (best == UINT32_MAX) return fail("no winner", (size_t)round);
        const dcn_ins_event &w = events[slots[best]];
        const std::string got((const char *)bases.data() + w.bases_offset, w.len);
        if (best_count != want_count || (w.flags & DCN_INS_FRONT) != std::get<0>(want) || w.len != std::get<1>(want) || got != std::get<2>(want))
            return fail("the winner differs from sort and count", (size_t)round);
    }
    return 0;
}

} // namespace

int main() {
    std::mt19937 rng(1701);
    if (dcn_ins_char(0, 0) != 'A' || dcn_ins_char(1, 0) != 'C' || dcn_ins_char(2, 0) != 'T' || dcn_ins_char(3, 0) != 'G' || dcn_ins_char(1, 1) != 'N')
        return fail("dcn_ins_char", 0);
    if (winner_checks(rng)) return 1;

    const char letters[5] = {'A', 'C', 'G', 'T', 'N'};
    size_t lists = 0, events_seen = 0;
    for (int round = 0; round < 4000; ++round) {
        uint32_t count = 1 + rng() % 12, i_len = 0;
        int first_op = -1, last_op = -1, i_at = -1;
        const uint32_t special[4] = {63, 64, 65, 129}, lens[4] = {1, 63, 64, 65};
        if (round % 10 == 1) count = special[(round / 10) % 4];
        if (round % 10 == 2) i_at = (int)(rng() % count), i_len = lens[(round / 10) % 4];
        if (round % 10 == 3) first_op = (int)DCN_ALN_I;
        if (round % 10 == 4) last_op = (int)DCN_ALN_I;
        if (round % 10 == 5) first_op = last_op = (int)DCN_ALN_I, count = 2 + rng() % 70;
        if (round % 10 == 6) count = 66 + rng() % 70, i_at = 63, i_len = lens[(round / 10) % 4]; // an I run as the 64th run
        if (round % 10 == 7) count = 66 + rng() % 70, i_at = 64, i_len = lens[(round / 10) % 4]; // ... and as the 65th
        const std::vector<uint32_t> runs = make_runs(rng, count, first_op, last_op, i_at, i_len);
        if (i_at >= 0 && first_op < 0 && (runs[(size_t)i_at] & 15u) != DCN_ALN_I) return fail("the planted I run is not there", lists);
        uint32_t m = 0, n = 0;
        for (const uint32_t x : runs) m += dcn_pile_step_s(x), n += dcn_pile_step_t(x);
        std::string s(m, 'A');
        for (auto &c : s) c = letters[rng() % 5];
        const uint64_t t0 = 1000 + rng() % 1000;
        for (uint32_t reverse = 0; reverse < 2; ++reverse) {
            const std::vector<plain_event> want = step_walk(runs, s, reverse, t0);
            // the counting pass: 64 lanes stride over the runs
            uint32_t n_events = 0, n_bases = 0;
            for (uint32_t lane = 0; lane < 64; ++lane)
                for (uint32_t r = lane; r < runs.size(); r += 64) n_events += dcn_ins_run_events(runs[r]), n_bases += dcn_ins_run_bases(runs[r]);
            size_t want_bases = 0;
            for (const auto &e : want) want_bases += e.len;
            if (n_events != want.size() || n_bases != want_bases) return fail("the counting pass differs from the step-by-step walk", lists);
            // arrays of exactly the counted size between guards; the ledger already holds event0 events and base0 bases
            const uint64_t event0 = rng() % 3, base0 = rng() % 7;
            std::vector<uint8_t> ev_mem(2 * GUARD + (event0 + n_events) * sizeof(dcn_ins_event), GUARD_BYTE), base_mem(2 * GUARD + base0 + n_bases, GUARD_BYTE);
            std::vector<uint8_t> ev_before = ev_mem, base_before = base_mem;
            dcn_ins_event *const events = reinterpret_cast<dcn_ins_event *>(ev_mem.data() + GUARD);
            uint8_t *const bases = base_mem.data() + GUARD;
            bool inside = true;
            const auto char_of = [&](uint32_t i) -> uint8_t {
                if (i >= m) {
                    inside = false;
                    return 'N';
                }
                return (uint8_t)s[i];
            };
            uint32_t i0 = 0, j0 = 0;
            uint64_t event_at = event0, base_at = base0;
            const uint32_t total = (uint32_t)runs.size();
            for (uint32_t c0 = 0; c0 < total; c0 += 64) {
                const uint32_t here = total - c0 < 64 ? total - c0 : 64;
                uint32_t my_i[64], my_j[64], si = 0, sj = 0, se = 0, sb = 0;
                uint64_t my_e[64], my_b[64];
                for (uint32_t r = 0; r < here; ++r) { // the exclusive prefix of the chunk's steps
                    my_i[r] = i0 + si, my_j[r] = j0 + sj, my_e[r] = event_at + se, my_b[r] = base_at + sb;
                    si += dcn_pile_step_s(runs[c0 + r]), sj += dcn_pile_step_t(runs[c0 + r]);
                    se += dcn_ins_run_events(runs[c0 + r]), sb += dcn_ins_run_bases(runs[c0 + r]);
                }
                for (uint32_t r = 0; r < here; ++r) {
                    if (!dcn_ins_run_events(runs[c0 + r])) continue;
                    if (my_e[r] >= event0 + n_events || my_b[r] + (runs[c0 + r] >> 4) > base0 + n_bases) return fail("a run past the counted size", lists);
                    for (uint32_t lane = 0; lane < 64; ++lane)
                        dcn_ins_write_run(runs[c0 + r], my_i[r], my_j[r], reverse, t0, my_e[r], my_b[r], lane, 64u, char_of, events, bases);
                }
                i0 += si, j0 += sj, event_at += se, base_at += sb;
            }
            if (!inside || i0 != m || j0 != n || event_at != event0 + n_events || base_at != base0 + n_bases)
                return fail("a base outside S, or the steps do not sum up", lists);
            if (memcmp(ev_mem.data(), ev_before.data(), GUARD + event0 * sizeof(dcn_ins_event)) != 0 ||
                memcmp(ev_mem.data() + ev_mem.size() - GUARD, ev_before.data() + ev_mem.size() - GUARD, GUARD) != 0 ||
                memcmp(base_mem.data(), base_before.data(), GUARD + base0) != 0 ||
                memcmp(base_mem.data() + base_mem.size() - GUARD, base_before.data() + base_mem.size() - GUARD, GUARD) != 0)
                return fail("a guard, or what the ledger held before, was written", lists);
            uint64_t at = base0;
            for (size_t e = 0; e < want.size(); ++e) { // a row's events lie in run order, their bases densely behind each other
                dcn_ins_event got;
                memcpy(&got, ev_mem.data() + GUARD + (event0 + e) * sizeof(dcn_ins_event), sizeof(got));
                const uint32_t flags = (want[e].front ? DCN_INS_FRONT : 0u) | (reverse ? DCN_INS_REVERSE : 0u);
                if (got.base != want[e].base || got.len != want[e].len || got.flags != flags || got.bases_offset != at ||
                    memcmp(bases + at, want[e].bases.data(), got.len) != 0)
                    return fail("an event differs from the step-by-step walk", lists);
                for (uint32_t q = 0; q < got.len; ++q)
                    if (!strchr("ACGTN", bases[at + q])) return fail("a byte that is no base", lists);
                at += got.len;
            }
            events_seen += want.size();
        }
        ++lists;
    }
    std::printf("insertion walk ok: %zu run lists, %zu events\n", lists, events_seen);
    return 0;
}

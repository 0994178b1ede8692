// pileup_walk_test.cpp -- the run walk of the pileup kernel (dcn_pileup.h) on the host, under the address and
// undefined-behaviour sanitizers (tests/test_pileup_abi.py builds and runs it).  The kernel's shape is kept: the runs in
// chunks of 64, each run's (i, j) from the prefix sum of the chunk's steps (emulated serially here) on top of where the
// chunk begins, then dcn_pile_run for every run by each of 64 lanes.  The adds go into an array of exactly n positions
// with guard words on both sides, and are compared with a walk step by step by rule P3.  dcn_pile_index and
// dcn_pile_call are checked on the way.
#include "dcn_pileup.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

namespace {

constexpr uint32_t GUARD = 0xC0FFEEu, GUARD_WORDS = 16;

int fail(const char *what, size_t list) {
    std::fprintf(stderr, "run list %zu: %s\n", list, what);
    return 1;
}

// rule P3 step by step: counts[8 * j + column]
void step_walk(const std::vector<uint32_t> &runs, const std::vector<uint8_t> &s_columns, uint32_t reverse, std::vector<uint32_t> &counts) {
    uint32_t i = 0, j = 0;
    for (const uint32_t run : runs) {
        const uint32_t op = run & 15u, len = run >> 4;
        if (op == DCN_ALN_I) {
            counts[8 * (j > 0 ? j - 1 : 0) + DCN_PILE_INS] += 1;
            i += len;
            continue;
        }
        for (uint32_t q = 0; q < len; ++q) {
            counts[8 * j + (op == DCN_ALN_D ? DCN_PILE_DEL : s_columns[i])] += 1;
            if (op != DCN_ALN_D) ++i;
            if (reverse) counts[8 * j + DCN_PILE_REV] += 1;
            ++j;
        }
    }
}

// the kernel's walk; -> false when an add fell outside [0, n) or a base outside [0, m)
bool lane_walk(const std::vector<uint32_t> &runs, const std::vector<uint8_t> &s_columns, uint32_t n, uint32_t reverse,
               std::vector<uint32_t> &guarded) {
    bool inside = true;
    const uint32_t m = (uint32_t)s_columns.size();
    const auto column_of = [&](uint32_t i) -> uint32_t {
        if (i >= m) {
            inside = false;
            return DCN_PILE_N;
        }
        return s_columns[i];
    };
    const auto add = [&](uint32_t column, uint32_t j) {
        if (j >= n || column >= DCN_PILE_COLUMNS) inside = false;
        else guarded[GUARD_WORDS + 8 * (size_t)j + column] += 1;
    };
    uint32_t i0 = 0, j0 = 0;
    const uint32_t count = (uint32_t)runs.size();
    for (uint32_t c0 = 0; c0 < count; c0 += 64) {
        const uint32_t here = count - c0 < 64 ? count - c0 : 64;
        uint32_t my_i[64], my_j[64], si = 0, sj = 0;
        for (uint32_t r = 0; r < here; ++r) { // the exclusive prefix of the chunk's steps
            my_i[r] = i0 + si;
            my_j[r] = j0 + sj;
            si += dcn_pile_step_s(runs[c0 + r]);
            sj += dcn_pile_step_t(runs[c0 + r]);
        }
        for (uint32_t r = 0; r < here; ++r)
            for (uint32_t lane = 0; lane < 64; ++lane) dcn_pile_run(runs[c0 + r], my_i[r], my_j[r], reverse, lane, 64u, column_of, add);
        i0 += si;
        j0 += sj;
    }
    return inside && i0 == m && j0 == n;
}

// a list of `count` runs with no equal neighbours; n > 0 is seen to
std::vector<uint32_t> make_runs(std::mt19937 &rng, uint32_t count, int first_op, int last_op, uint32_t fixed_len) {
    const uint32_t ops[4] = {DCN_ALN_EQ, DCN_ALN_X, DCN_ALN_I, DCN_ALN_D};
    std::vector<uint32_t> runs;
    uint32_t prev = 99;
    for (uint32_t r = 0; r < count; ++r) {
        uint32_t op;
        do op = ops[rng() % 4];
        while (op == prev);
        if (r == 0 && first_op >= 0) op = (uint32_t)first_op;
        if (r == count - 1 && last_op >= 0 && (uint32_t)last_op != prev) op = (uint32_t)last_op;
        if (op == prev) op = op == DCN_ALN_EQ ? DCN_ALN_X : DCN_ALN_EQ;
        const uint32_t len = fixed_len ? fixed_len : 1 + (rng() % 8 == 0 ? rng() % 130 : rng() % 5);
        runs.push_back(len << 4 | op);
        prev = op;
    }
    bool any_t = false;
    for (const uint32_t x : runs) any_t = any_t || dcn_pile_step_t(x) > 0;
    if (!any_t) runs.push_back(3u << 4 | ((runs.back() & 15u) == DCN_ALN_EQ ? DCN_ALN_D : DCN_ALN_EQ));
    return runs;
}

} // namespace

int main() {
    std::mt19937 rng(1501);
    // where a counter lies: every (column, base) of a small pileup has a word of its own inside the allocation
    {
        const uint64_t bases = 96;
        std::vector<int> seen(bases * DCN_PILE_COLUMNS, 0);
        for (uint32_t c = 0; c < DCN_PILE_COLUMNS; ++c)
            for (uint64_t b = 0; b < bases; ++b) {
                const uint64_t at = dcn_pile_index(c, b, bases);
                if (at >= seen.size() || seen[at]++) return fail("dcn_pile_index is not one to one", 0);
            }
    }
    if (dcn_pile_column(0, 0) != DCN_PILE_A || dcn_pile_column(1, 0) != DCN_PILE_C || dcn_pile_column(2, 0) != DCN_PILE_T ||
        dcn_pile_column(3, 0) != DCN_PILE_G || dcn_pile_column(2, 1) != DCN_PILE_N)
        return fail("dcn_pile_column", 0);
    {
        const uint32_t tie[7] = {2, 2, 0, 0, 0, 0, 0}, del[7] = {1, 0, 0, 0, 0, 3, 4};
        if (dcn_pile_call(tie, DCN_PILE_C, 3, 500) != (1u | 0u << 8 | 1u << 16)) return fail("a tie A = C calls A", 0);
        if (dcn_pile_call(del, DCN_PILE_N, 3, 750) != (2u | 4u | 4u << 8 | 7u << 16)) return fail("a DEL majority with an INS flag", 0);
        if (dcn_pile_call(tie, DCN_PILE_A, 5, 500) != (7u << 8)) return fail("depth below min_depth", 0);
    }

    size_t lists = 0;
    for (int round = 0; round < 4000; ++round) {
        uint32_t count = 1 + rng() % 12, fixed_len = 0;
        int first_op = -1, last_op = -1;
        const uint32_t special[4] = {63, 64, 65, 129}, lens[3] = {63, 64, 65};
        if (round % 10 == 1) count = special[(round / 10) % 4];
        if (round % 10 == 2) fixed_len = lens[(round / 10) % 3];
        if (round % 10 == 3) first_op = (int)DCN_ALN_I;
        if (round % 10 == 4) last_op = (int)DCN_ALN_I;
        if (round % 10 == 5) first_op = last_op = (int)DCN_ALN_I, count = 2 + rng() % 70;
        const std::vector<uint32_t> runs = make_runs(rng, count, first_op, last_op, fixed_len);
        uint32_t m = 0, n = 0;
        for (const uint32_t x : runs) m += dcn_pile_step_s(x), n += dcn_pile_step_t(x);
        std::vector<uint8_t> s_columns(m);
        for (auto &c : s_columns) c = (uint8_t)(rng() % 5); // A C G T N
        for (uint32_t reverse = 0; reverse < 2; ++reverse) {
            std::vector<uint32_t> want(8 * (size_t)n, 0), guarded(2 * GUARD_WORDS + 8 * (size_t)n, 0);
            for (uint32_t g = 0; g < GUARD_WORDS; ++g) guarded[g] = guarded[guarded.size() - 1 - g] = GUARD;
            step_walk(runs, s_columns, reverse, want);
            if (!lane_walk(runs, s_columns, n, reverse, guarded)) return fail("an add outside T, a base outside S, or the steps do not sum to (m, n)", lists);
            for (uint32_t g = 0; g < GUARD_WORDS; ++g)
                if (guarded[g] != GUARD || guarded[guarded.size() - 1 - g] != GUARD) return fail("a guard word was written", lists);
            for (size_t q = 0; q < want.size(); ++q)
                if (guarded[GUARD_WORDS + q] != want[q]) return fail("the counts differ from the step-by-step walk", lists);
            for (uint32_t j = 0; j < n; ++j) { // rule P4: one add among columns 0-5 per position
                uint32_t depth = 0;
                for (uint32_t c = 0; c <= DCN_PILE_DEL; ++c) depth += want[8 * (size_t)j + c];
                if (depth != 1 || want[8 * (size_t)j + DCN_PILE_REV] != reverse) return fail("rule P4", lists);
            }
        }
        ++lists;
    }
    std::printf("pileup walk ok: %zu run lists\n", lists);
    return 0;
}

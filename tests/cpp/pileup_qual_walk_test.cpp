// pileup_qual_walk_test.cpp -- the quality walk of the pileup kernel (dcn_pileup.h: dcn_pile_run_qual and rules Q2 - Q4's
// arithmetic) on the host, under the address and undefined-behaviour sanitizers (tests/test_pileup_qual_abi.py builds and
// runs it).  The kernel's shape is kept, as in pileup_walk_test.cpp: the runs in chunks of 64, each run's (i, j) from the
// prefix of the chunk's steps (serially here), then dcn_pile_run_qual for every run by each of 64 lanes, with the kernel's
// guards i < m and j < n.  Counters and sums go into arrays of exactly n positions between guard words; the qualities are
// read from an array of exactly the batch's bytes between guard bytes, at dcn_pile_qual_pos.  All of it is compared with a
// walk step by step over S's own qualities, which knows nothing of batch positions.
#include "dcn_pileup.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

namespace {

constexpr uint32_t GUARD = 0xC0FFEEu, GUARD_WORDS = 16, GUARD_BYTES = 64;
constexpr uint8_t GUARD_BYTE = 0xEE; // (as a quality it would show in every sum)

int fail(const char *what, size_t list) {
    std::fprintf(stderr, "run list %zu: %s\n", list, what);
    return 1;
}

// rules P3, Q3 and Q4 step by step: counts[8 * j + column], sums[4 * j + column]; s_q[i] = q(S[i])
void step_walk(const std::vector<uint32_t> &runs, const std::vector<uint8_t> &s_columns, const std::vector<uint32_t> &s_q, uint32_t reverse,
               uint32_t min_base_qual, std::vector<uint32_t> &counts, std::vector<uint32_t> &sums) {
    uint32_t i = 0, j = 0;
    for (const uint32_t run : runs) {
        const uint32_t op = run & 15u, len = run >> 4;
        if (op == DCN_ALN_I) {
            counts[8 * (j > 0 ? j - 1 : 0) + DCN_PILE_INS] += 1;
            i += len;
            continue;
        }
        for (uint32_t q = 0; q < len; ++q) {
            if (op == DCN_ALN_D) {
                counts[8 * j + DCN_PILE_DEL] += 1;
            } else {
                const bool base = s_columns[i] < 4, good = s_q[i] >= min_base_qual;
                counts[8 * j + (base && !good ? DCN_PILE_N : s_columns[i])] += 1;
                if (base && good) sums[4 * j + s_columns[i]] += s_q[i];
                ++i;
            }
            if (reverse) counts[8 * j + DCN_PILE_REV] += 1;
            ++j;
        }
    }
}

struct batch_quals {
    std::vector<uint8_t> guarded; // GUARD_BYTES, the batch's bytes, GUARD_BYTES
    int64_t n_bases, s_origin;
    const uint8_t *bytes() const { return guarded.data() + GUARD_BYTES; }
};

// the kernel's walk; -> false when an add fell outside [0, n), a base outside [0, m) or a quality outside the batch
bool lane_walk(const std::vector<uint32_t> &runs, const std::vector<uint8_t> &s_columns, const batch_quals &bq, uint32_t n, uint32_t reverse,
               uint32_t qual_offset, uint32_t min_base_qual, bool keep_sums, std::vector<uint32_t> &guarded, std::vector<uint32_t> &guarded_sums) {
    bool inside = true;
    const uint32_t m = (uint32_t)s_columns.size();
    const auto column_of = [&](uint32_t i) -> uint32_t {
        if (i >= m) {
            inside = false;
            return DCN_PILE_N;
        }
        return s_columns[i];
    };
    const auto quality_of = [&](uint32_t i) -> uint32_t {
        if (i >= m) {
            inside = false;
            return 0u;
        }
        const int64_t at = dcn_pile_qual_pos(bq.s_origin, reverse, i);
        if (at < 0 || at >= bq.n_bases) inside = false; // (the load below then reads a guard byte, and the sums show it)
        return dcn_pile_quality(bq.bytes()[at], qual_offset);
    };
    const auto add = [&](uint32_t column, uint32_t j) {
        if (j >= n || column >= DCN_PILE_COLUMNS) inside = false;
        else guarded[GUARD_WORDS + 8 * (size_t)j + column] += 1;
    };
    const auto add_sum = [&](uint32_t column, uint32_t j, uint32_t q) {
        if (!keep_sums) return;
        if (j >= n || column >= DCN_PILE_SUM_COLUMNS) inside = false;
        else guarded_sums[GUARD_WORDS + 4 * (size_t)j + column] += q;
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
            for (uint32_t lane = 0; lane < 64; ++lane)
                dcn_pile_run_qual(runs[c0 + r], my_i[r], my_j[r], reverse, min_base_qual, lane, 64u, column_of, quality_of, add, add_sum);
        i0 += si;
        j0 += sj;
    }
    return inside && i0 == m && j0 == n;
}

// a list of `count` runs with no equal neighbours; n > 0 is seen to
std::vector<uint32_t> make_runs(std::mt19937 &rng, uint32_t count, uint32_t fixed_len) {
    const uint32_t ops[4] = {DCN_ALN_EQ, DCN_ALN_X, DCN_ALN_I, DCN_ALN_D};
    std::vector<uint32_t> runs;
    uint32_t prev = 99;
    for (uint32_t r = 0; r < count; ++r) {
        uint32_t op;
        do op = ops[rng() % 4];
        while (op == prev);
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
    std::mt19937 rng(1801);
    // rule Q2: a byte below the offset is quality 0, byte 255 at offset 0 is 255
    if (dcn_pile_quality(33, 33) != 0 || dcn_pile_quality(32, 33) != 0 || dcn_pile_quality(0, 33) != 0 || dcn_pile_quality(73, 33) != 40 ||
        dcn_pile_quality(255, 33) != 222 || dcn_pile_quality(255, 0) != 255 || dcn_pile_quality(254, 255) != 0)
        return fail("dcn_pile_quality", 0);
    // rule Q3: only a base column falls, and only below the threshold
    for (uint32_t c = 0; c < DCN_PILE_COLUMNS; ++c) {
        if (dcn_pile_qual_column(c, 19, 20) != (c <= DCN_PILE_T ? DCN_PILE_N : c) || dcn_pile_qual_column(c, 20, 20) != c) return fail("dcn_pile_qual_column", 0);
        if (dcn_pile_qual_column(c, 0, 0) != c || dcn_pile_qual_column(c, 254, 255) != (c <= DCN_PILE_T ? DCN_PILE_N : c) || dcn_pile_qual_column(c, 255, 255) != c)
            return fail("dcn_pile_qual_column at thresholds 0 and 255", 0);
    }
    if (dcn_pile_qual_pos(100, 0, 0) != 100 || dcn_pile_qual_pos(100, 0, 7) != 107 || dcn_pile_qual_pos(100, 1, 0) != 99 || dcn_pile_qual_pos(100, 1, 99) != 0)
        return fail("dcn_pile_qual_pos", 0);
    { // where a sum lies: every (column, base) has a word of its own inside the allocation
        const uint64_t bases = 96;
        std::vector<int> seen(bases * DCN_PILE_SUM_COLUMNS, 0);
        for (uint32_t c = 0; c < DCN_PILE_SUM_COLUMNS; ++c)
            for (uint64_t b = 0; b < bases; ++b) {
                const uint64_t at = dcn_pile_sum_index(c, b, bases);
                if (at >= seen.size() || seen[at]++) return fail("dcn_pile_sum_index is not one to one", 0);
            }
    }

    size_t lists = 0;
    for (int round = 0; round < 4000; ++round) {
        uint32_t count = 1 + rng() % 12, fixed_len = 0;
        const uint32_t special[4] = {63, 64, 65, 129}, lens[3] = {63, 64, 65};
        if (round % 10 == 1) count = special[(round / 10) % 4];
        if (round % 10 == 2) fixed_len = lens[(round / 10) % 3];
        const std::vector<uint32_t> runs = make_runs(rng, count, fixed_len);
        uint32_t m = 0, n = 0;
        for (const uint32_t x : runs) m += dcn_pile_step_s(x), n += dcn_pile_step_t(x);
        std::vector<uint8_t> s_columns(m);
        for (auto &c : s_columns) c = (uint8_t)(rng() % 5); // A C G T N
        const uint32_t offsets[4] = {33, 33, 0, 64}, thresholds[6] = {20, 0, 255, 1, 41, 20};
        const uint32_t qual_offset = offsets[round % 4], min_base_qual = thresholds[round % 6];
        std::vector<uint8_t> s_bytes(m); // the quality byte of S[i]: mostly 0 .. 41 above the offset, some below it, some up to 255
        for (auto &b : s_bytes) b = (uint8_t)(rng() % 16 == 0 ? rng() % 256 : qual_offset + rng() % 42);
        std::vector<uint32_t> s_q(m);
        for (uint32_t i = 0; i < m; ++i) s_q[i] = s_bytes[i] >= qual_offset ? s_bytes[i] - qual_offset : 0u; // rule Q2, restated
        const uint32_t pre = round % 3 == 0 ? 0 : rng() % 40, post = round % 3 == 1 ? 0 : rng() % 40; // (the read interval inside its batch)
        for (uint32_t reverse = 0; reverse < 2; ++reverse) {
            batch_quals bq;
            bq.n_bases = (int64_t)pre + m + post;
            bq.s_origin = reverse ? (int64_t)pre + m : (int64_t)pre;
            bq.guarded.assign(2 * GUARD_BYTES + (size_t)bq.n_bases, GUARD_BYTE);
            for (int64_t b = 0; b < bq.n_bases; ++b) bq.guarded[GUARD_BYTES + (size_t)b] = (uint8_t)(rng() % 256);
            for (uint32_t i = 0; i < m; ++i) bq.guarded[GUARD_BYTES + pre + (reverse ? m - 1 - i : i)] = s_bytes[i]; // (not complemented, only turned)
            for (int keep = 0; keep < 2; ++keep) {
                std::vector<uint32_t> want(8 * (size_t)n, 0), want_sums(4 * (size_t)n, 0);
                std::vector<uint32_t> guarded(2 * GUARD_WORDS + 8 * (size_t)n, 0), guarded_sums(2 * GUARD_WORDS + 4 * (size_t)n, 0);
                for (uint32_t g = 0; g < GUARD_WORDS; ++g)
                    guarded[g] = guarded[guarded.size() - 1 - g] = guarded_sums[g] = guarded_sums[guarded_sums.size() - 1 - g] = GUARD;
                step_walk(runs, s_columns, s_q, reverse, min_base_qual, want, want_sums);
                if (!keep) want_sums.assign(want_sums.size(), 0);
                if (!lane_walk(runs, s_columns, bq, n, reverse, qual_offset, min_base_qual, keep != 0, guarded, guarded_sums))
                    return fail("an add outside T, a base outside S, a quality outside the batch, or the steps do not sum to (m, n)", lists);
                for (uint32_t g = 0; g < GUARD_WORDS; ++g)
                    if (guarded[g] != GUARD || guarded[guarded.size() - 1 - g] != GUARD || guarded_sums[g] != GUARD ||
                        guarded_sums[guarded_sums.size() - 1 - g] != GUARD)
                        return fail("a guard word was written", lists);
                for (size_t q = 0; q < want.size(); ++q)
                    if (guarded[GUARD_WORDS + q] != want[q]) return fail("the counts differ from the step-by-step walk", lists);
                for (size_t q = 0; q < want_sums.size(); ++q)
                    if (guarded_sums[GUARD_WORDS + q] != want_sums[q]) return fail("the sums differ from the step-by-step walk", lists);
                for (uint32_t j = 0; j < n; ++j) { // rule P4 holds unchanged: one add among columns 0-5 per position
                    uint32_t depth = 0;
                    for (uint32_t c = 0; c <= DCN_PILE_DEL; ++c) depth += want[8 * (size_t)j + c];
                    if (depth != 1 || want[8 * (size_t)j + DCN_PILE_REV] != reverse) return fail("rule P4", lists);
                }
            }
            if (min_base_qual == 0) { // rule Q3: with threshold 0 the counters are dcn_pile_run's
                std::vector<uint32_t> plain(8 * (size_t)n, 0), with_q(2 * GUARD_WORDS + 8 * (size_t)n, 0), none(2 * GUARD_WORDS + 4 * (size_t)n, 0);
                const auto column_of = [&](uint32_t i) -> uint32_t { return s_columns[i]; };
                const auto add = [&](uint32_t column, uint32_t j) { plain[8 * (size_t)j + column] += 1; };
                uint32_t i = 0, j = 0;
                for (const uint32_t run : runs) {
                    for (uint32_t lane = 0; lane < 64; ++lane) dcn_pile_run(run, i, j, reverse, lane, 64u, column_of, add);
                    i += dcn_pile_step_s(run), j += dcn_pile_step_t(run);
                }
                if (!lane_walk(runs, s_columns, bq, n, reverse, qual_offset, 0, false, with_q, none)) return fail("threshold 0", lists);
                for (size_t q = 0; q < plain.size(); ++q)
                    if (with_q[GUARD_WORDS + q] != plain[q]) return fail("threshold 0 differs from dcn_pile_run", lists);
            }
        }
        ++lists;
    }
    std::printf("pileup quality walk ok: %zu run lists\n", lists);
    return 0;
}

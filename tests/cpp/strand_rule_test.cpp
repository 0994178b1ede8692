// strand_rule_test.cpp -- rules S2 - S6 of THE DEFINITION OF STRAND EVIDENCE on the host, under the address and
// undefined-behaviour sanitizers (tests/test_strand_abi.py builds and runs it).  dcn_strand.h against a brute force that
// computes rule S5 with unsigned __int128 and, for m < 1024, without the shift; rows written by hand; and the walk of the
// pileup kernel with rule S2's callback (dcn_pileup.h: dcn_pile_run and dcn_pile_run_qual, in the kernel's shape as
// pileup_qual_walk_test.cpp keeps it) against a walk step by step, on rows with every run kind on both strands.
// Every table that is scored is also printed, "T a b c d max_sb min_alt min_depth -> sb flags", for the Python model of the
// GPU tests (tests/_strand_worker.py) to be checked against the same rows.
#include "dcn_pileup.h"
#include "dcn_strand.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

namespace {

constexpr uint32_t GUARD = 0xC0FFEEu, GUARD_WORDS = 16;

int fail(const char *what, size_t at) {
    std::fprintf(stderr, "case %zu: %s\n", at, what);
    return 1;
}

uint32_t bit_length(uint32_t m) {
    uint32_t n = 0;
    while (m) ++n, m >>= 1;
    return n;
}

// rule S5 as it reads, in 128 bits
uint32_t brute_score(uint32_t a0, uint32_t b0, uint32_t c0, uint32_t d0) {
    uint32_t m = a0;
    if (b0 > m) m = b0;
    if (c0 > m) m = c0;
    if (d0 > m) m = d0;
    const uint32_t s = m < 1024u ? 0u : bit_length(m) - 10u;
    const unsigned __int128 a = a0 >> s, b = b0 >> s, c = c0 >> s, d = d0 >> s;
    const unsigned __int128 N = a + b + c + d, r1 = a + b, r2 = c + d, c1 = a + c, c2 = b + d;
    if (r1 * r2 * c1 * c2 == 0) return 0;
    const unsigned __int128 ad = a * d, bc = b * c, diff = ad > bc ? ad - bc : bc - ad;
    const unsigned __int128 sb = 100 * N * diff * diff / (r1 * r2 * c1 * c2);
    return sb > 65535 ? 65535u : (uint32_t)sb;
}

// ... and without any shift, which must agree while m < 1024
uint32_t brute_score_unshifted(uint32_t a0, uint32_t b0, uint32_t c0, uint32_t d0) {
    const unsigned __int128 a = a0, b = b0, c = c0, d = d0;
    const unsigned __int128 den = (a + b) * (c + d) * (a + c) * (b + d);
    if (den == 0) return 0;
    const unsigned __int128 diff = a * d > b * c ? a * d - b * c : b * c - a * d;
    const unsigned __int128 sb = 100 * (a + b + c + d) * diff * diff / den;
    return sb > 65535 ? 65535u : (uint32_t)sb;
}

uint32_t brute_flags(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t sb, uint32_t max_sb, uint32_t min_alt, uint32_t min_depth) {
    uint32_t f = 0;
    if (max_sb > 0 && sb >= max_sb) f |= 1u;
    if ((c < d ? c : d) < min_alt && (unsigned __int128)a + c >= min_depth && (unsigned __int128)b + d >= min_depth) f |= 2u;
    return f;
}

size_t n_tables = 0;

// one table through dcn_strand.h and the brute force; prints the row
bool check_table(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t max_sb = 1083, uint32_t min_alt = 1, uint32_t min_depth = 3) {
    const dcn_strand_table t = {a, b, c, d};
    const dcn_strand_prm p = {max_sb, min_alt, min_depth};
    const uint32_t sb = dcn_strand_score(t), fl = dcn_strand_flags(t, sb, p);
    std::printf("T %u %u %u %u %u %u %u -> %u %u\n", a, b, c, d, max_sb, min_alt, min_depth, sb, fl);
    ++n_tables;
    if (sb != brute_score(a, b, c, d)) return false;
    const uint32_t m = std::max(std::max(a, b), std::max(c, d));
    if (m < 1024u && sb != brute_score_unshifted(a, b, c, d)) return false;
    return fl == brute_flags(a, b, c, d, sb, max_sb, min_alt, min_depth);
}

// a row written by hand: the score and the flags are stated
bool hand(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t want_sb, uint32_t want_flags, uint32_t max_sb = 1083, uint32_t min_alt = 1,
          uint32_t min_depth = 3) {
    const dcn_strand_table t = {a, b, c, d};
    const dcn_strand_prm p = {max_sb, min_alt, min_depth};
    const uint32_t sb = dcn_strand_score(t);
    return check_table(a, b, c, d, max_sb, min_alt, min_depth) && sb == want_sb && dcn_strand_flags(t, sb, p) == want_flags;
}

// ---- rule S2: the walk -------------------------------------------------------------------------------------------------
// step by step: counts[8 j + column], planes[4 j + column]; s_q[i] = q(S[i]) (with_quals: rule Q3's column)
void step_walk(const std::vector<uint32_t> &runs, const std::vector<uint8_t> &s_columns, const std::vector<uint32_t> &s_q, uint32_t reverse,
               bool with_quals, uint32_t min_base_qual, std::vector<uint32_t> &counts, std::vector<uint32_t> &planes) {
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
                uint32_t column = s_columns[i];
                if (with_quals && column < 4 && s_q[i] < min_base_qual) column = DCN_PILE_N;
                counts[8 * j + column] += 1;
                if (reverse && column < 4) planes[4 * j + column] += 1;
                ++i;
            }
            if (reverse) counts[8 * j + DCN_PILE_REV] += 1;
            ++j;
        }
    }
}

// the kernel's walk; -> false when an add fell outside [0, n), a base outside [0, m), or the strand add came on a forward row
bool lane_walk(const std::vector<uint32_t> &runs, const std::vector<uint8_t> &s_columns, const std::vector<uint32_t> &s_q, uint32_t n,
               uint32_t reverse, bool with_quals, uint32_t min_base_qual, bool keep_planes, std::vector<uint32_t> &guarded,
               std::vector<uint32_t> &guarded_planes) {
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
        return s_q[i];
    };
    const auto add = [&](uint32_t column, uint32_t j) {
        if (j >= n || column >= DCN_PILE_COLUMNS) inside = false;
        else guarded[GUARD_WORDS + 8 * (size_t)j + column] += 1;
    };
    const auto add_sum = [&](uint32_t, uint32_t, uint32_t) {};
    const auto add_strand = [&](uint32_t column, uint32_t j) {
        if (!reverse || j >= n || column >= DCN_PILE_STRAND_COLUMNS) inside = false;
        else guarded_planes[GUARD_WORDS + 4 * (size_t)j + column] += 1;
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
            for (uint32_t lane = 0; lane < 64; ++lane) {
                if (with_quals && keep_planes)
                    dcn_pile_run_qual(runs[c0 + r], my_i[r], my_j[r], reverse, min_base_qual, lane, 64u, column_of, quality_of, add, add_sum, add_strand);
                else if (with_quals)
                    dcn_pile_run_qual(runs[c0 + r], my_i[r], my_j[r], reverse, min_base_qual, lane, 64u, column_of, quality_of, add, add_sum);
                else if (keep_planes)
                    dcn_pile_run(runs[c0 + r], my_i[r], my_j[r], reverse, lane, 64u, column_of, add, add_strand);
                else
                    dcn_pile_run(runs[c0 + r], my_i[r], my_j[r], reverse, lane, 64u, column_of, add);
            }
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
    std::mt19937 rng(2301);
    // ---- rows written by hand ----
    // a zero margin: an empty reference row (hom-alt, S7), an empty allele row, an empty strand
    if (!hand(0, 0, 7, 9, 0, 0) || !hand(7, 9, 0, 0, 0, 2) || !hand(5, 0, 5, 0, 0, 0) || !hand(0, 0, 0, 0, 0, 0)) return fail("zero margin", 0);
    // 100 * 20 * (5*5 - 5*5)^2 = 0; a perfectly split table; the fully one-sided one: N (ad-bc)^2 / (r1 r2 c1 c2) = N -> 100 N
    if (!hand(5, 5, 5, 5, 0, 0) || !hand(10, 0, 0, 10, 2000, 3) || !hand(3, 3, 3, 0, 225, 2)) return fail("small tables", 1);
    // m = 1023: no shift.  a = d = 1023, b = c = 0: 100 * 2046 = 204600 -> the cap
    if (!hand(1023, 0, 0, 1023, 65535, 3) || !hand(1023, 1023, 1023, 1023, 0, 0)) return fail("m = 1023", 2);
    // m = 1024: s = 1, so 1 >> 1 = 0 and the table is (512, 0, 0, 512) / (512, 512, 0, 0)
    if (!hand(1024, 0, 0, 1024, 65535, 3) || !hand(1024, 1024, 1, 1, 0, 0) || !hand(1024, 1, 1, 1024, 65535, 1)) return fail("m = 1024", 3);
    // (1024, 3, 3, 1024) >> 1 = (512, 1, 1, 512): 100 * 1026 * (512 * 512 - 1)^2 / 513^4 is above 100,000: the cap; min(c, d) = 3
    if (!hand(1024, 3, 3, 1024, 65535, 1)) return fail("m = 1024, odd cells", 4);
    // m = 2^32 - 1: s = 22, every full cell becomes 1023; (1023, 1023, 1023, 0): 100 * 3069 * 1023^4 / (4 * 1023^4) = 76725: the cap
    if (!hand(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0) || !hand(0xFFFFFFFFu, 0, 0, 0xFFFFFFFFu, 65535, 3) ||
        !hand(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 65535, 3))
        return fail("m = 2^32 - 1", 5);
    // the cap: 100 N = 65500 at N = 655 passes under it, N = 656 is capped
    if (!hand(327, 0, 0, 328, 65500, 3) || !hand(328, 0, 0, 328, 65535, 3)) return fail("the cap", 6);
    // DCN_STRAND_BIAS on each side of its threshold, and switched off: (6, 6, 6, 1): 100 * 19 * (6 - 36)^2 / (12 * 7 * 12 * 7) = 242
    if (!hand(6, 6, 6, 1, 242, 0, 243) || !hand(6, 6, 6, 1, 242, 1, 242) || !hand(6, 6, 6, 1, 242, 0, 0) || !hand(10, 0, 0, 10, 2000, 2, 0))
        return fail("the bias flag", 7);
    // DCN_STRAND_ONE_SIDED on each side of its three thresholds (max_sb = 0 keeps the other flag out).
    // (4, 3, 2, 0): 100 * 9 * 36 / (7 * 2 * 6 * 3) = 128; (4, 3, 2, 1): 100 * 10 * 4 / (7 * 3 * 6 * 4) = 7
    if (!hand(4, 3, 2, 0, 128, 2, 0, 1, 3) || !hand(4, 3, 2, 1, 7, 0, 0, 1, 3) || !hand(4, 3, 2, 1, 7, 2, 0, 2, 3) || !hand(4, 2, 2, 0, 88, 0, 0, 1, 3) ||
        !hand(0, 3, 2, 0, 500, 0, 0, 1, 3) || !hand(1, 3, 2, 0, 300, 2, 0, 1, 3) || !hand(4, 3, 2, 0, 128, 0, 0, 0, 3) || !hand(4, 3, 2, 0, 128, 2, 0, 1, 0))
        return fail("the one-sided flag", 8);

    // ---- rule S5 against the brute force ----
    for (uint32_t a = 0; a < 7; ++a) // every table of cells 0 .. 6
        for (uint32_t b = 0; b < 7; ++b)
            for (uint32_t c = 0; c < 7; ++c)
                for (uint32_t d = 0; d < 7; ++d)
                    if (!check_table(a, b, c, d)) return fail("an exhaustive small table", a * 343 + b * 49 + c * 7 + d);
    for (int round = 0; round < 6000; ++round) {
        const uint32_t bits[4] = {4, 10, 11, 32};
        uint32_t x[4];
        for (auto &v : x) {
            const uint32_t k = bits[rng() % 4];
            v = (uint32_t)(rng() & (k == 32 ? 0xFFFFFFFFu : (1u << k) - 1u));
            if (rng() % 8 == 0) v = 0;
            if (rng() % 16 == 0) v = 1023u + rng() % 3;
        }
        if (!check_table(x[0], x[1], x[2], x[3], round % 3 == 0 ? 0u : 1u + rng() % 3000, rng() % 4, rng() % 12)) return fail("a random table", (size_t)round);
    }

    // ---- rules S3 and S4 ----
    {
        const uint32_t n[4] = {10, 20, 30, 40}, r[4] = {1, 2, 30, 0};
        for (uint32_t ref = 0; ref < 4; ++ref)
            for (uint32_t mask = 1; mask < 16; ++mask) {
                if (mask & (1u << ref)) continue;
                const dcn_strand_table t = dcn_strand_base_table(n[0], n[1], n[2], n[3], r[0], r[1], r[2], r[3], ref, mask);
                uint32_t c = 0, d = 0;
                for (uint32_t x = 0; x < 4; ++x)
                    if (mask & (1u << x)) c += n[x] - r[x], d += r[x];
                if (t.a != n[ref] - r[ref] || t.b != r[ref] || t.c != c || t.d != d) return fail("rule S3", ref * 16 + mask);
            }
        if (dcn_strand_forward(3, 5) != 0 || dcn_strand_forward(5, 3) != 2) return fail("F = n - R", 0);
        // depth 20, REV 8, the allele 6 times of which 2 reverse: d = 2, c = 4, b = 8 - 2, a = 12 - 4
        dcn_strand_table t = dcn_strand_indel_table(20, 8, 6, 2);
        if (t.a != 8 || t.b != 6 || t.c != 4 || t.d != 2) return fail("rule S4", 0);
        t = dcn_strand_indel_table(20, 1, 6, 2); // REV(p) < d: b = 0
        if (t.a != 15 || t.b != 0 || t.c != 4 || t.d != 2) return fail("rule S4, REV < d", 1);
        t = dcn_strand_indel_table(5, 2, 6, 1); // depth - REV < c: a = 0
        if (t.a != 0 || t.b != 1 || t.c != 5 || t.d != 1) return fail("rule S4, forward < c", 2);
        t = dcn_strand_indel_table(2, 5, 1, 1); // depth < REV(p): taken as 0
        if (t.a != 0 || t.b != 4 || t.c != 0 || t.d != 1) return fail("rule S4, depth < REV", 3);
    }
    { // where a reverse counter lies: every (column, base) has a word of its own inside the allocation
        const uint64_t bases = 96;
        std::vector<int> seen(bases * DCN_PILE_STRAND_COLUMNS, 0);
        for (uint32_t c = 0; c < DCN_PILE_STRAND_COLUMNS; ++c)
            for (uint64_t b = 0; b < bases; ++b) {
                const uint64_t at = dcn_pile_strand_index(c, b, bases);
                if (at >= seen.size() || seen[at]++) return fail("dcn_pile_strand_index is not one to one", 0);
            }
    }

    // ---- rule S2: the host walk with the callback ----
    size_t lists = 0, plane_adds = 0;
    for (int round = 0; round < 3000; ++round) {
        uint32_t count = 1 + rng() % 12, fixed_len = 0;
        const uint32_t special[4] = {63, 64, 65, 129}, lens[3] = {63, 64, 65};
        if (round % 10 == 1) count = special[(round / 10) % 4];
        if (round % 10 == 2) fixed_len = lens[(round / 10) % 3];
        const std::vector<uint32_t> runs = make_runs(rng, count, fixed_len);
        uint32_t m = 0, n = 0;
        for (const uint32_t x : runs) m += dcn_pile_step_s(x), n += dcn_pile_step_t(x);
        std::vector<uint8_t> s_columns(m);
        for (auto &c : s_columns) c = (uint8_t)(rng() % 5); // A C G T N
        std::vector<uint32_t> s_q(m);
        for (auto &q : s_q) q = rng() % 42;
        const uint32_t thresholds[4] = {20, 0, 41, 255}, min_base_qual = thresholds[round % 4];
        for (uint32_t reverse = 0; reverse < 2; ++reverse)
            for (int with_quals = 0; with_quals < 2; ++with_quals)
                for (int keep = 0; keep < 2; ++keep) {
                    std::vector<uint32_t> want(8 * (size_t)n, 0), want_planes(4 * (size_t)n, 0);
                    std::vector<uint32_t> guarded(2 * GUARD_WORDS + 8 * (size_t)n, 0), guarded_planes(2 * GUARD_WORDS + 4 * (size_t)n, 0);
                    for (uint32_t g = 0; g < GUARD_WORDS; ++g)
                        guarded[g] = guarded[guarded.size() - 1 - g] = guarded_planes[g] = guarded_planes[guarded_planes.size() - 1 - g] = GUARD;
                    step_walk(runs, s_columns, s_q, reverse, with_quals != 0, min_base_qual, want, want_planes);
                    if (!keep) want_planes.assign(want_planes.size(), 0); // (planes off: the walk it was, and nothing written)
                    if (!lane_walk(runs, s_columns, s_q, n, reverse, with_quals != 0, min_base_qual, keep != 0, guarded, guarded_planes))
                        return fail("an add outside T, a base outside S, a strand add on a forward row, or the steps do not sum to (m, n)", lists);
                    for (uint32_t g = 0; g < GUARD_WORDS; ++g)
                        if (guarded[g] != GUARD || guarded[guarded.size() - 1 - g] != GUARD || guarded_planes[g] != GUARD ||
                            guarded_planes[guarded_planes.size() - 1 - g] != GUARD)
                            return fail("a guard word was written", lists);
                    for (size_t q = 0; q < want.size(); ++q)
                        if (guarded[GUARD_WORDS + q] != want[q]) return fail("the counts differ from the step-by-step walk", lists);
                    for (size_t q = 0; q < want_planes.size(); ++q)
                        if (guarded_planes[GUARD_WORDS + q] != want_planes[q]) return fail("the planes differ from the step-by-step walk", lists);
                    for (uint32_t j = 0; j < n; ++j) { // rule S2's inequalities
                        uint32_t sum = 0;
                        for (uint32_t c = 0; c < 4; ++c) {
                            if (want_planes[4 * (size_t)j + c] > want[8 * (size_t)j + c]) return fail("R[c] <= n[c]", lists);
                            sum += want_planes[4 * (size_t)j + c];
                        }
                        if (sum > want[8 * (size_t)j + DCN_PILE_REV] || (!reverse && sum)) return fail("RA + RC + RG + RT <= REV", lists);
                        plane_adds += sum;
                    }
                }
        ++lists;
    }
    if (plane_adds < 10000) return fail("the walk added to no plane", 0);
    std::printf("strand rule ok: %zu tables, %zu run lists, %zu plane adds\n", n_tables, lists, plane_adds);
    return 0;
}

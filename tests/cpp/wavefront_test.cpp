// The wavefront step that verify.hip, align.hip and extend.hip share (csrc/dcn_wavefront.h: dcn_wf_diagonal over
// dcn_wf_match_run) compiled for the host under the address and undefined-behaviour sanitizers (tests/test_verify_abi.py
// builds and runs it).  The step is driven over all scores 0 .. E as verify_kernel drives it -- two arrays of exactly
// 2 E + 1 words, diagonal k at [k + E], swapped per score -- and compared with a full Levenshtein table: every F_s[k] is the
// last i with D[i][i + k] <= s, and the thresholded distance is the table's.
//   Both sequences lie in streams of exactly the words they need (packed_stream.h) between bases that continue the match: a
// run that ignored its limit would change F.  S is read forwards and backwards (reverse-complemented).  With one word in
// front of both streams the plain and the guarded load must return the same i for every (s, k); with no word in front, the
// guarded load alone runs, with origins inside the first 16 bases of the stream and both sides read backwards as well.
#include "dcn_wavefront.h"
#include "packed_stream.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

static int failures = 0;
#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            if (++failures < 20) {                \
                std::printf("FAIL %s: ", #cond);  \
                std::printf(__VA_ARGS__);         \
                std::printf("\n");                \
            }                                     \
        }                                         \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 11);
}

static bool valid(char c) { return std::string("ACGTacgt").find(c) != std::string::npos; }
static char comp(char c) {
    switch (c) {
    case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A';
    case 'a': return 't'; case 'c': return 'g'; case 'g': return 'c'; case 't': return 'a';
    default: return c;
    }
}
static bool equal(char a, char b) { return valid(a) && valid(b) && (a | 0x20) == (b | 0x20); }
static std::string revcomp(const std::string &s) {
    std::string r(s.rbegin(), s.rend());
    for (auto &c : r) c = comp(c);
    return r;
}

static std::string random_text(size_t n, int p_invalid) {
    std::string s(n, 'A');
    for (auto &c : s) {
        c = "ACGT"[rnd() & 3];
        if (rnd() % 100 < 10) c |= 0x20;
        if ((int)(rnd() % 100) < p_invalid) c = "NnR-"[rnd() % 4];
    }
    return s;
}

// `s` with about `percent` of its bases substituted, dropped or followed by an inserted base
static std::string mutated(const std::string &s, int percent) {
    std::string out;
    for (char c : s) {
        if ((int)(rnd() % 100) < percent) {
            const uint32_t kind = rnd() % 3;
            if (kind == 0) out += "ACGT"[rnd() & 3];
            else if (kind == 1) out += c, out += "ACGT"[rnd() & 3];
        } else {
            out += c;
        }
    }
    return out;
}

// a sequence between `before` and `after` in a stream of its own, read forwards or backwards
struct Side {
    PackedStream stream;
    dcn_wf_side side;
    Side(const std::string &before, const std::string &seq, const std::string &after, bool reverse, size_t front_words)
        : stream(reverse ? revcomp(before + seq + after) : before + seq + after, front_words, 1),
          side{stream.p(), stream.m(), (int64_t)(reverse ? after.size() + seq.size() : before.size()), reverse ? 1u : 0u} {}
};

constexpr uint32_t OVER = 0xFFFFFFFFu;
static long n_cells = 0, n_both = 0, n_found = 0, n_over = 0;

// The wavefront of S against T to the threshold E, as verify_kernel runs it; every F_s[k] against the table D.  `both`:
// the streams have a word in front, so the plain load is legal and must agree with the guarded one.
static void drive(const std::string &S, const std::string &T, const Side &s_side, const Side &t_side, int64_t E, bool both,
                  const std::vector<int64_t> &D, const char *what) {
    const int64_t m = (int64_t)S.size(), n = (int64_t)T.size(), k_end = n - m;
    const auto at = [&](int64_t i, int64_t j) { return D[(size_t)(i * (n + 1) + j)]; };
    const uint32_t want = at(m, n) <= E ? (uint32_t)at(m, n) : OVER;
    uint32_t result = OVER;
    if (k_end <= E && -k_end <= E) {
        std::vector<uint32_t> a((size_t)(2 * E + 1), 0xDEADBEEFu), b((size_t)(2 * E + 1), 0xDEADBEEFu); // exactly the two arrays
        uint32_t *prev = a.data(), *cur = b.data();
        for (int64_t s = 0; s <= E; ++s) {
            const int64_t lo = dcn_wf_max(-s, -m), hi = dcn_wf_min(s, n);
            bool found = false;
            for (int64_t k = lo; k <= hi; ++k) {
                const int64_t i = dcn_wf_diagonal<dcn_wf_guarded>(prev, E, s, k, m, n, s_side.side, t_side.side);
                if (both) {
                    const int64_t i_plain = dcn_wf_diagonal<dcn_wf_plain>(prev, E, s, k, m, n, s_side.side, t_side.side);
                    CHECK(i_plain == i, "%s m=%lld n=%lld s=%lld k=%lld: plain %lld, guarded %lld", what, (long long)m, (long long)n,
                          (long long)s, (long long)k, (long long)i_plain, (long long)i);
                    ++n_both;
                }
                int64_t f = dcn_wf_max(0, -k); // the last i of diagonal k with D <= s (D never falls along a diagonal)
                while (f + 1 <= m && f + 1 + k <= n && at(f + 1, f + 1 + k) <= s) ++f;
                CHECK(i == f && at(f, f + k) <= s, "%s m=%lld n=%lld E=%lld s=%lld k=%lld: F = %lld, the table says %lld", what,
                      (long long)m, (long long)n, (long long)E, (long long)s, (long long)k, (long long)i, (long long)f);
                cur[k + E] = (uint32_t)i;
                if (k == k_end && i >= m) found = true;
                ++n_cells;
            }
            if (found) {
                result = (uint32_t)s;
                break;
            }
            std::swap(prev, cur);
        }
    }
    CHECK(result == want, "%s m=%lld n=%lld E=%lld: distance %u, the table says %u", what, (long long)m, (long long)n, (long long)E,
          result, want);
    n_found += result != OVER;
    n_over += result == OVER;
}

// S against T between the contexts (before, after), which both sides share: at every threshold around |n - m| and d, S
// forwards and backwards, both loads where a front word makes the plain one legal, and the guarded one alone without
static void check(const std::string &before, const std::string &S, const std::string &T, const std::string &after_s,
                  const std::string &after_t) {
    const int64_t m = (int64_t)S.size(), n = (int64_t)T.size();
    std::vector<int64_t> D((size_t)((m + 1) * (n + 1)));
    const auto at = [&](int64_t i, int64_t j) -> int64_t & { return D[(size_t)(i * (n + 1) + j)]; };
    for (int64_t j = 0; j <= n; ++j) at(0, j) = j;
    for (int64_t i = 1; i <= m; ++i) {
        at(i, 0) = i;
        for (int64_t j = 1; j <= n; ++j)
            at(i, j) = std::min({at(i - 1, j - 1) + (equal(S[(size_t)i - 1], T[(size_t)j - 1]) ? 0 : 1), at(i - 1, j) + 1, at(i, j - 1) + 1});
    }
    const int64_t gap = m > n ? m - n : n - m, d = at(m, n);
    std::vector<int64_t> thresholds = {0, gap - 1, gap, gap + 1, d - 1, d, d + 1, d + 5};
    std::sort(thresholds.begin(), thresholds.end());
    thresholds.erase(std::unique(thresholds.begin(), thresholds.end()), thresholds.end());
    for (int reverse = 0; reverse < 2; ++reverse) {
        // a word in front of both streams: the plain load may run (S backwards reads up to 15 bases in front of its first)
        const Side s1(before, S, after_s, reverse != 0, 1), t1(before, T, after_t, false, 1);
        // no word in front: origins within the first 16 bases when the context is short; T backwards as well
        const Side s0(before, S, after_s, reverse != 0, 0), t0(before, T, after_t, false, 0), t0r(before, T, after_t, true, 0);
        for (int64_t E : thresholds) {
            if (E < 0) continue;
            drive(S, T, s1, t1, E, true, D, reverse ? "reverse, front word" : "forward, front word");
            drive(S, T, s0, t0, E, false, D, reverse ? "reverse, no front word" : "forward, no front word");
            drive(S, T, s0, t0r, E, false, D, reverse ? "both backwards, no front word" : "T backwards, no front word");
        }
    }
}

int main() {
    const size_t lengths[] = {0, 1, 15, 16, 17, 31, 32, 33, 47};
    for (int round = 0; round < 6; ++round)
        for (size_t m : lengths)
            for (size_t n : lengths) {
                if (round >= 2 && (m > n ? m - n : n - m) > 16) continue; // (far apart: twice is enough)
                const int p_invalid = round % 3 == 1 ? 6 : 0;
                std::string T = random_text(n, p_invalid), S;
                if (m == n) S = mutated(T, round * 5), S.resize(std::min(S.size(), m)), S += random_text(m - S.size(), 0);
                else if (m < n) S = T.substr(0, m); // S ends where T goes on ...
                else S = T + random_text(m - n, p_invalid);
                if (round % 2 && m) S[rnd() % m] = "ACGTN"[rnd() % 5];
                // the contexts: up to 15 bases in front (an origin within the first 16 bases of a stream without a front
                // word; none in front now and then), and behind S what T goes on with, so the match continues past S
                const std::string before = random_text(round == 0 ? 0 : rnd() % 16, 0);
                const std::string tail = random_text(rnd() % 16, 0);
                const std::string after_s = (m < n ? T.substr(m) : std::string()) + tail, after_t = (m > n ? S.substr(n) : std::string()) + tail;
                check(before, S, T, after_s, after_t);
            }
    // random pairs with mutations and invalid bases, any lengths up to 60
    for (int trial = 0; trial < 300; ++trial) {
        const std::string T = random_text(rnd() % 61, trial % 4 == 0 ? 5 : 0), S = mutated(T, (int)(rnd() % 5) * 6);
        const std::string before = random_text(rnd() % 16, 0), after = random_text(rnd() % 20, 0);
        check(before, S, T, after, after);
    }
    std::printf("%ld cells, %ld under both loads, %ld distances found, %ld over\n", n_cells, n_both, n_found, n_over);
    CHECK(n_cells > 100000 && n_both > 30000 && n_found > 1000 && n_over > 1000, "the cases do not cover what they are meant to");
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("wavefront ok\n");
    return 0;
}

// align_trace_test.cpp -- the walk back of the align kernel (dcn_align.h) on the host, under the address and
// undefined-behaviour sanitizers (tests/test_align_abi.py builds and runs it).  The kernels' own wavefront step
// (dcn_wavefront.h, the plain load) fills the triangular trace exactly as align.hip lays it out -- F_s[k] at s * s + k + s, (d + 1)^2 words, diagonals outside
// [max(-s, -m), min(s, n)] never touched (they hold a poison value) -- dcn_aln_traceback walks it into a slot of exactly
// 2 d + 1 runs, and every run is compared with a walk over the full table by rule A3 cell by cell.
#include "dcn_align.h"
#include "packed_stream.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

namespace {

bool equal_bases(char a, char b) { return a == b && a != 'N'; } // rule 2: an invalid base equals nothing

// rule A3 over the full table -> runs from the start of both intervals, and the distance
std::vector<uint32_t> table_walk(const std::string &S, const std::string &T, int64_t *d_out) {
    const int64_t m = (int64_t)S.size(), n = (int64_t)T.size();
    std::vector<int64_t> D((size_t)((m + 1) * (n + 1)));
    auto at = [&](int64_t i, int64_t j) -> int64_t & { return D[(size_t)(i * (n + 1) + j)]; };
    for (int64_t j = 0; j <= n; ++j) at(0, j) = j;
    for (int64_t i = 1; i <= m; ++i) {
        at(i, 0) = i;
        for (int64_t j = 1; j <= n; ++j)
            at(i, j) = std::min({at(i - 1, j - 1) + (equal_bases(S[(size_t)i - 1], T[(size_t)j - 1]) ? 0 : 1), at(i - 1, j) + 1, at(i, j - 1) + 1});
    }
    *d_out = at(m, n);
    std::vector<uint32_t> steps; // from the end
    int64_t i = m, j = n;
    while (i > 0 || j > 0) {
        const int64_t s = at(i, j);
        if (i > 0 && j > 0 && at(i - 1, j - 1) == s - 1) steps.push_back(DCN_ALN_X), --i, --j;
        else if (i > 0 && at(i - 1, j) == s - 1) steps.push_back(DCN_ALN_I), --i;
        else if (j > 0 && at(i, j - 1) == s - 1) steps.push_back(DCN_ALN_D), --j;
        else {
            if (!(i > 0 && j > 0 && equal_bases(S[(size_t)i - 1], T[(size_t)j - 1]) && at(i - 1, j - 1) == s)) {
                std::fprintf(stderr, "the table walk met a cell without a predecessor\n");
                std::exit(1);
            }
            steps.push_back(DCN_ALN_EQ), --i, --j;
        }
    }
    std::reverse(steps.begin(), steps.end());
    std::vector<uint32_t> runs;
    for (uint32_t op : steps) {
        if (!runs.empty() && (runs.back() & 15u) == op) runs.back() += 16u;
        else runs.push_back(16u | op);
    }
    return runs;
}

constexpr uint32_t POISON = 0xDEADBEEFu;

// the wavefront of verify.hip / align.hip (dcn_wf_diagonal of dcn_wavefront.h with the plain load, as the kernels call
// it, over both texts packed) -> the trace of exactly (d + 1)^2 words.  The wavefront of score s - 1 is read where the
// trace holds it: F_{s-1}[k] at trace[(s - 1)^2 + k + (s - 1)].
std::vector<uint32_t> wavefront_trace(const std::string &S, const std::string &T, int64_t d) {
    const int64_t m = (int64_t)S.size(), n = (int64_t)T.size();
    const PackedStream ps(S, 0, 1), pt(T, 0, 1); // (both read forwards: one word behind the last base)
    const dcn_wf_side side_s = {ps.p(), ps.m(), 0, 0u}, side_t = {pt.p(), pt.m(), 0, 0u};
    std::vector<uint32_t> trace((size_t)dcn_aln_trace_words((uint64_t)d), POISON);
    for (int64_t s = 0; s <= d; ++s) {
        const int64_t lo = std::max(-s, -m), hi = std::min(s, n);
        const uint32_t *const prev = s > 0 ? trace.data() + dcn_aln_trace_at(s - 1, 1 - s) : nullptr;
        bool found = false;
        for (int64_t k = lo; k <= hi; ++k) {
            const int64_t i = dcn_wf_diagonal<dcn_wf_plain>(prev, s - 1, s, k, m, n, side_s, side_t);
            if (i > m || i + k > n || i + k < 0) {
                std::fprintf(stderr, "a position outside the rectangle at s=%lld k=%lld\n", (long long)s, (long long)k);
                std::exit(1);
            }
            trace[(size_t)dcn_aln_trace_at(s, k)] = (uint32_t)i;
            if (k == n - m && i >= m) found = true;
        }
        if (found != (s == d)) {
            std::fprintf(stderr, "the wavefront ends at %lld, the table says %lld\n", (long long)s, (long long)d);
            std::exit(1);
        }
    }
    return trace;
}

uint64_t checked = 0;
std::vector<uint64_t> seen_d(2048, 0);

void check(const std::string &S, const std::string &T) {
    int64_t d = 0;
    const std::vector<uint32_t> want = table_walk(S, T, &d);
    const std::vector<uint32_t> trace = wavefront_trace(S, T, d);
    std::vector<uint32_t> slot((size_t)dcn_aln_ops_bound((uint64_t)d), POISON); // exactly the bound: a run past it is a sanitizer error
    const uint32_t n_ops = dcn_aln_traceback(trace.data(), (int64_t)S.size(), (int64_t)T.size(), d, slot.data() + slot.size());
    bool ok = n_ops == want.size() && n_ops <= slot.size();
    for (size_t q = 0; ok && q < want.size(); ++q) ok = slot[slot.size() - n_ops + q] == want[q];
    uint64_t cover_s = 0, cover_t = 0, edits = 0;
    for (uint32_t run : want) {
        const uint32_t op = run & 15u, len = run >> 4;
        if (op != DCN_ALN_D) cover_s += len;
        if (op != DCN_ALN_I) cover_t += len;
        if (op != DCN_ALN_EQ) edits += len;
    }
    ok = ok && cover_s == S.size() && cover_t == T.size() && edits == (uint64_t)d;
    if (!ok) {
        std::fprintf(stderr, "S=%s\nT=%s\nd=%lld n_ops=%u want %zu\n", S.c_str(), T.c_str(), (long long)d, n_ops, want.size());
        std::exit(1);
    }
    ++checked;
    ++seen_d[(size_t)std::min<int64_t>(d, 2047)];
}

std::string random_seq(std::mt19937_64 &rng, size_t len, const char *alphabet, size_t letters) {
    std::string s(len, 'A');
    for (char &c : s) c = alphabet[rng() % letters];
    return s;
}

// every base is, with probability rate, substituted, deleted or followed by an inserted base
std::string mutate(std::mt19937_64 &rng, const std::string &s, double rate, const char *alphabet, size_t letters) {
    std::string out;
    for (char c : s) {
        if ((double)(rng() % 1000000) / 1e6 < rate) {
            const unsigned kind = (unsigned)(rng() % 3);
            if (kind == 0) out += alphabet[rng() % letters];
            else if (kind == 1) out += c, out += alphabet[rng() % letters];
        } else out += c;
    }
    return out;
}

// T with exactly `count` substitutions spread evenly: d = count
std::string spaced_subs(const std::string &T, size_t count) {
    std::string s = T;
    for (size_t q = 0; q < count; ++q) {
        const size_t at = (2 * q + 1) * T.size() / (2 * count);
        s[at] = s[at] == 'A' ? 'C' : 'A';
    }
    return s;
}

} // namespace

int main() {
    std::mt19937_64 rng(1401);
    const struct { const char *letters; size_t n; } alphabets[] = {{"ACGT", 4}, {"ACGTN", 5}, {"AC", 2}};
    for (int round = 0; round < 4000; ++round) {
        const auto &a = alphabets[round % 3];
        const size_t len = (size_t)(rng() % 120);
        const std::string T = random_seq(rng, len, a.letters, a.n);
        const double rate = (double)(rng() % 30) / 100.0;
        check(mutate(rng, T, rate, a.letters, a.n), T);
        if (round % 10 == 0) check(random_seq(rng, (size_t)(rng() % 40), a.letters, a.n), T); // unrelated
        if (round % 50 == 0) check("", T), check(T, ""), check(T, T);
    }
    check("", "");
    // the scores at which a wave's lanes go round once more, and the s * s index around them
    const std::string T = random_seq(rng, 700, "ACGT", 4);
    for (size_t d : {0, 1, 31, 32, 33, 63, 64, 65}) {
        if (d) check(spaced_subs(T, d), T);
        check(T.substr(0, 700 - d), T);                         // a gap of d at the end
        check(T.substr(d), T);                                  // ... at the front
        check(T + random_seq(rng, d, "ACGT", 4), T);            // ... on the other side
        check(mutate(rng, T, (double)d / 700.0, "ACGT", 4), T); // mixed, d near that
    }
    for (size_t d : {0, 1, 31, 32, 33, 64, 65})
        if (!seen_d[d]) {
            std::fprintf(stderr, "no pair of distance %zu\n", d);
            return 1;
        }
    // hand-written pairs: one per tie-break of rule A3 (the same as tests/test_align_abi.py states for the model)
    check("AAAA", "AAA"), check("AAA", "AAAA"), check("AC", "CA"), check("ACGACGACG", "ACGACG"), check("N", "N");
    std::printf("align trace ok: %llu pairs\n", (unsigned long long)checked);
    return 0;
}

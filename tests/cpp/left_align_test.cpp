// left_align_test.cpp -- the left alignment of a row's runs (dcn_left_align.h) on the host, under the address and
// undefined-behaviour sanitizers (tests/test_left_align_abi.py builds and runs it).  The header's procedure, with the host's
// form of its reads, writes and comparisons and the two stacks in a heap array of exactly 2 d + 1 words, against rules
// N1 - N5 of include/deacon_hip.h taken literally: a list of columns in which a gap moves one step at a time.  Both texts
// are packed as the pack kernel leaves them, the read on either strand, at every offset within a word, with no word in
// front of the stream when the text begins at base 0 (the backward comparison looks up to 15 bases in front of a text).
#include "dcn_left_align.h"
#include "packed_stream.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

namespace {

bool equal_bases(char a, char b) { return a == b && a != 'N'; } // rule 2: an invalid base equals nothing

std::vector<uint32_t> runs_of(const std::vector<uint32_t> &cols) {
    std::vector<uint32_t> runs;
    for (uint32_t op : cols) {
        if (!runs.empty() && (runs.back() & 15u) == op) runs.back() += 16u;
        else runs.push_back(16u | op);
    }
    return runs;
}

std::vector<uint32_t> cols_of(const std::vector<uint32_t> &runs) {
    std::vector<uint32_t> cols;
    for (uint32_t run : runs) cols.insert(cols.end(), run >> 4, run & 15u);
    return cols;
}

// rule A3 over the full table -> the columns from the start of both intervals, and the distance
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
        else steps.push_back(DCN_ALN_EQ), --i, --j;
    }
    std::reverse(steps.begin(), steps.end());
    return steps;
}

struct totals {
    uint64_t shifted = 0, passed = 0, merged = 0;
    bool operator==(const totals &o) const { return shifted == o.shifted && passed == o.passed && merged == o.merged; }
};

bool is_gap(uint32_t op) { return op == DCN_ALN_I || op == DCN_ALN_D; }

// rules N1 - N4 on a list of columns, a step at a time
std::vector<uint32_t> brute(const std::string &S, const std::string &T, std::vector<uint32_t> cols, totals *tot) {
    size_t from = 0;
    for (;;) {
        size_t p = from;
        while (p < cols.size() && !is_gap(cols[p])) ++p;
        if (p == cols.size()) break;
        const uint32_t op = cols[p];
        size_t q = p;
        while (q < cols.size() && cols[q] == op) ++q;
        uint64_t steps = 0;
        for (;;) {
            if (p == 0) break; // first in the row
            if (cols[p - 1] == op) { // N4: directly behind a gap of its kind
                while (p > 0 && cols[p - 1] == op) --p;
                tot->merged += 1;
                continue;
            }
            if (is_gap(cols[p - 1])) break;
            if (p - 1 == 0) break; // the row's first column is not passed
            size_t i = 0, j = 0;
            for (size_t c = 0; c < p; ++c) i += cols[c] != DCN_ALN_D, j += cols[c] != DCN_ALN_I;
            const size_t len = q - p;
            const bool allowed = op == DCN_ALN_D ? equal_bases(T[j - 1], T[j + len - 1]) : equal_bases(S[i - 1], S[i + len - 1]);
            if (!allowed) break;
            const uint32_t c = cols[p - 1];
            cols.erase(cols.begin() + (long)(p - 1));
            cols.insert(cols.begin() + (long)(q - 1), c);
            --p, --q, ++steps;
        }
        tot->shifted += steps != 0;
        tot->passed += steps;
        from = q;
    }
    return cols;
}

// the columns are an alignment of S and T of cost d
bool valid(const std::string &S, const std::string &T, const std::vector<uint32_t> &cols, int64_t d) {
    size_t i = 0, j = 0;
    int64_t cost = 0;
    for (uint32_t op : cols) {
        if (op == DCN_ALN_EQ || op == DCN_ALN_X) {
            if (i >= S.size() || j >= T.size() || equal_bases(S[i], T[j]) != (op == DCN_ALN_EQ)) return false;
            ++i, ++j;
        } else if (op == DCN_ALN_I) ++i;
        else ++j;
        cost += op != DCN_ALN_EQ;
    }
    return i == S.size() && j == T.size() && cost == d;
}

std::string revcomp(const std::string &s) {
    std::string r(s.rbegin(), s.rend());
    for (char &c : r) c = c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'N';
    return r;
}

constexpr uint32_t POISON = 0xDEADBEEFu;
uint64_t checked = 0, changed = 0, grew = 0, shrank = 0, merges = 0;

// the header's procedure over `runs`, with S on strand `reverse` at base `s_at` of its stream and T at `t_at` of its own
std::vector<uint32_t> by_header(const std::string &S, const std::string &T, const std::vector<uint32_t> &runs, int64_t d, bool reverse, size_t s_at,
                                size_t t_at, totals *tot) {
    const std::string junk_s(s_at, 'G'), junk_t(t_at, 'C');
    const PackedStream ps(junk_s + (reverse ? revcomp(S) : S), 0, 1), pt(junk_t + T, 0, 1);
    const dcn_wf_side side_s = {ps.p(), ps.m(), (int64_t)(reverse ? s_at + S.size() : s_at), reverse ? 1u : 0u};
    const dcn_wf_side side_t = {pt.p(), pt.m(), (int64_t)t_at, 0u};
    std::vector<uint32_t> words((size_t)dcn_aln_ops_bound((uint64_t)d), POISON); // exactly the bound
    dcn_la_row row = dcn_la_begin(words.data(), (uint32_t)words.size(), side_s, side_t);
    for (uint32_t run : runs) dcn_la_feed<dcn_la_serial>(row, run);
    const uint32_t n = dcn_la_end<dcn_la_serial>(row);
    if (!row.ok) {
        std::fprintf(stderr, "the row's words did not hold the stacks\n");
        std::exit(1);
    }
    tot->shifted = row.shifted, tot->passed = row.passed, tot->merged = row.merged;
    if (n == 0) return runs; // the row stays
    return std::vector<uint32_t>(words.begin(), words.begin() + n);
}

std::string text(const std::vector<uint32_t> &runs) {
    std::string s;
    for (uint32_t run : runs) s += std::to_string(run >> 4) + "-ID----=X"[run & 15u];
    return s;
}

// -> the left-aligned runs as text
std::string check_cols(const std::string &S, const std::string &T, const std::vector<uint32_t> &cols, int64_t d, bool from_a3) {
    const std::vector<uint32_t> runs = runs_of(cols);
    totals want_tot;
    const std::vector<uint32_t> want_cols = brute(S, T, cols, &want_tot);
    const std::vector<uint32_t> want = runs_of(want_cols);
    bool ok = valid(S, T, cols, d) && valid(S, T, want_cols, d) && want.size() <= (size_t)dcn_aln_ops_bound((uint64_t)d);
    // N5: the same multiset of ops; N4: no gap became first; N6: a second application changes nothing
    std::vector<uint32_t> a = cols, b = want_cols;
    std::sort(a.begin(), a.end()), std::sort(b.begin(), b.end());
    ok = ok && a == b && (cols.empty() || is_gap(want_cols[0]) == is_gap(cols[0]));
    totals again_tot;
    ok = ok && brute(S, T, want_cols, &again_tot) == want_cols && again_tot == totals();
    if (from_a3)
        for (size_t c = 1; ok && c < want_cols.size(); ++c) ok = !(is_gap(want_cols[c]) && is_gap(want_cols[c - 1]) && want_cols[c] != want_cols[c - 1]);
    for (int variant = 0; ok && variant < 4; ++variant) {
        const bool reverse = variant & 1;
        const size_t s_at = variant < 2 ? 0 : 1 + (checked * 7 + (size_t)variant) % 37, t_at = variant < 2 ? 0 : 1 + (checked * 5 + (size_t)variant) % 41;
        totals got_tot, twice_tot;
        const std::vector<uint32_t> got = by_header(S, T, runs, d, reverse, s_at, t_at, &got_tot);
        ok = got == want && got_tot == want_tot;
        ok = ok && by_header(S, T, got, d, reverse, s_at, t_at, &twice_tot) == got && twice_tot == totals();
        if (!ok) std::fprintf(stderr, "variant %d: got %s (%llu %llu %llu)\n", variant, text(got).c_str(), (unsigned long long)got_tot.shifted,
                              (unsigned long long)got_tot.passed, (unsigned long long)got_tot.merged);
    }
    if (!ok) {
        std::fprintf(stderr, "S=%s\nT=%s\nd=%lld runs %s want %s (%llu %llu %llu)\n", S.c_str(), T.c_str(), (long long)d, text(runs).c_str(),
                     text(want).c_str(), (unsigned long long)want_tot.shifted, (unsigned long long)want_tot.passed, (unsigned long long)want_tot.merged);
        std::exit(1);
    }
    ++checked;
    changed += want != runs;
    grew += want.size() > runs.size();
    shrank += want.size() < runs.size();
    merges += want_tot.merged;
    return text(want);
}

std::string check(const std::string &S, const std::string &T) {
    int64_t d = 0;
    const std::vector<uint32_t> cols = table_walk(S, T, &d);
    return check_cols(S, T, cols, d, true);
}

// runs written out, which need not be A3's: `cigar` as text
std::string check_runs(const std::string &S, const std::string &T, const std::string &cigar) {
    std::vector<uint32_t> runs;
    uint32_t len = 0;
    for (char c : cigar) {
        if (c >= '0' && c <= '9') len = len * 10 + (uint32_t)(c - '0');
        else runs.push_back((len << 4) | (c == 'I' ? DCN_ALN_I : c == 'D' ? DCN_ALN_D : c == '=' ? DCN_ALN_EQ : DCN_ALN_X)), len = 0;
    }
    const std::vector<uint32_t> cols = cols_of(runs);
    int64_t d = 0;
    for (uint32_t op : cols) d += op != DCN_ALN_EQ;
    return check_cols(S, T, cols, d, false);
}

void expect(const std::string &got, const char *want, const char *what) {
    if (got != want) {
        std::fprintf(stderr, "%s: %s, expected %s\n", what, got.c_str(), want);
        std::exit(1);
    }
}

std::string random_seq(std::mt19937_64 &rng, size_t len, const char *alphabet, size_t letters) {
    std::string s(len, 'A');
    for (char &c : s) c = alphabet[rng() % letters];
    return s;
}

// up to `edits` planted edits
std::string planted(std::mt19937_64 &rng, std::string s, unsigned edits, const char *alphabet, size_t letters) {
    for (unsigned e = 0; e < edits && !s.empty(); ++e) {
        const size_t at = (size_t)(rng() % s.size());
        const unsigned kind = (unsigned)(rng() % 3), len = 1 + (unsigned)(rng() % 3);
        if (kind == 0) s[at] = alphabet[rng() % letters];
        else if (kind == 1) s.erase(at, len);
        else s.insert(at, random_seq(rng, len, alphabet, letters));
    }
    return s;
}

} // namespace

int main() {
    std::mt19937_64 rng(2201);
    const struct { const char *letters; size_t n; } alphabets[] = {{"A", 1}, {"AC", 2}, {"ACGT", 4}, {"ACN", 3}};
    for (int round = 0; round < 6000; ++round) {
        const auto &a = alphabets[round % 4];
        const std::string T = random_seq(rng, 1 + (size_t)(rng() % 40), a.letters, a.n);
        check(planted(rng, T, (unsigned)(rng() % 4), a.letters, a.n), T);
        if (round % 20 == 0) check(random_seq(rng, (size_t)(rng() % 12), a.letters, a.n), T); // unrelated: gaps next to X columns
    }
    check("", ""), check("", "ACG"), check("ACG", ""), check("ACGT", "ACGT");
    // long rows over two letters: many gaps, many runs
    for (int round = 0; round < 60; ++round) {
        const std::string T = random_seq(rng, 300 + (size_t)(rng() % 200), "AC", 2);
        check(planted(rng, T, 40 + (unsigned)(rng() % 60), "AC", 2), T);
    }
    // homopolymers: a gap of one base that takes 1, 15, 16, 17, ... steps (the 16-base groups of the backward comparison), a
    // deletion and an insertion, and gaps of 1 - 65 bases cut out of one
    for (size_t steps : {1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129}) {
        const std::string head = "GTC", tail = "GTTCAG", hp(steps + 1, 'A');
        const std::string want_d = "3=1D" + std::to_string(steps + tail.size()) + "=", want_i = "3=1I" + std::to_string(steps + 1 + tail.size()) + "=";
        expect(check(head + hp.substr(1) + tail, head + hp + tail), want_d.c_str(), "a deletion in a homopolymer");
        expect(check(head + hp + "A" + tail, head + hp + tail), want_i.c_str(), "an insertion in a homopolymer");
    }
    for (size_t len = 1; len <= 65; ++len) {
        const std::string hp(len + 20, 'A');
        const std::string want = "2=" + std::to_string(len) + "D24=";
        expect(check("CG" + hp.substr(len) + "CGTA", "CG" + hp + "CGTA"), want.c_str(), "a long gap in a homopolymer");
    }
    // tandem repeats
    expect(check("GG" "ACACAC" "TT", "GG" "ACACACAC" "TT"), "2=2D8=", "a unit of a period-2 repeat");
    expect(check("GG" "ACACACAC" "TT", "GG" "ACACAC" "TT"), "2=2I8=", "... inserted");
    expect(check("GG" "ACTACTACT" "GA", "GG" "ACTACTACTACT" "GA"), "2=3D11=", "a unit of a period-3 repeat");
    expect(check("GG" "ACTACTACTACT" "GA", "GG" "ACTACTACT" "GA"), "2=3I11=", "... inserted");
    // stops: a base that differs, an invalid base, the row's first column, a gap that is first
    expect(check("TCAAAG", "TCAAAAG"), "2=1D4=", "a base that differs");
    expect(check("TCANAAG", "TCANAAAG"), "3=1X1D3=", "an invalid base of the record");
    expect(check_runs("CANAAAG", "CACAAG", "2=1X2=1I1="), "2=1X1I3=", "an invalid base of the read");
    expect(check("AAAC", "AAAAC"), "1=1D3=", "the row's first column: the gap is the second run");
    expect(check("AAAAC", "AAAC"), "1=1I3=", "... an insertion");
    expect(check_runs("AAC", "AAAC", "1D3="), "1D3=", "a gap that is first stays first");
    // passing runs
    expect(check_runs("GTCAAAG", "GTAAAAAG", "2=1X3=1D1="), "2=1D1X4=", "past '=' columns and an X column: the X keeps its op");
    expect(check_runs("GCATAAG", "GCAAAAAG", "3=1X2=1D1="), "2=1D1=1X3=", "as many runs: the last passed run merges with the run behind");
    expect(check_runs("GCATAAG", "GCAAAAAC", "3=1X2=1D1X"), "2=1D1=1X2=1X", "one run more");
    expect(check_runs("GCAAATTG", "GCAAAAATG", "5=1D1X2="), "2=1D3=1X2=", "a gap that stops within the run in front");
    expect(check_runs("GAATAAG", "GAAAAG", "3=1I3="), "3=1I3=", "an insertion that cannot move");
    expect(check_runs("CGAGAAAT", "CGTGAAT", "2=1X3=1I1="), "2=1X1=1I3=", "an insertion stops where the read's bases differ");
    expect(check_runs("CAAAAT", "CGAAT", "1=1X2=1I1="), "1=1I1X3=", "an insertion passes an X column whose read base equals the last inserted");
    // merging gaps
    expect(check_runs("GCAAAT", "GCAAAAAT", "2=1D2=1D2="), "2=2D4=", "two deletions become one and go on");
    expect(check_runs("GCAAAAAT", "GCAAAT", "2=1I2=1I2="), "2=2I4=", "two insertions become one");
    expect(check_runs("AAAT", "AAAAAT", "1D2=1D2="), "2D4=", "a gap merges into a leading gap");
    expect(check_runs("GCCCT", "GACCT", "1=1D2=1I1="), "1=1D1I3=", "a gap directly behind a gap of the other kind stops");
    if (changed < 2000 || grew < 100 || shrank < 100 || merges < 100) {
        std::fprintf(stderr, "too few rows that change: %llu changed, %llu grew, %llu shrank, %llu merges\n", (unsigned long long)changed,
                     (unsigned long long)grew, (unsigned long long)shrank, (unsigned long long)merges);
        return 1;
    }
    std::printf("left align ok: %llu rows, %llu changed, %llu grew, %llu shrank, %llu merges\n", (unsigned long long)checked,
                (unsigned long long)changed, (unsigned long long)grew, (unsigned long long)shrank, (unsigned long long)merges);
    return 0;
}

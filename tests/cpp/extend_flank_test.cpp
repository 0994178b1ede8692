// The flank routine of the extend kernel (csrc/dcn_extend.h: dcn_ext_flank over dcn_wavefront.h's dcn_wf_diagonal with the
// guarded load, the fetch that never reads in front of a stream) compiled for the host, against rules X3-X5 of THE DEFINITION OF AN EXTENDED
// PLACEMENT from a full table.  The streams are heap arrays of exactly the words the real ones have: the batch stream with
// its pad in front and behind, the store with no word in front of base 0 and its pad words behind -- under the address
// sanitizer a read of word -1 of the store, or past either pad, ends the program.  All four combinations of strand and
// side; left flanks that start at store bases 0 .. 33; right flanks that end at the last base of the last record; reads
// and records that lie side by side and continue each other's bases.  Packing is dcn_pack.h's, as on the device.
#include "dcn_extend.h"
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
static std::string reversed(const std::string &s) { return std::string(s.rbegin(), s.rend()); }

static std::string random_text(size_t n, int p_invalid) {
    std::string s(n, 'A');
    for (auto &c : s) {
        c = "ACGT"[rnd() & 3];
        if (rnd() % 100 < 10) c |= 0x20;
        if ((int)(rnd() % 100) < p_invalid) c = 'N';
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

// rules X3-X5 from the full table
static void by_table(const std::string &U, const std::string &V, int64_t penalty, int64_t end_bonus, int64_t max_edits, int64_t *bi, int64_t *bj,
                     int64_t *bd) {
    const int64_t f = (int64_t)U.size(), g = (int64_t)V.size();
    std::vector<int64_t> prev(g + 1), cur(g + 1);
    int64_t best = INT64_MIN;
    *bi = *bj = *bd = 0;
    for (int64_t i = 0; i <= f; ++i) {
        for (int64_t j = 0; j <= g; ++j) {
            int64_t d;
            if (i == 0) d = j;
            else if (j == 0) d = i;
            else d = std::min(prev[j - 1] + (equal(U[i - 1], V[j - 1]) ? 0 : 1), std::min(prev[j], cur[j - 1]) + 1);
            cur[j] = d;
            if (d > max_edits) continue;
            const int64_t v = i + j - penalty * d + (i == f ? end_bonus : 0);
            if (v > best || (v == best && (d < *bd || (d == *bd && i > *bi)))) best = v, *bi = i, *bj = j, *bd = d;
        }
        std::swap(prev, cur);
    }
}

int main() {
    const size_t FRONT_PAD = 64, TAIL_PAD = 8, STORE_PAD = 8; // DCN_FRONT_PAD, and no fewer words behind than the real streams
    int n_flanks = 0, n_extended = 0, n_edits = 0, n_at_base0 = 0, n_at_end = 0;
    for (int trial = 0; trial < 1500; ++trial) {
        // two records side by side in the store, the second anywhere within a word; three reads side by side in the batch
        const std::string rec0 = random_text(40 + rnd() % 120, trial % 7 == 0 ? 3 : 0);
        std::string rec1 = random_text(30 + rnd() % 90, 0);
        const uint32_t R = rnd() & 1u;
        const std::string &rec = R ? rec1 : rec0;
        const uint64_t rec_start = R ? rec0.size() : 0, Lr = rec.size();
        // the record interval: left flanks at store bases 0 .. 33 of record 0, right flanks up to the last base of record 1
        uint64_t fs = trial % 3 == 0 ? (uint64_t)(trial / 3 % 34) : rnd() % (Lr / 2);
        if (fs > Lr) fs = Lr;
        uint64_t fe = fs + rnd() % (Lr - fs + 1);
        if (trial % 5 == 0) fe = Lr - rnd() % 3;
        if (fe < fs) fe = fs;
        // R': a copy of the record around the interval with edits, clipped junk at either end now and then
        const int percent = (int)(rnd() % 4) * 6;
        uint64_t lo = fs - std::min<uint64_t>(fs, rnd() % 50), hi = fe + std::min<uint64_t>(Lr - fe, rnd() % 50);
        std::string left = mutated(rec.substr(lo, fs - lo), percent), right = mutated(rec.substr(fe, hi - fe), percent);
        if (rnd() % 3 == 0) left = random_text(rnd() % 12, 0) + left;
        if (rnd() % 3 == 0) right += random_text(rnd() % 12, 0);
        // (what lies beyond the record continues R' now and then: a run that left the flank would go on matching)
        const std::string mid = random_text(rnd() % 20, 0);
        const std::string oriented = left + mid + right;
        const uint64_t L = oriented.size(), a = left.size(), b = a + mid.size();
        const uint32_t reverse = rnd() & 1u;
        const std::string read = reverse ? revcomp(oriented) : oriented;
        const uint64_t rs = reverse ? L - b : a, re = reverse ? L - a : b;
        // the neighbours in the batch continue the record's bases, so a run that left the read would go on
        const std::string before = reverse ? revcomp(rec.substr(std::min(Lr, hi), std::min<uint64_t>(Lr - std::min(Lr, hi), 20))) : rec.substr(lo - std::min<uint64_t>(lo, 20), std::min<uint64_t>(lo, 20));
        const std::string after = reverse ? revcomp(rec.substr(lo - std::min<uint64_t>(lo, 20), std::min<uint64_t>(lo, 20))) : rec.substr(std::min(Lr, hi), std::min<uint64_t>(Lr - std::min(Lr, hi), 20));
        const bool first = trial % 4 == 0, last = trial % 4 == 1;
        const std::string batch_text = (first ? std::string() : before) + read + (last ? std::string() : after);
        const uint64_t read_off = first ? 0 : before.size();
        const PackedStream batch(batch_text, FRONT_PAD, TAIL_PAD), store(rec0 + rec1, 0, STORE_PAD);

        const uint32_t penalty = 2 + rnd() % 8, end_bonus = rnd() % 12, max_edits = rnd() % 4 == 0 ? rnd() % 4 : 1023;
        for (int side = 0; side < 2; ++side) {
            const bool is_left = side == 0;
            const std::string U = is_left ? reversed(oriented.substr(0, a)) : oriented.substr(b);
            const std::string V = is_left ? reversed(rec.substr(0, fs)) : rec.substr(fe);
            int64_t wi, wj, wd;
            by_table(U, V, penalty, end_bonus, max_edits, &wi, &wj, &wd);
            // the item, as extend_api.hip resolves it
            const bool u_back = is_left != (reverse != 0);
            const uint32_t f = (uint32_t)(u_back ? rs : L - re), g = (uint32_t)(is_left ? fs : Lr - fe);
            CHECK(f == U.size() && g == V.size(), "trial %d side %d: f %u g %u", trial, side, f, g);
            const dcn_wf_side Us = {batch.p(), batch.m(), (int64_t)(read_off + (u_back ? rs : re)), u_back ? 1u : 0u};
            const dcn_wf_side Vs = {store.p(), store.m(), (int64_t)(rec_start + (is_left ? fs : fe)), is_left ? 1u : 0u};
            const uint32_t cap = dcn_ext_cap(f, g, penalty, end_bonus, max_edits);
            std::vector<uint32_t> wave(2 * (2 * (size_t)cap + 1)); // exactly the two arrays
            uint32_t gi = 0, gj = 0, gd = 0;
            dcn_ext_flank(Us, Vs, f, g, cap, penalty, end_bonus, wave.data(), &gi, &gj, &gd);
            CHECK(gi == wi && gj == wj && gd == wd, "trial %d side %d rev %u f %u g %u p %u b %u e %u: got (%u, %u, %u), the table (%lld, %lld, %lld)",
                  trial, side, reverse, f, g, penalty, end_bonus, max_edits, gi, gj, gd, (long long)wi, (long long)wj, (long long)wd);
            ++n_flanks;
            n_extended += gi > 0;
            n_edits += gd > 0;
            n_at_base0 += is_left && R == 0 && fs < 34 && gj == fs && fs > 0;
            n_at_end += !is_left && R == 1 && gj == Lr - fe && fe < Lr;
        }
    }
    std::printf("%d flanks, %d extended, %d with edits, %d reached base 0 of the store, %d reached its last base\n", n_flanks, n_extended,
                n_edits, n_at_base0, n_at_end);
    CHECK(n_extended > 500 && n_edits > 100 && n_at_base0 > 20 && n_at_end > 20, "the cases do not cover what they are meant to");
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("extend flank ok\n");
    return 0;
}

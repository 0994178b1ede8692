// The word helpers of the verify kernel (csrc/dcn_wavefront.h) compiled for the host, against naive loops over ASCII:
// fetches at every bit offset, the reverse complement of a word, and the run of EQUAL bases from every offset 0..31 of both
// streams, forward and reverse, with and without invalid bases.  Packing is dcn_pack.h's, as on the device.
#include "dcn_pack.h"
#include "dcn_wavefront.h"

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

// a stream as the pack kernel leaves it, with `pad` words in front of and behind it (views point behind the front pad)
struct Stream {
    std::vector<uint32_t> packed, mask;
    int pad;
    Stream(const std::string &s, int pad_words) : pad(pad_words) {
        const size_t groups = (s.size() + 31) / 32;
        packed.assign(2 * groups + 2 * pad, 0);
        mask.assign(groups + 2 * pad, 0);
        for (size_t g = 0; g < groups; ++g) {
            for (int q = 0; q < 8; ++q) {
                uint32_t w = 0;
                for (int j = 0; j < 4; ++j) {
                    const size_t i = g * 32 + 4 * q + j;
                    w |= (uint32_t)(uint8_t)(i < s.size() ? s[i] : 'A') << (8 * j);
                }
                packed[pad + 2 * g + q / 4] |= dcn_pack4(w) << (8 * (q % 4));
                mask[pad + g] |= dcn_invalid4(w) << (4 * q);
            }
        }
    }
    const uint32_t *p() const { return packed.data() + pad; }
    const uint32_t *m() const { return mask.data() + pad; }
};

static std::string random_text(size_t n, int p_invalid, int p_lower) {
    std::string s(n, 'A');
    for (auto &c : s) {
        c = "ACGT"[rnd() & 3];
        if ((int)(rnd() % 100) < p_lower) c |= 0x20;
        if ((int)(rnd() % 100) < p_invalid) c = "NnRY-"[rnd() % 5];
    }
    return s;
}

int main() {
    // bit reverse and the reverse complement of a word against loops over its groups
    for (int t = 0; t < 2000; ++t) {
        const uint32_t x = rnd() ^ (rnd() << 16);
        uint32_t br = 0, rc = 0;
        for (int b = 0; b < 32; ++b) br |= ((x >> b) & 1u) << (31 - b);
        for (int u = 0; u < 16; ++u) rc |= ((((x >> (2 * (15 - u))) & 3u) ^ 2u)) << (2 * u);
        CHECK(dcn_wf_brev32(x) == br, "%08x", x);
        CHECK(dcn_wf_revcomp16(x) == rc, "%08x", x);
        CHECK(dcn_wf_rev16(x & 0xFFFFu) == (br >> 16), "%08x", x);
    }
    // run16: first difference or invalid bit, whichever comes first
    for (int u = 0; u <= 16; ++u)
        for (int v = 0; v <= 16; ++v) {
            const uint32_t xs = rnd() ^ (rnd() << 16);
            uint32_t xt = xs;
            if (u < 16) xt ^= 1u << (2 * u + (rnd() & 1)); // group u differs
            if (u < 15 && (rnd() & 1)) xt ^= rnd() << (2 * u + 2); // ... and anything behind it may
            const uint32_t inv = v < 16 ? (1u << v) | ((rnd() & 0xFFFFu) << v) : 0u;
            CHECK(dcn_wf_run16(xs, xt, inv & 0xFFFFu) == (uint32_t)(u < v ? u : v), "u=%d v=%d", u, v);
        }
    // fetches and runs over text, at every offset 0..31 of both streams
    const int PAD = 2;
    for (int variant = 0; variant < 3; ++variant) {
        const int p_invalid = variant == 1 ? 3 : 0, p_lower = variant == 2 ? 30 : 0;
        const std::string a = random_text(700, p_invalid, p_lower);
        // b: a with a change every ~40 bases, so runs end by a difference, by an invalid base and by the limit
        std::string b = a;
        for (size_t i = 20; i < b.size(); i += 25 + rnd() % 40) b[i] = b[i] == 'A' ? 'C' : 'A';
        if (variant == 2)
            for (auto &c : b) c ^= (rnd() & 1) ? 0x20 : 0; // case differs at random: equal all the same
        const Stream A(a, PAD), B(b, PAD);
        for (size_t i = 0; i + 16 <= a.size(); i += 7) {
            const uint32_t x = dcn_wf_fetch16<dcn_wf_plain>(A.p(), (int64_t)i), m = dcn_wf_mask16<dcn_wf_plain>(A.m(), (int64_t)i);
            for (int u = 0; u < 16; ++u) {
                CHECK(((x >> (2 * u)) & 3u) == (((uint32_t)a[i + u] >> 1) & 3u), "fetch16 at %zu + %d", i, u);
                CHECK(((m >> u) & 1u) == (valid(a[i + u]) ? 0u : 1u), "mask16 at %zu + %d", i, u);
            }
        }
        // forward against forward
        for (int so = 0; so < 32; ++so)
            for (int to = 0; to < 32; ++to)
                for (int rep = 0; rep < 6; ++rep) {
                    const int64_t base = 32 * (rnd() % 12);
                    const int64_t i = base + so, j = base + to + (rep & 1 ? 0 : so - to); // same text position half the time
                    if (j < 0) continue;
                    const uint64_t limit = rep == 5 ? rnd() % 40 : std::min(a.size() - i, b.size() - j);
                    uint64_t want = 0;
                    while (want < limit && equal(a[i + want], b[j + want])) ++want;
                    const dcn_wf_side S = {A.p(), A.m(), 0, 0u}, T = {B.p(), B.m(), 0, 0u};
                    const uint64_t got = dcn_wf_match_run<dcn_wf_plain>(S, i, T, j, limit);
                    CHECK(got == want, "forward variant %d i=%lld j=%lld limit=%llu: %llu, want %llu", variant, (long long)i,
                          (long long)j, (unsigned long long)limit, (unsigned long long)got, (unsigned long long)want);
                }
        // the reverse complement of an interval of a against b: plant revcomp(a[lo, hi)) in a third text
        for (int so = 0; so < 32; ++so)
            for (int to = 0; to < 32; ++to) {
                const size_t lo = so, hi = 300 + 32 + (rnd() % 32); // the interval [lo, hi) of a, read backwards
                std::string rc;
                for (size_t q = hi; q-- > lo;) rc.push_back(comp(a[q]));
                std::string c = std::string(to, 'G') + rc; // T: the same sequence at offset `to`, with changes
                for (size_t q = to + 10 + rnd() % 30; q < c.size(); q += 30 + rnd() % 50) c[q] = c[q] == 'A' ? 'C' : 'A';
                // ... and forward: a from base so on, against the same text at offset `to` with changes
                std::string f = std::string(to, 'G') + a.substr(so, 400);
                for (size_t q = to + rnd() % 40; q < f.size(); q += 30 + rnd() % 50) f[q] = f[q] == 'A' ? 'C' : 'A';
                const Stream Fs(f, PAD);
                const dcn_wf_side SF = {A.p(), A.m(), (int64_t)so, 0u}, TF = {Fs.p(), Fs.m(), (int64_t)to, 0u};
                for (int rep = 0; rep < 4; ++rep) {
                    const int64_t i = rep == 0 ? 0 : (int64_t)(rnd() % 400);
                    const uint64_t limit = 400 - i;
                    uint64_t want = 0;
                    while (want < limit && equal(a[so + i + want], f[to + i + want])) ++want;
                    const uint64_t got = dcn_wf_match_run<dcn_wf_plain>(SF, i, TF, i, limit);
                    CHECK(got == want, "shifted variant %d so=%d to=%d i=%lld: %llu, want %llu", variant, so, to, (long long)i,
                          (unsigned long long)got, (unsigned long long)want);
                }
                const Stream Cs(c, PAD);
                const dcn_wf_side S = {A.p(), A.m(), (int64_t)hi, 1u}, T = {Cs.p(), Cs.m(), (int64_t)to, 0u};
                for (int rep = 0; rep < 4; ++rep) {
                    const int64_t i = rep == 0 ? 0 : (int64_t)(rnd() % (hi - lo));
                    const uint64_t limit = (hi - lo) - i;
                    uint64_t want = 0;
                    while (want < limit && equal(comp(a[hi - 1 - (i + want)]), c[to + i + want])) ++want;
                    const uint64_t got = dcn_wf_match_run<dcn_wf_plain>(S, i, T, i, limit);
                    CHECK(got == want, "reverse variant %d lo=%zu to=%d i=%lld: %llu, want %llu", variant, lo, to, (long long)i,
                          (unsigned long long)got, (unsigned long long)want);
                }
            }
    }
    // a run of exactly the limit, limits 0..40, and N against N
    {
        const std::string a = random_text(200, 0, 0);
        const Stream A(a, PAD);
        const dcn_wf_side S = {A.p(), A.m(), 0, 0u};
        for (uint64_t limit = 0; limit <= 40; ++limit)
            for (int64_t i = 0; i < 33; ++i) CHECK(dcn_wf_match_run<dcn_wf_plain>(S, i, S, i, limit) == limit, "limit %llu", (unsigned long long)limit);
        std::string n = a;
        n[37] = 'N';
        const Stream Ns(n, PAD);
        const dcn_wf_side SN = {Ns.p(), Ns.m(), 0, 0u};
        CHECK(dcn_wf_match_run<dcn_wf_plain>(SN, 0, SN, 0, 200) == 37, "N against N");
        CHECK(dcn_wf_match_run<dcn_wf_plain>(SN, 37, SN, 37, 5) == 0, "N against N at the start");
        CHECK(dcn_wf_match_run<dcn_wf_plain>(SN, 38, SN, 38, 100) == 100, "behind the N");
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("verify helpers ok\n");
    return 0;
}

// phase_rule_test.cpp -- csrc/dcn_phase.h on the host: rule H2's observation over every column and every pair of alleles, rule
// H5's decision at every boundary, the scan operator's associativity by brute force over all short sequences, and a blocked
// scan (per block, over the blocks' aggregates, apply: the shape of the three kernels) with block sizes 1 .. 9 against the
// sequential rule H6.  Built by tests/test_phase_abi.py with -fsanitize=address,undefined and run as a program of its own.
#include "dcn_phase.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                             \
        }                                                                             \
    } while (0)

static bool same(const dcn_phase_elem &a, const dcn_phase_elem &b) { return a.heads == b.heads && a.x == b.x && a.last == b.last; }

static uint32_t decide(uint32_t n00, uint32_t n01, uint32_t n10, uint32_t n11, uint32_t min_reads, uint32_t permille) {
    const uint32_t n[4] = {n00, n01, n10, n11};
    return dcn_phase_decide(n, min_reads, permille);
}

// rule H5 as the header states it, in the widest integers there are
static uint32_t decide_slow(const uint32_t *n, uint32_t min_reads, uint32_t permille) {
    const unsigned __int128 c = (unsigned __int128)n[0] + n[3], t = (unsigned __int128)n[1] + n[2], total = c + t, minor = c < t ? c : t;
    const bool joined = total >= (min_reads > 1 ? min_reads : 1) && c != t && minor * 1000 <= total * permille;
    return joined ? (DCN_PHASE_DEC_JOINED | (t > c ? DCN_PHASE_DEC_TRANS : 0u)) : 0u;
}

static uint64_t observations() {
    uint64_t n = 0;
    for (uint32_t a0 = 0; a0 < 4; ++a0)
        for (uint32_t a1 = 0; a1 < 4; ++a1) {
            if (a0 == a1) continue;
            const uint32_t al = dcn_phase_pack_alleles(a0, a1);
            for (uint32_t col = 0; col < 8; ++col, ++n) {
                const uint32_t want = col == a0 ? 0u : col == a1 ? 1u : DCN_PHASE_NONE;
                CHECK(dcn_phase_observation(col, al) == want);
                CHECK(dcn_phase_observation(col, al | 16u) == want); // (the bit beside the alleles is not looked at)
            }
        }
    CHECK(dcn_phase_counter(0, 0) == 0 && dcn_phase_counter(0, 1) == 1 && dcn_phase_counter(1, 0) == 2 && dcn_phase_counter(1, 1) == 3);
    return n;
}

static uint64_t decisions() {
    const uint32_t J = DCN_PHASE_DEC_JOINED, R = DCN_PHASE_DEC_TRANS;
    // N = min_reads - 1 and N = min_reads
    CHECK(decide(1, 0, 0, 0, 2, 200) == 0 && decide(1, 0, 0, 1, 2, 200) == J && decide(0, 1, 1, 0, 2, 200) == (J | R));
    CHECK(decide(4, 0, 0, 0, 5, 1000) == 0 && decide(5, 0, 0, 0, 5, 1000) == J && decide(0, 2, 3, 0, 5, 0) == (J | R));
    // min_reads 0 and 1 both ask for one row; nothing joins on nothing
    CHECK(decide(0, 0, 0, 0, 0, 1000) == 0 && decide(0, 0, 0, 0, 1, 1000) == 0 && decide(1, 0, 0, 0, 0, 0) == J && decide(0, 0, 1, 0, 1, 0) == (J | R));
    // c == t never joins, whatever the permille
    CHECK(decide(1, 1, 0, 0, 1, 1000) == 0 && decide(3, 2, 1, 0, 2, 1000) == 0 && decide(500, 250, 250, 0, 2, 1000) == 0);
    // minor * 1000 == N * permille, and one more on either side
    CHECK(decide(8, 2, 0, 0, 2, 200) == J && decide(8, 1, 1, 0, 2, 200) == J && decide(7, 2, 0, 1, 2, 200) == J);
    CHECK(decide(8, 2, 0, 0, 2, 199) == 0 && decide(7, 3, 0, 0, 2, 200) == 0 && decide(79, 20, 0, 0, 2, 200) == 0 && decide(80, 20, 0, 0, 2, 200) == J);
    CHECK(decide(2, 8, 0, 0, 2, 200) == (J | R) && decide(1, 4, 4, 1, 2, 200) == (J | R) && decide(3, 7, 0, 0, 2, 200) == 0);
    // permille 0: only a clean link; permille 1000: everything but a tie
    CHECK(decide(1000000, 0, 0, 0, 2, 0) == J && decide(1000000, 1, 0, 0, 2, 0) == 0 && decide(0, 7, 9, 0, 2, 0) == (J | R));
    CHECK(decide(5, 4, 0, 0, 2, 1000) == J && decide(4, 5, 0, 0, 2, 1000) == (J | R) && decide(2, 3, 2, 2, 2, 1000) == (J | R));
    // counters at their ends: the sums and products are 64 bits
    CHECK(decide(0xFFFFFFFFu, 0, 0, 0xFFFFFFFFu, 0xFFFFFFFFu, 0) == J && decide(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFEu, 2, 1000) == (J | R));
    CHECK(decide(0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0xFFFFFFFFu, 2, 333) == 0 && decide(0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0xFFFFFFFFu, 2, 334) == J);
    uint64_t n = 0;
    const uint32_t v[] = {0, 1, 2, 3, 4, 5, 8, 9, 10, 0xFFFFFFFFu};
    const uint32_t pm[] = {0, 1, 199, 200, 201, 250, 333, 334, 500, 999, 1000}, mr[] = {0, 1, 2, 3, 10, 20};
    for (uint32_t a : v)
        for (uint32_t b : v)
            for (uint32_t c : v)
                for (uint32_t d : v) {
                    const uint32_t c4[4] = {a, b, c, d};
                    for (uint32_t p : pm)
                        for (uint32_t m : mr) {
                            CHECK(dcn_phase_decide(c4, m, p) == decide_slow(c4, m, p));
                            ++n;
                        }
                }
    return n;
}

// every element a stretch can be, small: with and without heads, both relations, two head indices
static std::vector<dcn_phase_elem> alphabet() {
    std::vector<dcn_phase_elem> e;
    for (uint32_t heads = 0; heads < 3; ++heads)
        for (uint32_t x = 0; x < 2; ++x)
            for (uint64_t last : {(uint64_t)0, (uint64_t)5, (uint64_t)1 << 40}) {
                if (heads == 0 && last != 0) continue; // (no head: last is 0 by the element's definition)
                dcn_phase_elem v;
                v.heads = heads, v.x = x, v.last = last;
                e.push_back(v);
            }
    return e;
}

static uint64_t associativity() {
    const std::vector<dcn_phase_elem> e = alphabet();
    const dcn_phase_elem id = dcn_phase_identity();
    uint64_t n = 0;
    for (const auto &a : e) {
        CHECK(same(dcn_phase_combine(id, a), a) && same(dcn_phase_combine(a, id), a));
        for (const auto &b : e)
            for (const auto &c : e) {
                CHECK(same(dcn_phase_combine(dcn_phase_combine(a, b), c), dcn_phase_combine(a, dcn_phase_combine(b, c))));
                ++n;
            }
    }
    // all sequences of up to 7 sites over the three decisions a link can have: every bracketing point agrees with the fold
    for (uint32_t len = 1; len <= 7; ++len) {
        uint32_t total = 1;
        for (uint32_t i = 0; i + 1 < len; ++i) total *= 3;
        for (uint32_t code = 0; code < total; ++code) {
            std::vector<dcn_phase_elem> s(len);
            uint32_t q = code;
            for (uint32_t i = 0; i < len; ++i) {
                const uint32_t dec = i == 0 ? 0u : (q % 3 == 0 ? 0u : q % 3 == 1 ? DCN_PHASE_DEC_JOINED : (DCN_PHASE_DEC_JOINED | DCN_PHASE_DEC_TRANS));
                if (i) q /= 3;
                s[i] = dcn_phase_site_elem(i, dec);
            }
            dcn_phase_elem fold = id;
            for (const auto &v : s) fold = dcn_phase_combine(fold, v);
            for (uint32_t cut = 0; cut <= len; ++cut, ++n) {
                dcn_phase_elem l = id, r = id;
                for (uint32_t i = 0; i < cut; ++i) l = dcn_phase_combine(l, s[i]);
                for (uint32_t i = len; i-- > cut;) r = dcn_phase_combine(s[i], r); // (folded from the right)
                CHECK(same(dcn_phase_combine(l, r), fold));
            }
        }
    }
    return n;
}

struct site_result {
    uint64_t head;
    uint32_t set_index, hap;
};

// rule H6, site after site
static std::vector<site_result> sequential(const std::vector<uint32_t> &dec) {
    std::vector<site_result> out(dec.size());
    uint32_t heads = 0;
    for (size_t s = 0; s < dec.size(); ++s) {
        const uint32_t before = s ? dec[s - 1] : 0u;
        if (!(before & DCN_PHASE_DEC_JOINED)) out[s] = {s, heads++, 0u};
        else out[s] = {out[s - 1].head, out[s - 1].set_index, out[s - 1].hap ^ ((before & DCN_PHASE_DEC_TRANS) ? 1u : 0u)};
    }
    return out;
}

// the three passes of phase.hip with `block` sites per block
static std::vector<site_result> blocked(const std::vector<uint32_t> &dec, size_t block) {
    const size_t n = dec.size(), blocks = (n + block - 1) / block;
    std::vector<dcn_phase_elem> agg(blocks);
    for (size_t b = 0; b < blocks; ++b) {
        dcn_phase_elem v = dcn_phase_identity();
        for (size_t s = b * block; s < n && s < (b + 1) * block; ++s) v = dcn_phase_combine(v, dcn_phase_site_elem(s, s ? dec[s - 1] : 0u));
        agg[b] = v;
    }
    dcn_phase_elem before = dcn_phase_identity();
    for (size_t b = 0; b < blocks; ++b) {
        const dcn_phase_elem v = agg[b];
        agg[b] = before;
        before = dcn_phase_combine(before, v);
    }
    std::vector<site_result> out(n);
    for (size_t b = 0; b < blocks; ++b) {
        dcn_phase_elem v = agg[b];
        for (size_t s = b * block; s < n && s < (b + 1) * block; ++s) {
            v = dcn_phase_combine(v, dcn_phase_site_elem(s, s ? dec[s - 1] : 0u));
            CHECK(v.heads >= 1 && v.last <= s);
            out[s] = {v.last, v.heads - 1, v.x};
        }
    }
    return out;
}

static uint64_t blocked_scans() {
    uint64_t n = 0, state = 88172645463325252ull;
    const auto rnd = [&state]() {
        state ^= state << 13, state ^= state >> 7, state ^= state << 17;
        return state;
    };
    const uint32_t kinds[3] = {0u, DCN_PHASE_DEC_JOINED, DCN_PHASE_DEC_JOINED | DCN_PHASE_DEC_TRANS};
    for (uint32_t round = 0; round < 400; ++round) {
        const size_t len = round < 40 ? round : 1 + rnd() % 60;
        std::vector<uint32_t> dec(len);
        const uint32_t bias = round % 4; // all kinds; mostly joined; all unjoined; all joined with alternating relation
        for (size_t s = 0; s < len; ++s)
            dec[s] = bias == 2 ? 0u : bias == 3 ? kinds[1 + s % 2] : kinds[bias == 1 && rnd() % 8 ? 1 + rnd() % 2 : rnd() % 3];
        const std::vector<site_result> want = sequential(dec);
        for (size_t block = 1; block <= 9; ++block, ++n) {
            const std::vector<site_result> got = blocked(dec, block);
            for (size_t s = 0; s < len; ++s)
                CHECK(got[s].head == want[s].head && got[s].set_index == want[s].set_index && got[s].hap == want[s].hap);
        }
    }
    return n;
}

int main() {
    const uint64_t o = observations(), d = decisions(), a = associativity(), b = blocked_scans();
    std::printf("phase rule ok: %llu observations, %llu decisions, %llu bracketings, %llu blocked scans\n", (unsigned long long)o,
                (unsigned long long)d, (unsigned long long)a, (unsigned long long)b);
    return 0;
}

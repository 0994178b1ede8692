// duplicate_key_test.cpp -- the end and key rules of csrc/dcn_duplicates.h (rules D3 and D4 of include/deacon_hip.h) on the
// host alone, against cases whose answers are written out: clip equivalence on both strands, a negative pos5, a pos5 past
// the record's end beside a neighbouring record's coordinate, the mate swap, and every component of a key differing
// alone.  Built with -fsanitize=address,undefined by tests/test_duplicates_abi.py and run as a child process.
#include "dcn_duplicates.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

static int failures = 0;
static int checks = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        ++checks;                                                    \
        if (!(cond)) {                                               \
            ++failures;                                              \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);    \
        }                                                            \
    } while (0)

static dcn_dup_item item(uint32_t record, uint32_t reverse, uint32_t read_start, uint32_t read_end, uint64_t ref_start, uint64_t ref_end,
                         uint32_t read_len) {
    dcn_dup_item it;
    it.ref_start = ref_start, it.ref_end = ref_end, it.record = record, it.reverse = reverse;
    it.read_start = read_start, it.read_end = read_end, it.read_len = read_len, it.reserved = 0;
    return it;
}
static dcn_dup_item none() { return item(DCN_DUP_NO_RECORD, 0, 0, 0, 0, 0, 100); }

static dcn_dup_key single(const dcn_dup_item &a, uint32_t both_ends) { return dcn_dup_unit_key(&a, 0, 0, both_ends); }
static dcn_dup_key pair(const dcn_dup_item &a, const dcn_dup_item &b, uint32_t both_ends) {
    const dcn_dup_item two[2] = {a, b};
    return dcn_dup_unit_key(two, 0, 1, both_ends);
}
static bool same(const dcn_dup_key &a, const dcn_dup_key &b) {
    const bool eq = dcn_dup_key_equal(a, b);
    if (eq) CHECK(dcn_dup_key_hash(a) == dcn_dup_key_hash(b)); // equal keys begin their probes in one place
    CHECK(dcn_dup_key_equal(b, a) == eq);
    return eq;
}

int main() {
    // ---- D3: ends ----
    {
        const dcn_dup_end f = dcn_dup_end_of(item(3, 0, 5, 90, 105, 191, 100), 1);
        CHECK(f.record == 3 && f.reverse == 0 && f.pos5 == 100 && f.pos3 == 201);
        const dcn_dup_end r = dcn_dup_end_of(item(3, 1, 5, 90, 105, 191, 100), 1);
        CHECK(r.record == 3 && r.reverse == 1 && r.pos5 == 196 && r.pos3 == 95);
        CHECK(dcn_dup_end_of(item(3, 0, 5, 90, 105, 191, 100), 0).pos3 == 0); // without both_ends there is no pos3
        // negative: a forward read at a record's start, clipped by 7; a reverse read whose 3' end hangs over the start
        CHECK(dcn_dup_end_of(item(1, 0, 7, 100, 0, 93, 100), 0).pos5 == -7);
        CHECK(dcn_dup_end_of(item(1, 1, 0, 90, 0, 90, 100), 1).pos3 == -10);
        // past the record's end: a reverse read at the end of a record of 1000 bases, clipped by 4
        CHECK(dcn_dup_end_of(item(0, 1, 4, 100, 904, 1000, 100), 0).pos5 == 1004);
        // the largest coordinates a row can have stay exact in 64 bits
        CHECK(dcn_dup_end_of(item(0, 1, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0xFFFFFFFFull, 0xFFFFFFFFu), 0).pos5 == 0x1FFFFFFFEll);
        CHECK(dcn_dup_end_of(item(0, 0, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0, 0xFFFFFFFFu), 0).pos5 == -0xFFFFFFFFll);
    }
    // ---- clip equivalence ----
    CHECK(same(single(item(2, 0, 0, 100, 100, 200, 100), 0), single(item(2, 0, 5, 100, 105, 200, 100), 0)));
    CHECK(same(single(item(2, 0, 0, 100, 100, 200, 100), 1), single(item(2, 0, 5, 92, 105, 192, 100), 1)));
    CHECK(same(single(item(2, 1, 0, 100, 100, 200, 100), 0), single(item(2, 1, 6, 100, 100, 194, 100), 0)));
    CHECK(same(single(item(2, 1, 0, 100, 100, 200, 100), 1), single(item(2, 1, 6, 97, 103, 194, 100), 1)));
    // the 3' end does not matter without both_ends, and does with
    CHECK(same(single(item(2, 0, 0, 100, 100, 200, 100), 0), single(item(2, 0, 0, 80, 100, 180, 150), 0)));
    CHECK(!same(single(item(2, 0, 0, 100, 100, 200, 100), 1), single(item(2, 0, 0, 80, 100, 180, 150), 1)));
    // ---- negative pos5 and the neighbouring record ----
    {
        // record 0 has 1000 bases.  A: forward at the start of record 1, clipped by 5: pos5 = -5.  B: forward on record 0 at
        // 995 = 1000 - 5, where a coordinate over concatenated records would put A.  C: reverse on record 0 hanging 5 over its
        // end (pos5 = 1005) against D: forward on record 1 at 5
        const dcn_dup_key A = single(item(1, 0, 5, 100, 0, 95, 100), 0), B = single(item(0, 0, 0, 100, 995, 1000, 100), 0);
        CHECK(!same(A, B));
        CHECK((int64_t)A.w[2] == -5 && (int64_t)B.w[2] == 995);
        const dcn_dup_key Cc = single(item(0, 1, 5, 100, 905, 1000, 100), 0), D = single(item(1, 0, 0, 100, 5, 105, 100), 0);
        CHECK(!same(Cc, D));
        CHECK((int64_t)Cc.w[2] == 1005);
        CHECK(same(A, single(item(1, 0, 9, 100, 4, 95, 100), 0))); // -5 again, by another clip
        CHECK(!same(A, single(item(1, 0, 0, 100, 5, 105, 100), 0))); // +5 is not -5
    }
    // ---- the mate swap ----
    {
        const dcn_dup_item m1 = item(4, 0, 0, 100, 1000, 1100, 100), m2 = item(4, 1, 0, 100, 1300, 1400, 100);
        for (uint32_t be = 0; be < 2; ++be) {
            CHECK(same(pair(m1, m2, be), pair(m2, m1, be)));
            CHECK(same(pair(m1, none(), be), pair(none(), m1, be))); // one end, whichever mate has it
            CHECK(!same(pair(m1, m2, be), pair(m1, none(), be)));    // two ends against one
            CHECK(!same(pair(m1, none(), be), single(m1, be)));      // a lone mate of a pair against a single read
            CHECK(!dcn_dup_has_key(pair(none(), none(), be)) && !dcn_dup_has_key(single(none(), be)));
            CHECK(dcn_dup_has_key(pair(none(), m2, be)) && dcn_dup_has_key(single(m1, be)));
        }
        // the order of two ends is by (record, pos5, reverse, pos3): the sorted key holds the smaller first
        const dcn_dup_key k = pair(m2, m1, 1);
        CHECK((uint32_t)k.w[1] == 4 && (int64_t)k.w[2] == 1000 && (int64_t)k.w[4] == 1400 && ((k.w[0] >> 4) & 3) == 2);
        const dcn_dup_item lo = item(3, 1, 0, 100, 5000, 5100, 100);
        CHECK((uint32_t)pair(m1, lo, 0).w[1] == 3 && (uint32_t)(pair(m1, lo, 0).w[1] >> 32) == 4); // record before pos5
        // mates with the same record and pos5 but other strands: still one key under the swap
        const dcn_dup_item s1 = item(4, 0, 0, 100, 1000, 1100, 100), s2 = item(4, 1, 0, 100, 900, 1000, 100);
        CHECK(dcn_dup_end_of(s1, 0).pos5 == dcn_dup_end_of(s2, 0).pos5);
        CHECK(same(pair(s1, s2, 0), pair(s2, s1, 0)) && same(pair(s1, s2, 1), pair(s2, s1, 1)));
        // ... and with record, pos5 and strand equal, pos3 decides the order
        const dcn_dup_item t1 = item(4, 0, 0, 100, 1000, 1100, 100), t2 = item(4, 0, 0, 100, 1000, 1090, 100);
        CHECK(same(pair(t1, t2, 1), pair(t2, t1, 1)));
        CHECK(same(pair(t1, t2, 0), pair(t1, t1, 0))); // without both_ends the two are one end twice
    }
    // ---- every component alone ----
    {
        const dcn_dup_item base = item(2, 0, 0, 100, 100, 200, 100);
        const dcn_dup_key k0 = single(base, 0), k1 = single(base, 1);
        CHECK(!same(k0, single(item(3, 0, 0, 100, 100, 200, 100), 0)));  // record
        CHECK(!same(k0, single(item(2, 1, 0, 100, 0, 100, 100), 0)));    // strand, at the same pos5 = 100
        CHECK(dcn_dup_end_of(item(2, 1, 0, 100, 0, 100, 100), 0).pos5 == 100);
        CHECK(!same(k0, single(item(2, 0, 0, 100, 101, 201, 100), 0)));  // pos5 by 1
        CHECK(!same(k0, single(item(2, 0, 0, 100, 99, 199, 100), 0)));
        CHECK(!same(k1, single(item(2, 0, 0, 100, 100, 201, 100), 1)));  // pos3 by 1, only with both_ends
        CHECK(same(k0, single(item(2, 0, 0, 100, 100, 201, 100), 0)));
        CHECK(!same(k0, k1));                                           // the mode bit both_ends
        CHECK(!same(k0, pair(base, none(), 0)));                        // the mode bit paired
        CHECK(!same(pair(base, none(), 0), pair(base, none(), 1)));
        CHECK(!same(pair(base, none(), 0), pair(base, base, 0)));       // one end against two
        // the second end of a pair, component by component
        const dcn_dup_item m = item(2, 1, 0, 100, 300, 400, 100);
        const dcn_dup_key p1 = pair(base, m, 1);
        CHECK(!same(p1, pair(base, item(5, 1, 0, 100, 300, 400, 100), 1)));
        CHECK(!same(p1, pair(base, item(2, 0, 0, 100, 400, 500, 100), 1)));
        CHECK(!same(p1, pair(base, item(2, 1, 0, 100, 300, 401, 100), 1)));
        CHECK(!same(p1, pair(base, item(2, 1, 0, 100, 301, 400, 100), 1)));
        CHECK(same(pair(base, m, 0), pair(base, item(2, 1, 0, 100, 301, 400, 100), 0)));
    }
    // ---- equality is exact among many keys whose words differ in one bit ----
    {
        std::vector<dcn_dup_key> keys;
        for (int w = 0; w < 6; ++w)
            for (int b = 0; b < 64; b += 7) {
                dcn_dup_key k = pair(item(2, 0, 0, 100, 100, 200, 100), item(2, 1, 0, 100, 300, 400, 100), 1);
                k.w[w] ^= 1ull << b;
                keys.push_back(k);
            }
        for (size_t i = 0; i < keys.size(); ++i)
            for (size_t j = 0; j < keys.size(); ++j) CHECK(dcn_dup_key_equal(keys[i], keys[j]) == (i == j));
    }
    if (failures) {
        std::printf("duplicate key rule FAILED: %d of %d checks\n", failures, checks);
        return 1;
    }
    std::printf("duplicate key rule ok: %d checks\n", checks);
    return 0;
}

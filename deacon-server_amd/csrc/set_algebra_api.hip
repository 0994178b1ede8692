// set_algebra_api.hip -- the C ABI of set algebra beyond union and diff: dcn_index_set_select, dcn_index_set_overlap and
// dcn_index_intersect (the kernels are in set_algebra.hip).  Blocking, on the index's device; key 0, which has no slot,
// is decided here from has_zero / zero_label.
#include "dcn_ctx.h"
#include "dcn_derive.h"
#include "dcn_set_algebra.h"

#include <algorithm>
#include <vector>

using namespace dcn_impl;

extern "C" int dcn_index_set_select(const dcn_index *set, uint32_t all_of, uint32_t any_of, uint32_t none_of,
                                    uint32_t min_members, uint32_t max_members, uint64_t *n_selected, dcn_index **out) {
    if (out) *out = nullptr;
    if (n_selected) *n_selected = 0;
    if (!out && !n_selected) return dcn_fail(DCN_ERR_ARG, "out and n_selected are both NULL");
    if (max_members != 0 && min_members > max_members)
        return dcn_fail(DCN_ERR_ARG, "min_members " + std::to_string(min_members) + " > max_members " + std::to_string(max_members));
    DCN_TRY(check_set(set));
    const uint32_t n = set->n_members, members = n >= 32 ? ~0u : (1u << n) - 1;
    if ((all_of | any_of | none_of) & ~members)
        return dcn_fail(DCN_ERR_ARG, "a mask names a member at or above " + std::to_string(n) + ", the set's member count");
    const dcn_select_pred pred = {all_of, any_of, none_of, std::max(min_members, 1u),
                                  max_members == 0 ? DCN_MAX_SET_MEMBERS : std::min(max_members, DCN_MAX_SET_MEMBERS)};
    DCN_HIP(hipSetDevice(set->device));
    DevMem d_n;
    DCN_TRY(d_n.alloc(sizeof(unsigned long long), true, "select"));
    DCN_TRY(dcn_set_select_sweep(set, pred, nullptr, d_n.as<unsigned long long>()));
    unsigned long long counted = 0;
    DCN_TRY(read_count(d_n, "select", &counted));
    const bool zero = set->has_zero && dcn_select_pass(set->zero_label, pred);
    if (n_selected) *n_selected = counted + (zero ? 1 : 0);
    if (!out) return DCN_OK;
    dcn_index *idx = nullptr;
    int rc = new_index_like(set, counted + (zero ? 1 : 0), &idx);
    if (rc == DCN_OK) rc = d_n.clear("select");
    if (rc == DCN_OK) rc = dcn_set_select_sweep(set, pred, idx, d_n.as<unsigned long long>());
    return finish_build(rc, d_n, counted, zero, "select", idx, out);
}

extern "C" int dcn_index_set_overlap(const dcn_index *set, uint64_t *shared, uint64_t *exclusive, uint64_t *by_count) {
    if (!shared && !exclusive && !by_count) return dcn_fail(DCN_ERR_ARG, "shared, exclusive and by_count are all NULL");
    DCN_TRY(check_set(set));
    DCN_HIP(hipSetDevice(set->device));
    DevMem d_tally;
    DCN_TRY(d_tally.alloc(DCN_OVL_WORDS * sizeof(unsigned long long), true, "overlap"));
    DCN_TRY(dcn_set_overlap_sweep(set, d_tally.as<unsigned long long>()));
    std::vector<unsigned long long> t(DCN_OVL_WORDS);
    DCN_HIP(hipMemcpy(t.data(), d_tally.p, DCN_OVL_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    const uint32_t n = set->n_members, M = DCN_MAX_SET_MEMBERS;
    if (set->has_zero && set->zero_label) { // key 0 has no slot: its mask is tallied here, by the kernel's rule
        const uint32_t v = set->zero_label;
        if ((v & (v - 1)) == 0) {
            t[DCN_OVL_SINGLE + (__builtin_ffs(v) - 1)] += 1;
        } else {
            t[DCN_OVL_COUNT + __builtin_popcount(v) - 1] += 1;
            for (uint32_t i = 0; i < n; ++i)
                for (uint32_t j = i; j < n; ++j)
                    if ((v >> i) & (v >> j) & 1u) t[i * M + j] += 1;
        }
    }
    unsigned long long singles = 0;
    for (uint32_t j = 0; j < n; ++j) singles += t[DCN_OVL_SINGLE + j];
    for (uint32_t i = 0; i < n; ++i) {
        if (exclusive) exclusive[i] = t[DCN_OVL_SINGLE + i];
        if (by_count) by_count[i] = i == 0 ? singles : t[DCN_OVL_COUNT + i];
        for (uint32_t j = 0; shared && j < n; ++j)
            shared[(uint64_t)i * n + j] = t[std::min(i, j) * M + std::max(i, j)] + (i == j ? t[DCN_OVL_SINGLE + i] : 0);
    }
    return DCN_OK;
}

// The smallest input is swept once and each of its keys probed in the others, whatever their number: the hits are kept
// as one bit per slot, the result's table is allocated for their count, and a second sweep inserts the marked keys.
extern "C" int dcn_index_intersect(const dcn_index *const *inputs, uint32_t n, dcn_index **out) {
    if (!out) return dcn_fail(DCN_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!inputs || n == 0 || !inputs[0]) return dcn_fail(DCN_ERR_ARG, "at least one input index is required");
    const dcn_index *src = inputs[0];
    bool zero = true;
    for (uint32_t i = 0; i < n; ++i) {
        if (!inputs[i]) return dcn_fail(DCN_ERR_ARG, "input index is NULL");
        DCN_TRY(same_params(inputs[0], inputs[i]));
        if (inputs[i]->n_keys < src->n_keys) src = inputs[i];
        zero = zero && inputs[i]->has_zero;
    }
    std::vector<dcn_table_view> others;
    for (uint32_t i = 0; i < n; ++i)
        if (inputs[i] != src) others.push_back(inputs[i]->view());
    DCN_HIP(hipSetDevice(src->device));
    const uint64_t n_slots = src->n_groups * DCN_GROUP_SLOTS;
    DevMem d_n, d_bits, d_others;
    DCN_TRY(d_n.alloc(sizeof(unsigned long long), true, "intersect"));
    DCN_TRY(d_bits.alloc((n_slots + 63) / 64 * sizeof(unsigned long long), false, "intersect bitmap"));
    DCN_TRY(d_others.alloc(others.size() * sizeof(dcn_table_view), false, "intersect"));
    if (!others.empty())
        DCN_HIP(hipMemcpy(d_others.p, others.data(), others.size() * sizeof(dcn_table_view), hipMemcpyHostToDevice));
    DCN_TRY(dcn_intersect_mark(src, d_others.as<dcn_table_view>(), (uint32_t)others.size(), d_bits.as<unsigned long long>(),
                               d_n.as<unsigned long long>()));
    unsigned long long counted = 0;
    DCN_TRY(read_count(d_n, "intersect", &counted));
    dcn_index *idx = nullptr;
    int rc = new_index_like(src, counted + (zero ? 1 : 0), &idx);
    if (rc == DCN_OK) rc = d_n.clear("intersect");
    if (rc == DCN_OK) rc = dcn_intersect_build(src, d_bits.as<unsigned long long>(), idx, d_n.as<unsigned long long>());
    return finish_build(rc, d_n, counted, zero, "intersect", idx, out);
}

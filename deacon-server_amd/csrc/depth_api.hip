// depth_api.hip -- the C ABI of a set's depth counters: enable, reset and the three read-outs (kernels in depth.hip;
// classify_api.hip launches the counting sweep inside every classify call against a set that has counters).
#include "dcn_ctx.h"
#include "dcn_classify.h"
#include "dcn_depth.h"

#include <vector>

using namespace dcn_impl;

namespace {
int check_depth(const dcn_index *set) {
    DCN_TRY(check_set(set));
    if (!set->d_depth) return dcn_fail(DCN_ERR_ARG, "depth is not enabled on this set (dcn_index_set_depth_enable)");
    return DCN_OK;
}

int check_member(const dcn_index *set, uint32_t member, uint32_t *mask) {
    if (member != UINT32_MAX && member >= set->n_members)
        return dcn_fail(DCN_ERR_ARG, "member " + std::to_string(member) + " out of range: the set has " +
                                         std::to_string(set->n_members) + " members");
    *mask = member == UINT32_MAX ? ~0u : 1u << member;
    return DCN_OK;
}

// key 0's depth (it has no slot: the word behind the slots' counters); 0 when the set does not hold key 0
int zero_depth(const dcn_index *set, uint32_t *d0) {
    uint32_t w = 0;
    const hipError_t e = hipMemcpy(&w, set->d_depth + set->depth_words, sizeof(w), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return dcn_hip_fail(e, "depth");
    *d0 = set->has_zero ? (w & DCN_DEPTH_MAX) : 0u;
    return DCN_OK;
}
} // namespace

extern "C" int dcn_index_set_depth_enable(dcn_index *set, int enable) {
    DCN_TRY(check_set(set));
    DCN_HIP(hipSetDevice(set->device));
    if (!enable) {
        if (set->d_depth) hipFree(set->d_depth);
        set->d_depth = nullptr;
        set->depth_words = 0;
        return DCN_OK;
    }
    if (set->d_depth) return DCN_OK; // already on: the counts stay
    const uint64_t words = (set->n_groups * DCN_GROUP_SLOTS + 1) / 2;
    DCN_TRY(dev_alloc_zeroed(&set->d_depth, words + 1, "depth counters")); // (on failure the set is as it was)
    set->depth_words = words;
    return DCN_OK;
}

extern "C" int dcn_index_set_depth_reset(dcn_index *set) {
    DCN_TRY(check_depth(set));
    DCN_HIP(hipSetDevice(set->device));
    DCN_HIP(hipMemset(set->d_depth, 0, (set->depth_words + 1) * sizeof(uint32_t)));
    DCN_HIP(hipDeviceSynchronize());
    return DCN_OK;
}

extern "C" int dcn_index_set_depth_stats(const dcn_index *set, uint64_t *observed, uint64_t *sum, uint64_t *saturated) {
    DCN_TRY(check_depth(set));
    if (!observed || !sum || !saturated) return dcn_fail(DCN_ERR_ARG, "observed/sum/saturated is NULL");
    DCN_HIP(hipSetDevice(set->device));
    unsigned long long h[3 * DCN_MAX_SET_MEMBERS] = {};
    DCN_TRY(dcn_device_tally(3 * DCN_MAX_SET_MEMBERS, h, "depth stats", [&](unsigned long long *d) { return dcn_depth_stats(set, d, 0); }));
    uint32_t d0 = 0;
    DCN_TRY(zero_depth(set, &d0));
    for (uint32_t j = 0; j < set->n_members; ++j) {
        const bool zero = d0 && ((set->zero_label >> j) & 1u);
        observed[j] = h[j] + (zero ? 1 : 0);
        sum[j] = h[DCN_MAX_SET_MEMBERS + j] + (zero ? d0 : 0);
        saturated[j] = h[2 * DCN_MAX_SET_MEMBERS + j] + (zero && d0 == DCN_DEPTH_MAX ? 1 : 0);
    }
    return DCN_OK;
}

extern "C" int dcn_index_set_depth_hist(const dcn_index *set, uint32_t member, uint32_t n_bins, uint64_t *hist) {
    DCN_TRY(check_depth(set));
    if (!hist) return dcn_fail(DCN_ERR_ARG, "hist is NULL");
    uint32_t mask = 0;
    DCN_TRY(check_member(set, member, &mask));
    if (n_bins < 2 || n_bins > DCN_DEPTH_MAX_BINS)
        return dcn_fail(DCN_ERR_ARG, "n_bins must be 2 to " + std::to_string(DCN_DEPTH_MAX_BINS) + ", not " + std::to_string(n_bins));
    DCN_HIP(hipSetDevice(set->device));
    std::vector<unsigned long long> h(n_bins, 0);
    DCN_TRY(dcn_device_tally(n_bins, h.data(), "depth histogram",
                  [&](unsigned long long *d) { return dcn_depth_hist(set, mask, n_bins, d, 0); }));
    uint32_t d0 = 0;
    DCN_TRY(zero_depth(set, &d0));
    for (uint32_t b = 0; b < n_bins; ++b) hist[b] = h[b];
    if (set->has_zero && (set->zero_label & mask)) hist[std::min(d0, n_bins - 1)] += 1;
    return DCN_OK;
}

extern "C" int dcn_index_set_depth_keys(const dcn_index *set, uint32_t member, uint64_t *keys, uint32_t *depths,
                                        uint64_t capacity, uint64_t *n) {
    DCN_TRY(check_depth(set));
    if (!n) return dcn_fail(DCN_ERR_ARG, "n is NULL");
    *n = 0;
    uint32_t mask = 0;
    DCN_TRY(check_member(set, member, &mask));
    if ((!keys || !depths) && capacity > 0) return dcn_fail(DCN_ERR_ARG, "keys/depths is NULL");
    DCN_HIP(hipSetDevice(set->device));
    uint32_t d0 = 0;
    DCN_TRY(zero_depth(set, &d0));
    const bool zero = d0 && (set->zero_label & mask);
    const char *what = "depth keys";
    DevMem d_n, d_keys, d_depths;
    DCN_TRY(d_n.alloc(sizeof(unsigned long long), true, what));
    DCN_TRY(dcn_depth_keys(set, mask, nullptr, nullptr, 0, d_n.as<unsigned long long>(), 0));
    unsigned long long count = 0;
    DCN_TRY(read_count(d_n, what, &count));
    const uint64_t total = count + (zero ? 1 : 0);
    if (total > capacity) {
        *n = total;
        return dcn_fail(DCN_ERR_CAPACITY, "depth keys: " + std::to_string(total) + " observed keys, capacity " +
                                              std::to_string(capacity));
    }
    if (count > 0) {
        DCN_TRY(d_keys.alloc(count * sizeof(uint64_t), false, what));
        DCN_TRY(d_depths.alloc(count * sizeof(uint32_t), false, what));
        DCN_TRY(d_n.clear(what));
        DCN_TRY(dcn_depth_keys(set, mask, d_keys.as<uint64_t>(), d_depths.as<uint32_t>(), count, d_n.as<unsigned long long>(), 0));
        unsigned long long written = 0;
        DCN_TRY(read_count(d_n, what, &written));
        if (written != count)
            return dcn_fail(DCN_ERR_INTERNAL, "depth keys: the counters changed between the count and the copy (a classify call in flight?)");
        DCN_TRY(d_keys.read(keys, count * sizeof(uint64_t), what));
        DCN_TRY(d_depths.read(depths, count * sizeof(uint32_t), what));
    }
    *n = total;
    if (zero) {
        keys[count] = 0;
        depths[count] = d0;
    }
    return DCN_OK;
}

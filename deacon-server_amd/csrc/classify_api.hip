// classify_api.hip -- the C ABI of labelled index sets: creation, per-member coverage, and classification of a batch
// against a set (the kernels are in classify.hip; the batch runs the dump front end of ctx.hip on a filter context).
#include "dcn_ctx.h"
#include "dcn_classify.h"
#include "dcn_depth.h"

#include <cstring>

using namespace dcn_impl;

int dcn_impl::check_set(const dcn_index *set) {
    if (!set) return dcn_fail(DCN_ERR_ARG, "set is NULL");
    if (set->n_members == 0 || !set->d_labels) return dcn_fail(DCN_ERR_ARG, "index is not a labelled set (dcn_index_set_create)");
    return DCN_OK;
}

extern "C" int dcn_index_set_create(const dcn_index *const *members, uint32_t n, dcn_index **out) {
    if (!out) return dcn_fail(DCN_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!members) return dcn_fail(DCN_ERR_ARG, "members is NULL");
    if (n == 0 || n > DCN_MAX_SET_MEMBERS)
        return dcn_fail(DCN_ERR_ARG, "an index set has 1 to 32 members, not " + std::to_string(n));
    uint64_t sum = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (!members[i]) return dcn_fail(DCN_ERR_ARG, "member index " + std::to_string(i) + " is NULL");
        int rc = same_params(members[0], members[i]);
        if (rc != DCN_OK) return rc;
        sum += members[i]->n_keys; // worst case, as union sizes its table
    }
    dcn_index *set = new (std::nothrow) dcn_index();
    if (!set) return dcn_fail(DCN_ERR_NOMEM, "host allocation failed");
    set->device = members[0]->device;
    set->variant = members[0]->variant;
    set->k = members[0]->k;
    set->w = members[0]->w;
    int rc = dcn_table_alloc(set, std::max<uint64_t>(sum, 16));
    if (rc == DCN_OK) rc = dev_alloc_zeroed(&set->d_labels, set->n_groups * DCN_GROUP_SLOTS, "index set labels");
    set->n_members = n;
    for (uint32_t i = 0; i < n && rc == DCN_OK; ++i) rc = dcn_set_add_member(set, members[i], i);
    if (rc != DCN_OK) {
        dcn_index_destroy(set);
        return rc;
    }
    *out = set;
    return DCN_OK;
}

extern "C" void dcn_index_set_destroy(dcn_index *set) { dcn_index_destroy(set); }

extern "C" int dcn_index_set_info(const dcn_index *set, uint32_t *n_members, uint8_t *k, uint8_t *w, uint64_t *n_keys,
                                  uint64_t *table_bytes) {
    DCN_TRY(check_set(set));
    if (n_members) *n_members = set->n_members;
    if (k) *k = set->k;
    if (w) *w = set->w;
    if (n_keys) *n_keys = set->n_keys;
    if (table_bytes) *table_bytes = set->n_groups * DCN_GROUP_SLOTS * (sizeof(uint64_t) + sizeof(uint32_t));
    return DCN_OK;
}

// ---- coverage (classify.hip's COV kernels and sweeps) ---------------------------------------------------------------
namespace {
int check_coverage(const dcn_index *set) {
    DCN_TRY(check_set(set));
    if (!set->d_cov) return dcn_fail(DCN_ERR_ARG, "coverage is not enabled on this set (dcn_index_set_coverage_enable)");
    return DCN_OK;
}

// counts[0..n) of a coverage_count pass (all_slots: every occupied slot; else the marked ones), key 0 not included
int coverage_counts(const dcn_index *set, bool all_slots, uint64_t *counts) {
    unsigned long long h[DCN_MAX_SET_MEMBERS] = {};
    DCN_TRY(dcn_device_tally(DCN_MAX_SET_MEMBERS, h, "coverage",
                             [&](unsigned long long *d) { return dcn_coverage_count(set, all_slots, d, 0); }));
    for (uint32_t j = 0; j < set->n_members; ++j) counts[j] = h[j];
    return DCN_OK;
}

bool zero_observed(const dcn_index *set, int *rc) {
    uint32_t w = 0;
    const hipError_t e = hipMemcpy(&w, set->d_cov + set->cov_words, sizeof(w), hipMemcpyDeviceToHost);
    *rc = e == hipSuccess ? DCN_OK : dcn_hip_fail(e, "coverage");
    return (w & 1u) != 0;
}
} // namespace

extern "C" int dcn_index_set_coverage_enable(dcn_index *set, int enable) {
    DCN_TRY(check_set(set));
    DCN_HIP(hipSetDevice(set->device));
    if (!enable) {
        if (set->d_cov) hipFree(set->d_cov);
        set->d_cov = nullptr;
        set->cov_words = 0;
        return DCN_OK;
    }
    if (set->d_cov) return DCN_OK; // already on: the marks stay
    const uint64_t words = (set->n_groups * DCN_GROUP_SLOTS + 31) / 32;
    DCN_TRY(dev_alloc_zeroed(&set->d_cov, words + 1, "coverage bitmap"));
    set->cov_words = words;
    uint64_t keys[DCN_MAX_SET_MEMBERS] = {};
    int rc = coverage_counts(set, true, keys);
    if (rc != DCN_OK) {
        dcn_index_set_coverage_enable(set, 0);
        return rc;
    }
    for (uint32_t j = 0; j < set->n_members; ++j)
        set->cov_keys[j] = keys[j] + (set->has_zero && ((set->zero_label >> j) & 1u) ? 1 : 0);
    return DCN_OK;
}

extern "C" int dcn_index_set_coverage_reset(dcn_index *set) {
    DCN_TRY(check_coverage(set));
    DCN_HIP(hipSetDevice(set->device));
    DCN_HIP(hipMemset(set->d_cov, 0, (set->cov_words + 1) * sizeof(uint32_t)));
    DCN_HIP(hipDeviceSynchronize());
    return DCN_OK;
}

extern "C" int dcn_index_set_coverage(const dcn_index *set, uint64_t *observed, uint64_t *keys) {
    DCN_TRY(check_coverage(set));
    if (!observed || !keys) return dcn_fail(DCN_ERR_ARG, "observed/keys is NULL");
    DCN_HIP(hipSetDevice(set->device));
    uint64_t obs[DCN_MAX_SET_MEMBERS] = {};
    DCN_TRY(coverage_counts(set, false, obs));
    int rc = DCN_OK;
    const bool zero = zero_observed(set, &rc);
    DCN_TRY(rc);
    for (uint32_t j = 0; j < set->n_members; ++j) {
        observed[j] = obs[j] + (zero && ((set->zero_label >> j) & 1u) ? 1 : 0);
        keys[j] = set->cov_keys[j];
    }
    return DCN_OK;
}

extern "C" int dcn_index_set_coverage_keys(const dcn_index *set, uint32_t member, uint64_t *out, uint64_t capacity,
                                           uint64_t *n) {
    DCN_TRY(check_coverage(set));
    if (!n) return dcn_fail(DCN_ERR_ARG, "n is NULL");
    *n = 0;
    if (member != UINT32_MAX && member >= set->n_members)
        return dcn_fail(DCN_ERR_ARG, "member " + std::to_string(member) + " out of range: the set has " +
                                         std::to_string(set->n_members) + " members");
    if (!out && capacity > 0) return dcn_fail(DCN_ERR_ARG, "out is NULL");
    const uint32_t mask = member == UINT32_MAX ? ~0u : 1u << member;
    DCN_HIP(hipSetDevice(set->device));
    int rc = DCN_OK;
    const bool zero = zero_observed(set, &rc) && (set->zero_label & mask);
    DCN_TRY(rc);
    const char *what = "coverage keys";
    DevMem d_n, d_out;
    DCN_TRY(d_n.alloc(sizeof(unsigned long long), true, what));
    DCN_TRY(dcn_coverage_count_mask(set, mask, d_n.as<unsigned long long>(), 0));
    unsigned long long count = 0;
    DCN_TRY(read_count(d_n, what, &count));
    const uint64_t total = count + (zero ? 1 : 0);
    if (total > capacity) {
        *n = total;
        return dcn_fail(DCN_ERR_CAPACITY, "coverage keys: " + std::to_string(total) + " observed keys, capacity " +
                                              std::to_string(capacity));
    }
    if (count > 0) {
        DCN_TRY(d_out.alloc(count * sizeof(uint64_t), false, what));
        DCN_TRY(d_n.clear(what));
        DCN_TRY(dcn_coverage_collect(set, mask, d_out.as<uint64_t>(), count, d_n.as<unsigned long long>(), 0));
        unsigned long long written = 0;
        DCN_TRY(read_count(d_n, what, &written));
        if (written != count)
            return dcn_fail(DCN_ERR_INTERNAL, "coverage keys: the bitmap changed between the count and the copy (a classify call in flight?)");
        DCN_TRY(d_out.read(out, count * sizeof(uint64_t), what));
    }
    *n = total;
    if (zero) out[count] = 0;
    return DCN_OK;
}

namespace {
int classify_check(dcn_ctx *ctx, const dcn_index *set, const dcn_params *params) {
    if (!ctx) return dcn_fail(DCN_ERR_ARG, "ctx is NULL");
    DCN_TRY(check_set(set));
    DCN_TRY(check_params(params));
    return check_ctx_matches(ctx, set, "the set");
}

// the lazily allocated buffers of classification: the dump arrays, the work list and (host form) the outputs
int classify_buffers(dcn_ctx *c, const dcn_index *set, bool host_outputs) {
    const uint32_t n_members = set->n_members;
    DCN_TRY(ensure_dump_buffers(c));
    if (set->d_depth) DCN_TRY(ensure_position_bitmap(c)); // (the counting sweep's)
    if (!c->d_cls_big) {
        DCN_TRY(dev_alloc(&c->d_cls_big, c->max_reads, "classify work list"));
        DCN_TRY(dev_alloc(&c->d_cls_n_big, 1, "classify work list length"));
    }
    if (host_outputs) {
        if (!c->d_cls_match) {
            DCN_TRY(dev_alloc(&c->d_cls_match, c->max_reads, "classify match"));
            DCN_TRY(dev_alloc(&c->d_cls_total, c->max_reads, "classify total"));
        }
        if (c->cls_hits_members < n_members) {
            if (c->d_cls_hits) hipFree(c->d_cls_hits);
            c->d_cls_hits = nullptr;
            c->cls_hits_members = 0;
            DCN_TRY(dev_alloc(&c->d_cls_hits, (uint64_t)c->max_reads * n_members, "classify hits"));
            c->cls_hits_members = n_members;
        }
    }
    return DCN_OK;
}

// pack -> plan -> scan (minimizer dump) -> classification kernels, on the context's stream; the batch's inputs are
// device pointers (the host form has staged them into the context's buffers).  Leaves the six counters alone.
int classify_enqueue(dcn_ctx *c, const dcn_index *set, const uint8_t *d_ascii, const uint64_t *d_offsets,
                     const uint32_t *d_unit_id, uint32_t n_reads, uint64_t n_bases, uint32_t n_units,
                     const dcn_params *params, uint32_t *d_match, uint32_t *d_hits, uint32_t *d_total) {
    hipStream_t st = c->stream;
    DCN_HIP(hipMemsetAsync(c->d_status, 0, sizeof(dcn_status), st));
    DCN_HIP(hipMemsetAsync(c->d_cls_n_big, 0, sizeof(uint32_t), st));
    int prof_slot = -1;
    dcn_dump_view dump;
    // (the device form's offsets have not been seen by the host: the plan kernel checks them.  The classification
    // kernels do not look at the dump's positions; the depth sweep does.)
    DCN_TRY(dump_front_end(c, set, d_ascii, d_offsets, d_unit_id, n_reads, n_units, n_bases, params->prefix_length, true,
                           &prof_slot, &dump));
    if (set->d_depth) { // the counting sweep of depth.hip, timed with the lane kernel (no stage of its own: DCN_N_STAGES is ABI)
        DCN_HIP(hipMemsetAsync(c->d_loc_bits, 0, ((n_bases + 31) / 32 + 1) * sizeof(uint32_t), st));
        dcn_depth_args da;
        memset(&da, 0, sizeof(da));
        da.table = set->view();
        da.dump = dump;
        da.status = c->d_status;
        da.bits = c->d_loc_bits;
        da.depth = set->d_depth;
        da.depth_zero = set->has_zero ? set->d_depth + set->depth_words : nullptr;
        DCN_TRY(dcn_launch_depth_count(da, st));
    }
    dcn_classify_args ca;
    memset(&ca, 0, sizeof(ca));
    ca.table = set->view();
    ca.labels = set->d_labels;
    ca.zero_label = set->zero_label;
    ca.n_members = set->n_members;
    ca.tiles = dump.tiles;
    ca.n_tiles = dump.n_tiles;
    ca.offsets = d_offsets;
    ca.read_tiles = c->d_read_tiles;
    ca.read_tile_first = c->d_read_tile_first;
    ca.unit_first_read = d_unit_id ? c->d_unit_first_read : nullptr;
    ca.dump_hash = dump.hash;
    ca.dump_valid = dump.valid;
    ca.dump_count = dump.count;
    ca.tile_windows = c->tile_windows;
    ca.n_units = n_units;
    ca.abs_threshold = params->abs_threshold;
    ca.rel_threshold = params->rel_threshold;
    ca.match = d_match;
    ca.hits = d_hits;
    ca.total = d_total;
    ca.big = c->d_cls_big;
    ca.n_big = c->d_cls_n_big;
    ca.status = c->d_status;
    ca.report = c->d_report;
    ca.cov_bits = set->d_cov; // null: the kernels without coverage
    ca.cov_zero = set->d_cov ? set->d_cov + set->cov_words : nullptr;
    DCN_TRY(dcn_launch_classify_units(ca, st));
    DCN_PROF_MARK(DCN_STAGE_DISTINCT);
    DCN_TRY(dcn_launch_classify_big(ca, st));
    DCN_PROF_MARK(DCN_STAGE_FINISH);
    DCN_TRY(record_run_end(c, prof_slot));
    c->batch_pending = true; // dcn_ctx_synchronize reports what the plan kernel found wrong with the batch
    return DCN_OK;
}
} // namespace

extern "C" int dcn_classify_batch(dcn_ctx *ctx, const dcn_index *set, const uint8_t *bases, const uint64_t *offsets,
                                  const uint32_t *unit_id, uint32_t n_reads, const dcn_params *params, uint32_t *match,
                                  uint32_t *hits, uint32_t *total) {
    DCN_TRY(classify_check(ctx, set, params));
    if (n_reads == 0) return DCN_OK;
    if (!offsets || !match) return dcn_fail(DCN_ERR_ARG, "offsets/match is NULL");
    DCN_TRY(validate_host_batch(ctx, offsets, n_reads));
    uint32_t n_units = n_reads;
    if (unit_id) {
        if (unit_id[0] != 0) return dcn_fail(DCN_ERR_ARG, "unit_id[0] must be 0");
        for (uint32_t r = 1; r < n_reads; ++r)
            if (unit_id[r] != unit_id[r - 1] && unit_id[r] != unit_id[r - 1] + 1)
                return dcn_fail(DCN_ERR_ARG, "unit_id must be non-decreasing in steps of 0 or 1");
        n_units = unit_id[n_reads - 1] + 1;
    }
    const uint64_t n_bases = offsets[n_reads];
    if (n_bases > 0 && !bases) return dcn_fail(DCN_ERR_ARG, "bases is NULL");
    dcn_ctx *c = ctx;
    DCN_HIP(hipSetDevice(c->device));
    DCN_TRY(classify_buffers(c, set, true));
    DCN_TRY(stage_batch(c, bases, n_bases, offsets, n_reads, unit_id));
    DCN_TRY(classify_enqueue(c, set, c->d_ascii, c->d_offsets, unit_id ? c->d_unit_id : nullptr, n_reads, n_bases, n_units,
                             params, c->d_cls_match, c->d_cls_hits, c->d_cls_total));
    DCN_TRY(sync_and_check(c, nullptr));
    DCN_HIP(hipMemcpy(match, c->d_cls_match, (uint64_t)n_units * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (hits)
        DCN_HIP(hipMemcpy(hits, c->d_cls_hits, (uint64_t)n_units * set->n_members * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (total) DCN_HIP(hipMemcpy(total, c->d_cls_total, (uint64_t)n_units * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return DCN_OK;
}

extern "C" int dcn_classify_batch_device(dcn_ctx *ctx, const dcn_index *set, const uint8_t *d_bases,
                                         const uint64_t *d_offsets, const uint32_t *d_unit_id, uint32_t n_reads,
                                         uint64_t n_bases, uint32_t n_units, const dcn_params *params, uint32_t *d_match,
                                         uint32_t *d_hits, uint32_t *d_total) {
    DCN_TRY(classify_check(ctx, set, params));
    if (n_reads == 0) return DCN_OK;
    if (!d_bases || !d_offsets || !d_match) return dcn_fail(DCN_ERR_ARG, "d_bases/d_offsets/d_match is NULL");
    DCN_TRY(check_device_batch(ctx, n_reads, n_bases, n_units, d_unit_id));
    DCN_HIP(hipSetDevice(ctx->device));
    DCN_TRY(classify_buffers(ctx, set, false));
    return classify_enqueue(ctx, set, d_bases, d_offsets, d_unit_id, n_reads, n_bases, n_units, params, d_match, d_hits,
                            d_total);
}

// index_builder_api.hip -- the C ABI of the counting index build: dcn_index_builder_create / _add / _info / _hist /
// _counts / _finish / _destroy (kernels in index_builder.hip; the chunk loop is dump.hip's, shared with dcn_index_build).
// Blocking, on the builder's device; key 0, which has no slot, is decided here from has_zero and its own counter word.
#include "dcn_ctx.h"
#include "dcn_derive.h"
#include "dcn_index_builder.h"

#include <algorithm>
#include <cstdlib>
#include <vector>

using namespace dcn_impl;

namespace {
int check_builder(const dcn_index_builder *b) {
    if (!b) return dcn_fail(DCN_ERR_ARG, "builder is NULL");
    return DCN_OK;
}

// key 0's count (0 while the builder has not met key 0)
int zero_count(const dcn_index_builder *b, uint32_t *c0) {
    uint32_t w = 0;
    const hipError_t e = hipMemcpy(&w, b->d_counts + b->count_words, sizeof(w), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return dcn_hip_fail(e, "index builder");
    *c0 = b->idx.has_zero ? (w & DCN_DEPTH_MAX) : 0u;
    return DCN_OK;
}

// dcn_table_reserve for a table with counters: a larger table, every key re-inserted, its counter moved to its new slot
int builder_reserve(dcn_index_builder *b, uint64_t n_keys_capacity) {
    dcn_index *idx = &b->idx;
    const uint64_t want = dcn_table_groups_for(n_keys_capacity);
    if (want <= idx->n_groups) return DCN_OK;
    if (want > (1ull << 32)) return dcn_fail(DCN_ERR_CAPACITY, "index too large for 2^32 groups");
    dcn_index grown = *idx; // (a view of the new table; owns nothing)
    grown.n_groups = want;
    grown.d_slots = nullptr;
    const uint64_t words = dcn_builder_count_words(&grown), old_n = idx->n_groups * DCN_GROUP_SLOTS;
    uint32_t *counts = nullptr;
    hipError_t e = dcn_table_malloc(&grown.d_slots, want * DCN_GROUP_SLOTS * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMalloc((void **)&counts, (words + 1) * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemset(grown.d_slots, 0, want * DCN_GROUP_SLOTS * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMemset(counts, 0, (words + 1) * sizeof(uint32_t));
    int rc = DCN_OK;
    if (e == hipSuccess) {
        const dcn_table_view v = grown.view();
        rc = dcn_builder_rehash(idx->d_slots, b->d_counts, old_n, grown.d_slots, v.group_shift, v.group_mask, counts, 0);
    }
    if (e == hipSuccess && rc == DCN_OK)
        e = hipMemcpy(counts + words, b->d_counts + b->count_words, sizeof(uint32_t), hipMemcpyDeviceToDevice);
    if (e == hipSuccess && rc == DCN_OK) e = hipDeviceSynchronize();
    if (e != hipSuccess || rc != DCN_OK) { // (the builder is as it was)
        if (grown.d_slots) hipFree(grown.d_slots);
        if (counts) hipFree(counts);
        return rc != DCN_OK ? rc : dcn_hip_fail(e, "index builder growth");
    }
    hipFree(idx->d_slots);
    hipFree(b->d_counts);
    idx->d_slots = grown.d_slots;
    idx->n_groups = want;
    b->d_counts = counts;
    b->count_words = words;
    return DCN_OK;
}

// the front end, made by the first add and kept: the chunk size is read then
int ensure_front_end(dcn_index_builder *b) {
    if (b->ctx) return DCN_OK;
    // a piece is cut only where its chunk ends (dump.hip caps a piece at 0xFFFFFF00 bases: never reached below 2^31)
    b->chunk_bases = std::min<uint64_t>(build_chunk_bases(), 1ull << 31);
    DCN_TRY(dev_alloc(&b->d_bits, (b->chunk_bases + 31) / 32 + 1, "position bitmap"));
    DCN_TRY(dev_alloc(&b->d_seam, DCN_BUILDER_SEAM_WORDS + 1, "seam bits"));
    const double t0 = build_now();
    DCN_TRY(dcn_ctx_create(&b->idx, b->chunk_bases, DCN_BUILD_MAX_PIECES, &b->ctx));
    b->front_end_s = build_now() - t0;
    b->timing = getenv("DCN_INDEX_TIMING") != nullptr;
    return b->timing ? build_timing_begin(b->ctx) : DCN_OK;
}

// one chunk's dump into the table and the counters
int count_chunk(dcn_index_builder *b, uint64_t nb, bool continues) {
    dcn_ctx *c = b->ctx;
    dcn_index *idx = &b->idx;
    hipStream_t st = c->stream;
    const uint32_t seam = (uint32_t)idx->k + idx->w - 2; // l - 1: what two pieces of a cut sequence share
    uint64_t n_valid = 0;
    DCN_TRY(dcn_table_count_valid(c->d_dump_valid, nb, &n_valid, st));
    const double t_grow = build_now();
    DCN_TRY(builder_reserve(b, idx->n_keys + n_valid)); // the insert loop always finds an empty slot
    b->growth_s += build_now() - t_grow;
    DCN_HIP(hipMemsetAsync(b->d_bits, 0, ((nb + 31) / 32 + 1) * sizeof(uint32_t), st));
    DCN_HIP(hipMemsetAsync(b->d_tally, 0, 3 * sizeof(unsigned long long), st));
    // the positions the chunk before this one counted in its last l-1 bases are this chunk's first l-1
    if (continues) DCN_TRY(dcn_launch_builder_seam(b->d_seam, 0, b->d_bits, 0, seam, st));
    const dcn_table_view v = idx->view();
    dcn_builder_count_args a;
    a.slots = idx->d_slots;
    a.group_shift = v.group_shift;
    a.group_mask = v.group_mask;
    a.dump_hash = c->d_dump_hash;
    a.dump_valid = c->d_dump_valid;
    a.dump_pos = c->d_dump_pos;
    a.n_bases = nb;
    a.ascii = c->d_ascii;
    a.k = idx->k;
    a.entropy_threshold = b->entropy_threshold;
    a.bits = b->d_bits;
    a.counts = b->d_counts;
    a.counts_zero = b->d_counts + b->count_words;
    a.tally = b->d_tally;
    DCN_TRY(dcn_launch_builder_count(a, st));
    DCN_HIP(hipMemsetAsync(b->d_seam, 0, (DCN_BUILDER_SEAM_WORDS + 1) * sizeof(uint32_t), st));
    if (nb >= seam) DCN_TRY(dcn_launch_builder_seam(b->d_bits, nb - seam, b->d_seam, 0, seam, st));
    unsigned long long t[3] = {0, 0, 0};
    DCN_HIP(hipMemcpyAsync(t, b->d_tally, sizeof(t), hipMemcpyDeviceToHost, st));
    DCN_HIP(hipStreamSynchronize(st));
    idx->n_keys += t[0] + ((t[2] && !idx->has_zero) ? 1 : 0);
    idx->has_zero = idx->has_zero || t[2] != 0;
    b->n_occurrences += t[1];
    return DCN_OK;
}
} // namespace

extern "C" int dcn_index_builder_create(uint8_t k, uint8_t w, float entropy_threshold, uint64_t capacity_keys, int device,
                                        void **out) {
    if (!out) return dcn_fail(DCN_ERR_ARG, "out is NULL");
    *out = nullptr;
    DCN_TRY(check_kw(k, w));
    if (!(entropy_threshold >= 0.0f && entropy_threshold <= 1.0f)) return dcn_fail(DCN_ERR_ARG, "entropy_threshold must be in [0, 1]");
    int ndev = 0;
    DCN_TRY(dcn_device_count(&ndev));
    if (device < 0 || device >= ndev) return dcn_fail(DCN_ERR_ARG, "no such HIP device");
    dcn_index_builder *b = new (std::nothrow) dcn_index_builder();
    if (!b) return dcn_fail(DCN_ERR_NOMEM, "host allocation failed");
    b->idx.device = device;
    b->idx.k = k;
    b->idx.w = w;
    b->entropy_threshold = entropy_threshold;
    int rc = dcn_table_alloc(&b->idx, std::max<uint64_t>(capacity_keys, 1024));
    if (rc == DCN_OK) {
        b->count_words = dcn_builder_count_words(&b->idx);
        rc = dev_alloc(&b->d_counts, b->count_words + 1, "counters");
    }
    if (rc == DCN_OK) rc = dev_alloc(&b->d_tally, 3, "tally");
    if (rc == DCN_OK) {
        hipError_t e = hipMemset(b->d_counts, 0, (b->count_words + 1) * sizeof(uint32_t));
        if (e == hipSuccess) e = hipDeviceSynchronize(); // (the front end's stream does not wait for the null stream)
        if (e != hipSuccess) rc = dcn_hip_fail(e, "index builder counters");
    }
    if (rc != DCN_OK) {
        dcn_index_builder_destroy(b);
        return rc;
    }
    *out = b;
    return DCN_OK;
}

extern "C" int dcn_index_builder_add(void *builder, const uint8_t *bases, const uint64_t *offsets, uint32_t n_seqs) {
    dcn_index_builder *b = (dcn_index_builder *)builder;
    DCN_TRY(check_builder(b));
    if (n_seqs == 0) return DCN_OK;
    if (!offsets) return dcn_fail(DCN_ERR_ARG, "offsets is NULL");
    if (offsets[0] != 0) return dcn_fail(DCN_ERR_ARG, "offsets[0] must be 0");
    for (uint32_t i = 0; i < n_seqs; ++i)
        if (offsets[i + 1] < offsets[i]) return dcn_fail(DCN_ERR_ARG, "offsets must be non-decreasing");
    if (offsets[n_seqs] > 0 && !bases) return dcn_fail(DCN_ERR_ARG, "bases is NULL");
    DCN_HIP(hipSetDevice(b->idx.device));
    DCN_TRY(ensure_front_end(b));
    build_times times;
    DCN_TRY(build_run_chunks(b->ctx, &b->idx, bases, offsets, n_seqs, b->chunk_bases,
                             [&](uint64_t nb, bool continues) { return count_chunk(b, nb, continues); }, b->timing ? &times : nullptr));
    b->staging_s += times.staging_s;
    b->n_bases += offsets[n_seqs];
    return DCN_OK;
}

extern "C" int dcn_index_builder_info(const void *builder, uint64_t *n_keys, uint64_t *n_occurrences, uint64_t *n_bases,
                                      uint64_t *device_bytes) {
    const dcn_index_builder *b = (const dcn_index_builder *)builder;
    DCN_TRY(check_builder(b));
    if (n_keys) *n_keys = b->idx.n_keys;
    if (n_occurrences) *n_occurrences = b->n_occurrences;
    if (n_bases) *n_bases = b->n_bases;
    if (device_bytes)
        *device_bytes = b->idx.n_groups * DCN_GROUP_SLOTS * sizeof(uint64_t) + (b->count_words + 1) * sizeof(uint32_t) +
                        (b->d_bits ? ((b->chunk_bases + 31) / 32 + 1) * sizeof(uint32_t) : 0);
    return DCN_OK;
}

extern "C" int dcn_index_builder_hist(const void *builder, uint32_t n_bins, uint64_t *hist) {
    const dcn_index_builder *b = (const dcn_index_builder *)builder;
    if (!hist) return dcn_fail(DCN_ERR_ARG, "hist is NULL");
    if (n_bins < 2 || n_bins > DCN_DEPTH_MAX_BINS)
        return dcn_fail(DCN_ERR_ARG, "n_bins must be 2 to " + std::to_string(DCN_DEPTH_MAX_BINS) + ", not " + std::to_string(n_bins));
    DCN_TRY(check_builder(b));
    DCN_HIP(hipSetDevice(b->idx.device));
    std::vector<unsigned long long> h(n_bins, 0);
    DCN_TRY(dcn_device_tally(n_bins, h.data(), "index builder histogram",
                             [&](unsigned long long *d) { return dcn_builder_hist(b, n_bins, d, 0); }));
    uint32_t c0 = 0;
    DCN_TRY(zero_count(b, &c0));
    for (uint32_t i = 0; i < n_bins; ++i) hist[i] = h[i];
    if (b->idx.has_zero) hist[std::min(c0, n_bins - 1)] += 1;
    return DCN_OK;
}

extern "C" int dcn_index_builder_counts(const void *builder, uint64_t *keys, uint32_t *counts, uint64_t capacity, uint64_t *n) {
    const dcn_index_builder *b = (const dcn_index_builder *)builder;
    if (!n) return dcn_fail(DCN_ERR_ARG, "n is NULL");
    *n = 0;
    DCN_TRY(check_builder(b));
    if ((!keys || !counts) && capacity > 0) return dcn_fail(DCN_ERR_ARG, "keys/counts is NULL");
    const uint64_t total = b->idx.n_keys, n_nonzero = total - (b->idx.has_zero ? 1 : 0);
    *n = total;
    if (total > capacity)
        return dcn_fail(DCN_ERR_CAPACITY, "index builder counts: " + std::to_string(total) + " keys, capacity " + std::to_string(capacity));
    if (total == 0) return DCN_OK;
    DCN_HIP(hipSetDevice(b->idx.device));
    if (n_nonzero) {
        DevMem d_n, d_keys, d_counts;
        DCN_TRY(d_n.alloc(sizeof(unsigned long long), true, "index builder counts"));
        DCN_TRY(d_keys.alloc(n_nonzero * sizeof(uint64_t), false, "index builder counts"));
        DCN_TRY(d_counts.alloc(n_nonzero * sizeof(uint32_t), false, "index builder counts"));
        DCN_TRY(dcn_builder_export(b, d_keys.as<uint64_t>(), d_counts.as<uint32_t>(), n_nonzero, d_n.as<unsigned long long>(), 0));
        unsigned long long written = 0;
        DCN_TRY(read_count(d_n, "index builder counts", &written));
        if (written != n_nonzero)
            return dcn_fail(DCN_ERR_INTERNAL, "index builder counts: the table holds " + std::to_string(written) + " keys, the builder counted " +
                                                  std::to_string(n_nonzero));
        DCN_HIP(hipMemcpy(keys, d_keys.p, n_nonzero * sizeof(uint64_t), hipMemcpyDeviceToHost));
        DCN_HIP(hipMemcpy(counts, d_counts.p, n_nonzero * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    if (b->idx.has_zero) {
        uint32_t c0 = 0;
        DCN_TRY(zero_count(b, &c0));
        keys[n_nonzero] = 0;
        counts[n_nonzero] = c0;
    }
    return DCN_OK;
}

extern "C" int dcn_index_builder_finish(const void *builder, uint32_t min_count, uint32_t max_count, uint64_t *n_selected,
                                        dcn_index **out) {
    const dcn_index_builder *b = (const dcn_index_builder *)builder;
    if (out) *out = nullptr;
    if (n_selected) *n_selected = 0;
    if (!out && !n_selected) return dcn_fail(DCN_ERR_ARG, "out and n_selected are both NULL");
    if (min_count > DCN_DEPTH_MAX || max_count > DCN_DEPTH_MAX)
        return dcn_fail(DCN_ERR_ARG, "min_count / max_count above " + std::to_string(DCN_DEPTH_MAX) + ", where a count saturates");
    if (max_count != 0 && min_count > max_count)
        return dcn_fail(DCN_ERR_ARG, "min_count " + std::to_string(min_count) + " > max_count " + std::to_string(max_count));
    DCN_TRY(check_builder(b));
    const uint32_t lo = std::max(min_count, 1u), hi = max_count == 0 ? DCN_DEPTH_MAX : max_count;
    DCN_HIP(hipSetDevice(b->idx.device));
    const double t0 = build_now();
    DevMem d_n;
    DCN_TRY(d_n.alloc(sizeof(unsigned long long), true, "index builder finish"));
    DCN_TRY(dcn_builder_select(b, lo, hi, nullptr, d_n.as<unsigned long long>(), 0));
    unsigned long long counted = 0;
    DCN_TRY(read_count(d_n, "index builder finish", &counted));
    uint32_t c0 = 0;
    DCN_TRY(zero_count(b, &c0));
    const bool zero = b->idx.has_zero && c0 >= lo && c0 <= hi;
    if (n_selected) *n_selected = counted + (zero ? 1 : 0);
    if (!out) return DCN_OK;
    dcn_index *idx = nullptr;
    const double t_table = build_now();
    int rc = new_index_like(&b->idx, counted + (zero ? 1 : 0), &idx);
    const double table_s = build_now() - t_table;
    if (rc == DCN_OK) rc = d_n.clear("index builder finish");
    if (rc == DCN_OK) rc = dcn_builder_select(b, lo, hi, idx, d_n.as<unsigned long long>(), 0);
    rc = finish_build(rc, d_n, counted, zero, "index builder finish", idx, out);
    if (b->timing && rc == DCN_OK) {
        build_times t;
        t.front_end_s = b->front_end_s;
        t.staging_s = b->staging_s;
        t.growth_s = b->growth_s;
        t.finish_s = build_now() - t0;
        t.finish_table_s = table_s;
        (void)build_times_print("counting", b->ctx, t); // (the index is made: a lost report is no reason to fail)
    }
    return rc;
}

extern "C" void dcn_index_builder_destroy(void *builder) {
    dcn_index_builder *b = (dcn_index_builder *)builder;
    if (!b) return;
    hipSetDevice(b->idx.device);
    if (b->ctx) dcn_ctx_destroy(b->ctx);
    if (b->idx.d_slots) hipFree(b->idx.d_slots);
    if (b->d_counts) hipFree(b->d_counts);
    if (b->d_bits) hipFree(b->d_bits);
    if (b->d_seam) hipFree(b->d_seam);
    if (b->d_tally) hipFree(b->d_tally);
    delete b;
}

// track_api.hip -- the C ABI of dcn_depth_track_batch: the depth track of every read of a host batch (kernels in
// track.hip; the batch runs the dump front end of ctx.hip on a filter context).
#include "dcn_ctx.h"
#include "dcn_track.h"

#include <cstring>

using namespace dcn_impl;

static_assert(sizeof(dcn_track_params) == 24 && sizeof(dcn_track_bin) == 24, "track structs are ABI");

namespace {
int track_check(dcn_ctx *ctx, const dcn_index *set, const dcn_track_params *p, const uint64_t *bin_offsets) {
    // (the parameters first: what is wrong with them does not depend on the context or the set)
    if (!p) return dcn_fail(DCN_ERR_ARG, "params is NULL");
    if (p->reserved != 0) return dcn_fail(DCN_ERR_ARG, "params.reserved must be 0");
    if (p->member_mask == 0) return dcn_fail(DCN_ERR_ARG, "params.member_mask must select a member");
    if (p->depth_cap > DCN_DEPTH_MAX) return dcn_fail(DCN_ERR_ARG, "params.depth_cap must be at most 65535");
    if (!bin_offsets) return dcn_fail(DCN_ERR_ARG, "bin_offsets is NULL");
    if (!ctx) return dcn_fail(DCN_ERR_ARG, "ctx is NULL");
    if (!set) return dcn_fail(DCN_ERR_ARG, "set is NULL");
    DCN_TRY(check_set(set));
    if (!set->d_depth) return dcn_fail(DCN_ERR_ARG, "depth is not enabled on this set (dcn_index_set_depth_enable)");
    if (set->n_members < 32 && (p->member_mask >> set->n_members) != 0)
        return dcn_fail(DCN_ERR_ARG, "params.member_mask has a bit at or above the set's member count (" +
                                         std::to_string(set->n_members) + ")");
    return check_ctx_matches(ctx, set, "the set");
}

int track_buffers(dcn_ctx *c) {
    DCN_TRY(ensure_dump_buffers(c));
    DCN_TRY(ensure_position_bitmap(c));
    DCN_TRY(ensure_position_words(c));
    if (!c->d_trk_bin_offsets) {
        DCN_TRY(dev_alloc(&c->d_trk_bin_offsets, (uint64_t)c->max_reads + 1, "track bin offsets"));
        DCN_TRY(dev_alloc(&c->d_trk_piece_offsets, (uint64_t)c->max_reads + 1, "track piece offsets"));
    }
    return DCN_OK;
}

int grow_bins(dcn_ctx *c, uint64_t need) {
    if (need <= c->trk_bin_cap) return DCN_OK;
    if (c->d_trk_bins) hipFree(c->d_trk_bins);
    c->d_trk_bins = nullptr;
    c->trk_bin_cap = 0;
    const uint64_t cap = std::max<uint64_t>(need + need / 4, 1u << 12);
    DCN_TRY(dev_alloc(&c->d_trk_bins, cap, "track bins"));
    c->trk_bin_cap = cap;
    return DCN_OK;
}
} // namespace

extern "C" int dcn_depth_track_batch(dcn_ctx *ctx, const dcn_index *set, const uint8_t *bases, const uint64_t *offsets,
                                     uint32_t n_reads, const void *params, uint64_t *bin_offsets, void *bins, uint64_t capacity) {
    const dcn_track_params *prm = static_cast<const dcn_track_params *>(params);
    DCN_TRY(track_check(ctx, set, prm, bin_offsets));
    bin_offsets[0] = 0;
    if (n_reads == 0) return DCN_OK;
    if (!offsets) return dcn_fail(DCN_ERR_ARG, "offsets is NULL");
    if (!bins && capacity > 0) return dcn_fail(DCN_ERR_ARG, "bins is NULL");
    DCN_TRY(validate_host_batch(ctx, offsets, n_reads));
    const uint64_t n_bases = offsets[n_reads];
    if (n_bases > 0 && !bases) return dcn_fail(DCN_ERR_ARG, "bases is NULL");
    // the bins follow from the offsets alone: the caller has them, and the capacity is checked, before any device work
    std::vector<uint64_t> piece_offsets((size_t)n_reads + 1);
    piece_offsets[0] = 0;
    for (uint32_t r = 0; r < n_reads; ++r) {
        const uint64_t len = offsets[r + 1] - offsets[r];
        const uint64_t nb = dcn_track_read_bins(len, prm->bin_bases);
        bin_offsets[r + 1] = bin_offsets[r] + nb;
        piece_offsets[r + 1] = piece_offsets[r] + nb * dcn_track_bin_pieces(len, prm->bin_bases);
    }
    const uint64_t total = bin_offsets[n_reads];
    if (total > capacity)
        return dcn_fail(DCN_ERR_CAPACITY, "track: " + std::to_string(total) + " bins, capacity " + std::to_string(capacity));
    if (total == 0) return DCN_OK;
    dcn_ctx *c = ctx;
    DCN_HIP(hipSetDevice(c->device));
    DCN_TRY(track_buffers(c));
    DCN_TRY(grow_bins(c, total));
    DCN_TRY(staged_h2d(c, c->d_trk_bin_offsets, bin_offsets, ((uint64_t)n_reads + 1) * sizeof(uint64_t)));
    DCN_TRY(staged_h2d(c, c->d_trk_piece_offsets, piece_offsets.data(), ((uint64_t)n_reads + 1) * sizeof(uint64_t)));
    DCN_TRY(stage_batch(c, bases, n_bases, offsets, n_reads, nullptr));
    hipStream_t st = c->stream;
    DCN_HIP(hipMemsetAsync(c->d_status, 0, sizeof(dcn_status), st));
    DCN_HIP(hipMemsetAsync(c->d_loc_bits, 0, ((n_bases + 31) / 32 + 1) * sizeof(uint32_t), st));
    int prof_slot = -1;
    dcn_track_args ta;
    memset(&ta, 0, sizeof(ta));
    DCN_TRY(dump_front_end(c, set, c->d_ascii, c->d_offsets, nullptr, n_reads, n_reads, n_bases, prm->prefix_length, false,
                           &prof_slot, &ta.dump));
    ta.table = set->view();
    ta.labels = set->d_labels;
    ta.zero_label = set->zero_label;
    ta.member_mask = prm->member_mask;
    ta.depth = set->d_depth;
    ta.depth_zero = set->has_zero ? set->d_depth + set->depth_words : nullptr;
    ta.depth_cap = prm->depth_cap;
    ta.offsets = c->d_offsets;
    ta.n_reads = n_reads;
    ta.bin_bases = prm->bin_bases;
    ta.bin_offsets = c->d_trk_bin_offsets;
    ta.piece_offsets = c->d_trk_piece_offsets;
    ta.n_bins = total;
    ta.n_pieces = piece_offsets[n_reads];
    ta.bits = c->d_loc_bits;
    ta.value = c->d_loc_labels;
    ta.bins = c->d_trk_bins;
    DCN_TRY(dcn_launch_track_mark(ta, st));
    DCN_PROF_MARK(DCN_STAGE_DISTINCT);
    DCN_TRY(dcn_launch_track_reduce(ta, st));
    DCN_PROF_MARK(DCN_STAGE_FINISH);
    DCN_TRY(finish_run(c, prof_slot));
    DCN_HIP(hipMemcpy(bins, c->d_trk_bins, total * sizeof(dcn_track_bin), hipMemcpyDeviceToHost));
    return DCN_OK;
}

// track_api.hip -- the C ABI of dcn_depth_track_batch: the depth track of every read of a host batch (kernels in
// track.hip; the batch runs locate's front end, pack -> plan -> scan in dump mode, on a filter context).
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
    const dcn_index *ix = ctx->index;
    if (ix->k != set->k || ix->w != set->w)
        return dcn_fail(DCN_ERR_ARG, "the context's index (k=" + std::to_string((int)ix->k) + ", w=" + std::to_string((int)ix->w) +
                                         ") and the set (k=" + std::to_string((int)set->k) + ", w=" + std::to_string((int)set->w) +
                                         ") differ");
    if (ix->device != set->device) return dcn_fail(DCN_ERR_ARG, "the context and the set live on different devices");
    if (ix->variant != set->variant)
        return dcn_fail(DCN_ERR_ARG, "the context's index and the set were created under different minimizer rules");
    return check_idle(ctx);
}

int track_buffers(dcn_ctx *c) {
    DCN_TRY(ensure_dump_buffers(c));
    // (either may be there already: classify with depth and locate use the bitmap, locate on a set the word per base)
    if (!c->d_loc_bits) DCN_TRY(dev_alloc(&c->d_loc_bits, (c->max_bases + 31) / 32 + 1, "position bitmap"));
    if (!c->d_loc_labels) DCN_TRY(dev_alloc(&c->d_loc_labels, c->max_bases + 2, "track values"));
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
    DCN_TRY(prof_begin(c, &prof_slot));
    DCN_TRY(dcn_launch_pack(c->d_ascii, 0, n_bases, c->d_packed + DCN_FRONT_PAD, c->d_invmask + DCN_FRONT_PAD, c->d_status, st));
    DCN_PROF_MARK(DCN_STAGE_PACK);
    // (check_offsets stays 0: validate_host_batch has walked the offsets on the host)
    dcn_plan_args pa = plan_args(c, set, c->d_ascii, c->d_offsets, nullptr, n_reads, n_reads, prm->prefix_length);
    pa.read_tiles = c->d_read_tiles;
    pa.read_tile_first = c->d_read_tile_first;
    DCN_TRY(dcn_launch_plan(pa, st));
    DCN_PROF_MARK(DCN_STAGE_PLAN);
    dcn_scan_args sa = dump_scan_args(c, set, n_bases);
    sa.dump_abs = 1;
    const uint32_t max_tiles = tile_bound(c, n_reads, n_bases);
    DCN_TRY(dcn_launch_scan(sa, max_tiles, true, st));
    DCN_PROF_MARK(DCN_STAGE_SCAN);
    dcn_track_args ta;
    memset(&ta, 0, sizeof(ta));
    ta.table = set->view();
    ta.labels = set->d_labels;
    ta.zero_label = set->zero_label;
    ta.member_mask = prm->member_mask;
    ta.depth = set->d_depth;
    ta.depth_zero = set->has_zero ? set->d_depth + set->depth_words : nullptr;
    ta.depth_cap = prm->depth_cap;
    ta.tiles = c->d_tiles;
    ta.n_tiles = &c->d_status->n_tiles;
    ta.dump_hash = c->d_dump_hash;
    ta.dump_valid = c->d_dump_valid;
    ta.dump_pos = c->d_dump_pos;
    ta.dump_count = c->d_dump_count;
    ta.max_tiles = max_tiles;
    ta.n_bases = n_bases;
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
    if (prof_slot >= 0) c->prof_used[prof_slot] = true;
    // a later device-pointer filter batch packs one batch ahead into these packed buffers on its own stream, after the
    // events below: they now stand after this run
    if (c->pack_ahead_state == 1) {
        DCN_HIP(hipEventRecord(c->plan_done, st));
        for (int i = 0; i < 2; ++i) DCN_HIP(hipEventRecord(c->buf_free[i], st));
    }
    DCN_TRY(sync_and_check(c, nullptr));
    DCN_HIP(hipMemcpy(bins, c->d_trk_bins, total * sizeof(dcn_track_bin), hipMemcpyDeviceToHost));
    return DCN_OK;
}

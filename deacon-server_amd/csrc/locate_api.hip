// locate_api.hip -- the C ABI of dcn_locate_batch: the segments of every read of a host batch (kernels in locate.hip;
// the batch runs the dump front end of ctx.hip on a filter context).
#include "dcn_ctx.h"
#include "dcn_locate.h"

#include <cstring>

using namespace dcn_impl;

namespace {
int locate_check(dcn_ctx *ctx, const dcn_index *index, const dcn_locate_params *p, const uint64_t *seg_offsets) {
    // (the parameters first: what is wrong with them does not depend on the context)
    if (!p) return dcn_fail(DCN_ERR_ARG, "params is NULL");
    if (p->reserved != 0) return dcn_fail(DCN_ERR_ARG, "params.reserved must be 0");
    if (p->min_hits == 0) return dcn_fail(DCN_ERR_ARG, "params.min_hits must be at least 1");
    if (!seg_offsets) return dcn_fail(DCN_ERR_ARG, "seg_offsets is NULL");
    if (!ctx) return dcn_fail(DCN_ERR_ARG, "ctx is NULL");
    if (!index) return dcn_fail(DCN_ERR_ARG, "index is NULL");
    return check_ctx_matches(ctx, index, "the set"); // (also where `index` is a plain index: the messages are ABI)
}

int locate_buffers(dcn_ctx *c, bool labelled) {
    DCN_TRY(ensure_dump_buffers(c));
    DCN_TRY(ensure_position_bitmap(c));
    if (!c->d_loc_counts) {
        DCN_TRY(dev_alloc(&c->d_loc_counts, c->max_reads, "locate counts"));
        DCN_TRY(dev_alloc(&c->d_loc_block_sums, (uint64_t)c->max_reads / DCN_SCAN_BLOCK + 1, "locate block sums"));
        DCN_TRY(dev_alloc(&c->d_loc_seg_offsets, (uint64_t)c->max_reads + 1, "locate segment offsets"));
        DCN_TRY(dev_alloc(&c->d_loc_big, c->max_reads, "locate work list"));
        DCN_TRY(dev_alloc(&c->d_loc_n_big, 1, "locate work list length"));
    }
    if (labelled) DCN_TRY(ensure_position_words(c));
    return DCN_OK;
}

int grow_segments(dcn_ctx *c, uint64_t need) {
    if (need <= c->loc_seg_cap) return DCN_OK;
    if (c->d_loc_segs) hipFree(c->d_loc_segs);
    c->d_loc_segs = nullptr;
    c->loc_seg_cap = 0;
    const uint64_t cap = std::max<uint64_t>(need + need / 4, 1u << 16);
    DCN_TRY(dev_alloc(&c->d_loc_segs, cap, "locate segments"));
    c->loc_seg_cap = cap;
    return DCN_OK;
}
} // namespace

extern "C" int dcn_locate_batch(dcn_ctx *ctx, const dcn_index *index, const uint8_t *bases, const uint64_t *offsets,
                                uint32_t n_reads, const void *params, uint64_t *seg_offsets, void *segs, uint64_t capacity) {
    const dcn_locate_params *prm = static_cast<const dcn_locate_params *>(params);
    DCN_TRY(locate_check(ctx, index, prm, seg_offsets));
    seg_offsets[0] = 0;
    if (n_reads == 0) return DCN_OK;
    if (!offsets) return dcn_fail(DCN_ERR_ARG, "offsets is NULL");
    if (!segs && capacity > 0) return dcn_fail(DCN_ERR_ARG, "segs is NULL");
    DCN_TRY(validate_host_batch(ctx, offsets, n_reads));
    const uint64_t n_bases = offsets[n_reads];
    if (n_bases > 0 && !bases) return dcn_fail(DCN_ERR_ARG, "bases is NULL");
    dcn_ctx *c = ctx;
    DCN_HIP(hipSetDevice(c->device));
    const bool labelled = index->n_members != 0 && index->d_labels;
    DCN_TRY(locate_buffers(c, labelled));
    DCN_TRY(grow_segments(c, 1));
    DCN_TRY(stage_batch(c, bases, n_bases, offsets, n_reads, nullptr));
    hipStream_t st = c->stream;
    DCN_HIP(hipMemsetAsync(c->d_status, 0, sizeof(dcn_status), st));
    DCN_HIP(hipMemsetAsync(c->d_loc_bits, 0, ((n_bases + 31) / 32 + 1) * sizeof(uint32_t), st));
    int prof_slot = -1;
    dcn_locate_args la;
    memset(&la, 0, sizeof(la));
    DCN_TRY(dump_front_end(c, index, c->d_ascii, c->d_offsets, nullptr, n_reads, n_reads, n_bases, prm->prefix_length, false,
                           &prof_slot, &la.dump));
    la.table = index->view();
    la.labels = labelled ? index->d_labels : nullptr;
    la.zero_label = labelled ? index->zero_label : (index->has_zero ? 1u : 0u);
    la.member_mask = labelled ? prm->member_mask : ~0u;
    la.offsets = c->d_offsets;
    la.n_reads = n_reads;
    la.k = index->k;
    la.join = (uint32_t)std::min<uint64_t>((uint64_t)index->k + prm->max_gap, 0xFFFFFFFFull);
    la.min_hits = prm->min_hits;
    la.bits = c->d_loc_bits;
    la.label_scratch = c->d_loc_labels;
    la.counts = c->d_loc_counts;
    la.block_sums = c->d_loc_block_sums;
    la.seg_offsets = c->d_loc_seg_offsets;
    la.segs = c->d_loc_segs;
    la.seg_cap = c->loc_seg_cap;
    la.big = c->d_loc_big;
    la.n_big = c->d_loc_n_big;
    DCN_TRY(dcn_launch_locate_mark(la, st));
    DCN_PROF_MARK(DCN_STAGE_DISTINCT);
    // the write pass is enqueued behind the count without the host having seen the total: it leaves out what does not
    // fit the segment buffer, and is run again after the buffer has grown (the first calls of a context only)
    DCN_TRY(dcn_launch_locate_count(la, st));
    DCN_TRY(dcn_launch_locate_write(la, st));
    DCN_PROF_MARK(DCN_STAGE_FINISH);
    DCN_TRY(finish_run(c, prof_slot));
    DCN_HIP(hipMemcpy(seg_offsets, c->d_loc_seg_offsets, ((uint64_t)n_reads + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    const uint64_t total = seg_offsets[n_reads];
    if (total > capacity)
        return dcn_fail(DCN_ERR_CAPACITY, "locate: " + std::to_string(total) + " segments, capacity " + std::to_string(capacity));
    if (total > c->loc_seg_cap) {
        DCN_TRY(grow_segments(c, total));
        la.segs = c->d_loc_segs;
        la.seg_cap = c->loc_seg_cap;
        DCN_TRY(dcn_launch_locate_write(la, st));
        DCN_HIP(hipStreamSynchronize(st));
    }
    if (total) DCN_HIP(hipMemcpy(segs, c->d_loc_segs, total * sizeof(dcn_segment), hipMemcpyDeviceToHost));
    return DCN_OK;
}

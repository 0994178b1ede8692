// extend_api.hip -- the C ABI of extended placements (dcn_extend_batch; kernel in extend.hip, the shared arithmetic in
// dcn_extend.h).  The once-only checks, the walk over the rows and the front end are every row call's (rows_check,
// rows_walk, rows_front; dcn_verify.h): the walk resolves every placed row to its two flanks, and the answers of the
// flanks are put together here by rule X6.
#include "dcn_ctx.h"
#include "dcn_extend.h"
#include "dcn_verify.h"

#include <cstring>

using namespace dcn_impl;

static_assert(sizeof(dcn_extend_params) == 24, "extend params are ABI");
static_assert(sizeof(dcn_extension) == 32, "extension rows are ABI");

namespace {
// One flank of a placed row (rule X2, and dcn_extend.h on which side is read backwards).  `left` is in the record's
// direction.
dcn_extend_item flank_item(const dcn_placement &p, bool left, uint64_t read_off, uint64_t read_len, uint64_t rec_start, uint64_t rec_len,
                           const dcn_extend_params &prm) {
    dcn_extend_item it;
    memset(&it, 0, sizeof(it));
    // R' runs against the read when the row is reverse: its left flank is what lies behind read_end
    const bool u_back = left != (p.reverse != 0);
    it.f = u_back ? p.read_start : (uint32_t)(read_len - p.read_end);
    it.g = (uint32_t)(left ? p.ref_start : rec_len - p.ref_end);
    it.u_origin = (int64_t)(read_off + (u_back ? p.read_start : p.read_end));
    it.v_origin = (int64_t)(rec_start + (left ? p.ref_start : p.ref_end));
    it.flags = (u_back ? 1u : 0u) | (left ? 2u : 0u);
    it.cap = dcn_ext_cap(it.f, it.g, prm.penalty, prm.end_bonus, prm.max_edits);
    return it;
}
} // namespace

extern "C" int dcn_extend_batch(dcn_ctx *ctx, const dcn_index *map, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                                const void *params, const uint64_t *row_offsets, const void *rows, uint64_t n_rows, void *out) {
    const dcn_extend_params *prm = static_cast<const dcn_extend_params *>(params);
    // (the parameters first, in dcn_verify_batch's order: what is wrong with them does not depend on the context or the map)
    if (!prm) return dcn_fail(DCN_ERR_ARG, "params is NULL");
    if (prm->reserved[0] != 0 || prm->reserved[1] != 0) return dcn_fail(DCN_ERR_ARG, "params.reserved must be 0");
    if (prm->penalty < 2 || prm->penalty > 255) return dcn_fail(DCN_ERR_ARG, "params.penalty must be 2..255");
    if (prm->end_bonus > 65535) return dcn_fail(DCN_ERR_ARG, "params.end_bonus must be 0..65535");
    const dcn_row_call call = {ctx, map, bases, offsets, n_reads, prm->max_edits, 0u, prm->row_stride, row_offsets, rows, n_rows};
    bool run = false;
    uint64_t n_bases = 0;
    DCN_TRY(rows_check(call, &run, &n_bases));
    if (!run) return DCN_OK;

    // every row is checked: two flanks of each
    std::vector<dcn_extend_item> items(2 * n_rows);
    uint32_t cap_max = 0;
    const int rc = rows_walk(call, [&](uint64_t row, const dcn_placement &p, uint64_t read_off, uint64_t read_len, uint64_t rec_start, uint64_t rec_len) {
        if (p.record == UINT32_MAX) {
            memset(&items[2 * row], 0, 2 * sizeof(dcn_extend_item));
            items[2 * row].flags = items[2 * row + 1].flags = 4u;
            return;
        }
        for (int side = 0; side < 2; ++side) {
            dcn_extend_item &it = items[2 * row + side];
            it = flank_item(p, side == 0, read_off, read_len, rec_start, rec_len, *prm);
            cap_max = std::max(cap_max, it.cap);
        }
    });
    DCN_TRY(rc);
    if (!out) return dcn_fail(DCN_ERR_ARG, "out is NULL");

    dcn_ctx *c = ctx;
    const uint64_t n_items = items.size();
    hipStream_t st = c->stream;
    int prof_slot = -1;
    DCN_HIP(hipSetDevice(c->device));
    DCN_TRY(grow(&c->d_ext_items, &c->ext_items_cap, n_items, "extend flanks"));
    DCN_TRY(grow(&c->d_ext_out, &c->ext_out_cap, n_items, "extend results"));
    DCN_TRY(rows_front(c, c->d_ext_items, items.data(), n_items * sizeof(dcn_extend_item), bases, n_bases, offsets, n_reads, &prof_slot));
    const dcn_base_store *store = map->store;
    dcn_extend_args xa;
    memset(&xa, 0, sizeof(xa));
    xa.items = c->d_ext_items;
    xa.n_items = n_items;
    xa.s_packed = c->d_packed + DCN_FRONT_PAD;
    xa.s_invmask = c->d_invmask + DCN_FRONT_PAD;
    xa.t_packed = store->d_packed;
    xa.t_invmask = store->d_invmask;
    xa.lds_stride = 2 * cap_max + 1;
    xa.penalty = prm->penalty;
    xa.end_bonus = prm->end_bonus;
    xa.out = c->d_ext_out;
    DCN_TRY(dcn_launch_extend(xa, st));
    DCN_PROF_MARK(DCN_STAGE_FINISH);
    DCN_TRY(finish_run(c, prof_slot));
    std::vector<dcn_extend_result> res(n_items);
    DCN_HIP(hipMemcpy(res.data(), c->d_ext_out, n_items * sizeof(dcn_extend_result), hipMemcpyDeviceToHost));

    // rule X6 (X7 for an unplaced row)
    dcn_extension *const ext = static_cast<dcn_extension *>(out);
    for (uint64_t row = 0; row < n_rows; ++row) {
        dcn_placement p;
        memcpy(&p, static_cast<const uint8_t *>(rows) + row * prm->row_stride, sizeof(p));
        dcn_extension e;
        memset(&e, 0, sizeof(e));
        e.read_start = p.read_start, e.read_end = p.read_end, e.ref_start = p.ref_start, e.ref_end = p.ref_end;
        if (p.record != UINT32_MAX) {
            const dcn_extend_result &l = res[2 * row], &r = res[2 * row + 1];
            e.read_start -= p.reverse ? r.i : l.i;
            e.read_end += p.reverse ? l.i : r.i;
            e.ref_start -= l.j;
            e.ref_end += r.j;
            e.left_edits = l.d;
            e.right_edits = r.d;
        }
        memcpy(ext + row, &e, sizeof(e));
    }
    return DCN_OK;
}

// verify_api.hip -- the C ABI of kept reference bases (dcn_anchor_map_keep_bases, dcn_anchor_map_fetch), the store behind
// them (dcn_verify.h; dcn_anchor_map_add of place_api.hip appends to it), the host side that every row call shares (the
// once-only checks rows_check, the front end rows_front; the walk rows_walk is a template in dcn_verify.h) and
// dcn_verify_batch (kernel in verify.hip).  Its checks with the walk over the rows (dcn_verify_walk) and its front end and
// launch (dcn_verify_enqueue) are functions of their own: dcn_align_batch and dcn_pileup_batch begin with the same two.
#include "dcn_ctx.h"
#include "dcn_verify.h"

#include <cstdlib>
#include <cstring>

using namespace dcn_impl;

static_assert(sizeof(dcn_verify_params) == 16, "verify params are ABI");

namespace {
int check_map(const dcn_index *map) {
    if (!map) return dcn_fail(DCN_ERR_ARG, "map is NULL");
    if (!map->d_anchor) return dcn_fail(DCN_ERR_ARG, "the index is not an anchor map (dcn_anchor_map_create)");
    return DCN_OK;
}

// bases the store starts with: DCN_STORE_INITIAL_BASES, or the test hook DCN_ANCHOR_STORE_BASES, read at call time
uint64_t initial_bases() {
    const char *s = std::getenv("DCN_ANCHOR_STORE_BASES");
    const uint64_t v = s && *s ? std::strtoull(s, nullptr, 10) : DCN_STORE_INITIAL_BASES;
    return std::max<uint64_t>((v + 31) / 32 * 32, 32);
}

// `cap` bases of store: both arrays with their pads, zeroed, holding the first `used` bases of `s`
int store_resize(dcn_base_store *s, uint64_t cap) {
    const uint64_t pw = cap / 16 + DCN_STORE_PAD_WORDS, mw = cap / 32 + DCN_STORE_PAD_WORDS;
    uint32_t *p = nullptr, *m = nullptr;
    hipError_t e = hipMalloc((void **)&p, pw * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&m, mw * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemset(p, 0, pw * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemset(m, 0, mw * sizeof(uint32_t));
    if (e == hipSuccess && s->used) e = hipMemcpy(p, s->d_packed, s->used / 16 * sizeof(uint32_t), hipMemcpyDeviceToDevice);
    if (e == hipSuccess && s->used) e = hipMemcpy(m, s->d_invmask, s->used / 32 * sizeof(uint32_t), hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize(); // (null-stream work must not be overtaken by the context's stream)
    if (e != hipSuccess) {
        if (p) hipFree(p);
        if (m) hipFree(m);
        return dcn_hip_fail(e, "kept bases");
    }
    if (s->d_packed) hipFree(s->d_packed);
    if (s->d_invmask) hipFree(s->d_invmask);
    s->d_packed = p;
    s->d_invmask = m;
    s->cap = cap;
    return DCN_OK;
}
} // namespace

int dcn_impl::check_store(const dcn_index *map) {
    DCN_TRY(check_map(map));
    if (!map->store) return dcn_fail(DCN_ERR_ARG, "the map keeps no bases (dcn_anchor_map_keep_bases before the first add)");
    return DCN_OK;
}

int dcn_impl::check_range(const dcn_index *map, const char *who, uint32_t record, uint64_t start, uint64_t n_bases, uint64_t *base0) {
    const dcn_base_store *s = map->store;
    if (record >= s->rec_len.size())
        return dcn_fail(DCN_ERR_ARG, std::string(who) + ": record " + std::to_string(record) + " of " + std::to_string(s->rec_len.size()) + " added");
    const uint64_t len = s->rec_len[record];
    if (start > len || n_bases > len - start)
        return dcn_fail(DCN_ERR_ARG, std::string(who) + ": bases [" + std::to_string(start) + ", " + std::to_string(start) + " + " +
                                         std::to_string(n_bases) + ") are past the record's " + std::to_string(len) + " bases");
    *base0 = s->rec_start[record] + start;
    return DCN_OK;
}

void dcn_base_store_free(dcn_base_store *s) {
    if (!s) return;
    if (s->d_packed) hipFree(s->d_packed);
    if (s->d_invmask) hipFree(s->d_invmask);
    delete s;
}

int dcn_base_store_append(dcn_base_store *s, const uint32_t *packed, const uint32_t *invmask, uint64_t n_bases, hipStream_t stream,
                          uint64_t *batch_start) {
    *batch_start = s->used;
    const uint64_t groups = (n_bases + 31) / 32, need = s->used + groups * 32;
    if (need > s->cap) { // geometric: at least twice what there was
        const uint64_t cap = std::max<uint64_t>(std::max<uint64_t>(need, 2 * s->cap), initial_bases());
        DCN_TRY(store_resize(s, cap));
    }
    if (groups == 0) return DCN_OK;
    // (the pack kernel writes whole 32-base groups: bases behind n_bases are 'A' and valid, and no record reaches them)
    DCN_HIP(hipMemcpyAsync(s->d_packed + s->used / 16, packed, groups * 2 * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
    DCN_HIP(hipMemcpyAsync(s->d_invmask + s->used / 32, invmask, groups * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
    return DCN_OK;
}

void dcn_base_store_commit(dcn_base_store *s, uint64_t batch_start, const uint64_t *offsets, uint32_t n_records) {
    for (uint32_t r = 0; r < n_records; ++r) {
        s->rec_start.push_back(batch_start + offsets[r]);
        s->rec_len.push_back((uint32_t)(offsets[r + 1] - offsets[r]));
    }
    s->used = batch_start + (offsets[n_records] + 31) / 32 * 32;
}

extern "C" int dcn_anchor_map_keep_bases(dcn_index *map) {
    DCN_TRY(check_map(map));
    if (map->store) return DCN_OK;
    if (map->anchor_records != 0)
        return dcn_fail(DCN_ERR_ARG, "dcn_anchor_map_keep_bases comes before the first dcn_anchor_map_add: the map has records already");
    map->store = new (std::nothrow) dcn_base_store();
    if (!map->store) return dcn_fail(DCN_ERR_NOMEM, "host allocation failed");
    return DCN_OK;
}

extern "C" int dcn_anchor_map_fetch(const dcn_index *map, uint32_t record, uint64_t start, uint64_t n_bases, uint8_t *out) {
    DCN_TRY(check_store(map));
    const dcn_base_store *s = map->store;
    uint64_t b0 = 0;
    DCN_TRY(check_range(map, "fetch", record, start, n_bases, &b0));
    if (n_bases == 0) return DCN_OK;
    if (!out) return dcn_fail(DCN_ERR_ARG, "out is NULL");
    DCN_HIP(hipSetDevice(map->device));
    const uint64_t b1 = b0 + n_bases;
    const uint64_t pw0 = b0 / 16, pw1 = (b1 + 15) / 16, mw0 = b0 / 32, mw1 = (b1 + 31) / 32;
    std::vector<uint32_t> p(pw1 - pw0), m(mw1 - mw0);
    DCN_HIP(hipMemcpy(p.data(), s->d_packed + pw0, p.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    DCN_HIP(hipMemcpy(m.data(), s->d_invmask + mw0, m.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (uint64_t b = b0; b < b1; ++b) {
        const uint32_t code = (p[b / 16 - pw0] >> (2 * (b % 16))) & 3u, inv = (m[b / 32 - mw0] >> (b % 32)) & 1u;
        out[b - b0] = inv ? 'N' : "ACTG"[code];
    }
    return DCN_OK;
}

int dcn_impl::rows_check(const dcn_row_call &call, bool *run, uint64_t *n_bases) {
    *run = false;
    *n_bases = 0;
    if (call.max_edits > DCN_VERIFY_MAX_EDITS)
        return dcn_fail(DCN_ERR_ARG, "params.max_edits must be 0.." + std::to_string(DCN_VERIFY_MAX_EDITS));
    if (call.max_permille > 1000) return dcn_fail(DCN_ERR_ARG, "params.max_permille must be 0..1000");
    DCN_TRY(rows_stride_check(call.row_stride));
    if (!call.ctx) return dcn_fail(DCN_ERR_ARG, "ctx is NULL");
    DCN_TRY(check_store(call.map));
    DCN_TRY(check_ctx_matches(call.ctx, call.map, "the map"));
    return rows_shape_check(call, run, n_bases);
}

int dcn_impl::rows_stride_check(uint32_t row_stride) {
    if (row_stride < sizeof(dcn_placement) || row_stride % 8 != 0)
        return dcn_fail(DCN_ERR_ARG, "params.row_stride must be at least 48 and a multiple of 8");
    return DCN_OK;
}

int dcn_impl::rows_shape_check(const dcn_row_call &call, bool *run, uint64_t *n_bases) {
    *run = false;
    *n_bases = 0;
    const uint32_t n_reads = call.n_reads;
    const uint64_t *const offsets = call.offsets, *const row_offsets = call.row_offsets;
    if (!row_offsets && call.n_rows != n_reads)
        return dcn_fail(DCN_ERR_ARG, "without row_offsets row r belongs to read r: n_rows must equal n_reads");
    if (n_reads == 0) {
        if (call.n_rows != 0) return dcn_fail(DCN_ERR_ARG, "row_offsets must end at n_rows");
        return DCN_OK;
    }
    if (!offsets) return dcn_fail(DCN_ERR_ARG, "offsets is NULL");
    if (call.ctx) DCN_TRY(validate_host_batch(call.ctx, offsets, n_reads));
    else DCN_TRY(check_offsets_walk(offsets, n_reads, "offsets", "read longer than 2^32 bases"));
    *n_bases = offsets[n_reads];
    if (call.ctx && *n_bases > 0 && !call.bases) return dcn_fail(DCN_ERR_ARG, "bases is NULL");
    if (row_offsets) {
        if (row_offsets[0] != 0) return dcn_fail(DCN_ERR_ARG, "row_offsets[0] must be 0");
        for (uint32_t r = 0; r < n_reads; ++r)
            if (row_offsets[r + 1] < row_offsets[r]) return dcn_fail(DCN_ERR_ARG, "row_offsets must be non-decreasing");
        if (row_offsets[n_reads] != call.n_rows) return dcn_fail(DCN_ERR_ARG, "row_offsets must end at n_rows");
    }
    if (call.n_rows == 0) return DCN_OK;
    if (!call.rows) return dcn_fail(DCN_ERR_ARG, "rows is NULL");
    *run = true;
    return DCN_OK;
}

int dcn_impl::rows_front(dcn_ctx *c, void *d_items, const void *items, uint64_t item_bytes, const uint8_t *bases, uint64_t n_bases,
                         const uint64_t *offsets, uint32_t n_reads, int *prof_slot_out) {
    DCN_TRY(staged_h2d(c, d_items, items, item_bytes));
    DCN_TRY(stage_batch(c, bases, n_bases, offsets, n_reads, nullptr));
    hipStream_t st = c->stream;
    DCN_HIP(hipMemsetAsync(c->d_status, 0, sizeof(dcn_status), st)); // (short_batch = 0: the pack kernel packs)
    int prof_slot = -1;
    DCN_TRY(prof_begin(c, &prof_slot));
    *prof_slot_out = prof_slot;
    DCN_TRY(dcn_launch_pack(c->d_ascii, 0, n_bases, c->d_packed + DCN_FRONT_PAD, c->d_invmask + DCN_FRONT_PAD, c->d_status, st));
    DCN_PROF_MARK(DCN_STAGE_PACK);
    DCN_PROF_MARK(DCN_STAGE_PLAN);
    DCN_PROF_MARK(DCN_STAGE_SCAN);
    DCN_PROF_MARK(DCN_STAGE_DISTINCT);
    return DCN_OK;
}

// The checks of dcn_verify_batch, dcn_align_batch and dcn_pileup_batch, in the order their messages promise, and the
// walk over the rows: what the kernel gets is resolved to stream positions here.  plan->items stays empty when the call
// has nothing to run (no reads or no rows).
int dcn_verify_walk(dcn_ctx *ctx, const dcn_index *map, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                    const void *params, const uint64_t *row_offsets, const void *rows, uint64_t n_rows, const uint32_t *edits,
                    dcn_verify_plan *plan) {
    plan->items.clear();
    plan->e_max = 0;
    plan->n_bases = 0;
    const dcn_verify_params *prm = static_cast<const dcn_verify_params *>(params);
    // (the parameters first: what is wrong with them does not depend on the context or the map)
    if (!prm) return dcn_fail(DCN_ERR_ARG, "params is NULL");
    if (prm->reserved != 0) return dcn_fail(DCN_ERR_ARG, "params.reserved must be 0");
    const dcn_row_call call = {ctx, map, bases, offsets, n_reads, prm->max_edits, prm->max_permille, prm->row_stride, row_offsets, rows, n_rows};
    bool run = false;
    DCN_TRY(rows_check(call, &run, &plan->n_bases));
    if (!run) return DCN_OK;
    if (!edits) return dcn_fail(DCN_ERR_ARG, "edits is NULL");

    std::vector<dcn_verify_item> &items = plan->items;
    items.resize(n_rows);
    uint32_t e_max = 0;
    const int rc = rows_walk(call, [&](uint64_t row, const dcn_placement &p, uint64_t read_off, uint64_t, uint64_t rec_start, uint64_t) {
        dcn_verify_item &it = items[row];
        memset(&it, 0, sizeof(it));
        if (p.record == UINT32_MAX) {
            it.flags = 2u;
            return;
        }
        it.m = p.read_end - p.read_start;
        it.n = (uint32_t)(p.ref_end - p.ref_start);
        it.E = (uint32_t)std::min<uint64_t>(prm->max_edits, (uint64_t)std::max(it.m, it.n) * prm->max_permille / 1000);
        it.flags = p.reverse;
        it.s_origin = (int64_t)(read_off + (p.reverse ? p.read_end : p.read_start));
        it.t_origin = (int64_t)(rec_start + p.ref_start);
        const uint64_t gap = it.m > it.n ? it.m - it.n : it.n - it.m;
        if (gap <= it.E) e_max = std::max(e_max, it.E); // (a row whose lengths differ by more is OVER without a wavefront)
    });
    DCN_TRY(rc);
    plan->e_max = e_max;
    return DCN_OK;
}

// The front end and the verify kernel: the run is left open behind the DISTINCT mark, its results in c->d_vfy_out.  The
// caller marks FINISH and ends the run (finish_run).
int dcn_verify_enqueue(dcn_ctx *c, const dcn_index *map, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                       const dcn_verify_plan &plan, int *prof_slot_out) {
    const dcn_base_store *store = map->store;
    const uint64_t n_rows = plan.items.size();
    *prof_slot_out = -1;
    DCN_HIP(hipSetDevice(c->device));
    DCN_TRY(grow(&c->d_vfy_items, &c->vfy_items_cap, n_rows, "verify rows"));
    DCN_TRY(grow(&c->d_vfy_out, &c->vfy_out_cap, n_rows, "verify edits"));
    DCN_TRY(rows_front(c, c->d_vfy_items, plan.items.data(), n_rows * sizeof(dcn_verify_item), bases, plan.n_bases, offsets, n_reads, prof_slot_out));
    dcn_verify_args va;
    memset(&va, 0, sizeof(va));
    va.items = c->d_vfy_items;
    va.n_rows = n_rows;
    va.s_packed = c->d_packed + DCN_FRONT_PAD;
    va.s_invmask = c->d_invmask + DCN_FRONT_PAD;
    va.t_packed = store->d_packed;
    va.t_invmask = store->d_invmask;
    va.lds_stride = (2 * plan.e_max + 1 + 3) / 4 * 4;
    va.out = c->d_vfy_out;
    DCN_TRY(dcn_launch_verify(va, c->stream));
    return DCN_OK;
}

extern "C" int dcn_verify_batch(dcn_ctx *ctx, const dcn_index *map, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                                const void *params, const uint64_t *row_offsets, const void *rows, uint64_t n_rows, uint32_t *edits) {
    dcn_verify_plan plan;
    DCN_TRY(dcn_verify_walk(ctx, map, bases, offsets, n_reads, params, row_offsets, rows, n_rows, edits, &plan));
    if (plan.items.empty()) return DCN_OK;
    dcn_ctx *c = ctx;
    hipStream_t st = c->stream;
    int prof_slot = -1;
    DCN_TRY(dcn_verify_enqueue(c, map, bases, offsets, n_reads, plan, &prof_slot));
    DCN_PROF_MARK(DCN_STAGE_FINISH);
    DCN_TRY(finish_run(c, prof_slot));
    DCN_HIP(hipMemcpy(edits, c->d_vfy_out, n_rows * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return DCN_OK;
}

// align_api.hip -- dcn_align_batch: the rows of dcn_verify_batch, each verified one with its alignment (kernels in
// align.hip, the trace and the walk back in dcn_align.h, the checks and the first pass in verify_api.hip), and
// dcn_left_align_batch: the same call with the left-align kernel (left_align.hip, dcn_left_align.h) in front of the scan.  Its rules
// over the rows (dcn_align_check_rows), its passes up to the scan of the run counts (dcn_align_runs) and its gather
// (dcn_align_gather_runs) are functions of their own: dcn_pileup_batch (pileup_api.hip) runs the same sequence.
#include "dcn_align.h"
#include "dcn_ctx.h"
#include "dcn_dump_sweep.h"
#include "dcn_left_align.h"
#include "dcn_verify.h"

#include <cstdlib>
#include <cstring>

using namespace dcn_impl;

namespace {
constexpr uint64_t DCN_ALIGN_TRACE_DEFAULT = 1ull << 30; // a convention, not a measured optimum

// bytes of trace a group of rows may take: DCN_ALIGN_TRACE_BYTES, read at call time
uint64_t trace_budget_words() {
    const char *s = std::getenv("DCN_ALIGN_TRACE_BYTES");
    const uint64_t bytes = s && *s ? std::strtoull(s, nullptr, 10) : DCN_ALIGN_TRACE_DEFAULT;
    return bytes / sizeof(uint32_t);
}
} // namespace

int dcn_align_check_rows(const dcn_verify_plan &plan) {
    const uint64_t n_rows = plan.items.size();
    if (n_rows > UINT32_MAX) return dcn_fail(DCN_ERR_ARG, "n_rows must be below 2^32 (the runs of a call are counted per row in 32 bits)");
    for (uint64_t row = 0; row < n_rows; ++row) {
        const dcn_verify_item &it = plan.items[row];
        if (!(it.flags & 2u) && std::max(it.m, it.n) >= (1u << 28))
            return dcn_fail(DCN_ERR_ARG, "row " + std::to_string(row) + ": an interval of 2^28 bases or more has no run length (len << 4 | op)");
    }
    return DCN_OK;
}

int dcn_align_runs(dcn_ctx *c, const dcn_index *map, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                   const dcn_verify_plan &plan, uint32_t *edits, int *prof_slot_out, uint64_t *n_work_out, dcn_la_totals *left) {
    const uint64_t n_rows = plan.items.size();
    hipStream_t st = c->stream;
    int prof_slot = -1;
    *prof_slot_out = -1;
    // pass 1: every row's d (verify_kernel, as dcn_verify_batch runs it)
    DCN_TRY(dcn_verify_enqueue(c, map, bases, offsets, n_reads, plan, &prof_slot));
    *prof_slot_out = prof_slot;
    DCN_HIP(hipStreamSynchronize(st));
    DCN_HIP(hipMemcpy(edits, c->d_vfy_out, n_rows * sizeof(uint32_t), hipMemcpyDeviceToHost));

    // the aligned rows in row order, with the sums of their trace sizes and op bounds
    std::vector<dcn_align_work> work;
    uint64_t trace_words = 0, slot_words = 0, largest = 0;
    uint32_t d_max = 0;
    for (uint64_t row = 0; row < n_rows; ++row) {
        const uint32_t d = edits[row];
        if (d >= DCN_VERIFY_OVER) continue;
        dcn_align_work wk;
        wk.trace_base = trace_words;
        trace_words += dcn_aln_trace_words(d);
        slot_words += dcn_aln_ops_bound(d);
        wk.slot_end = slot_words;
        wk.row = (uint32_t)row;
        wk.d = d;
        work.push_back(wk);
        largest = std::max<uint64_t>(largest, dcn_aln_trace_words(d));
        d_max = std::max(d_max, d);
    }
    const uint64_t n_work = work.size();
    const uint64_t budget = trace_budget_words();

    DCN_TRY(grow(&c->d_aln_n_ops, &c->aln_rows_cap, n_rows + 1, "align run counts"));
    if (!c->d_aln_offsets || c->aln_offsets_cap < n_rows + 1) {
        DCN_TRY(grow(&c->d_aln_offsets, &c->aln_offsets_cap, n_rows + 1, "align run offsets"));
        if (c->d_aln_block_sums) hipFree(c->d_aln_block_sums);
        c->d_aln_block_sums = nullptr;
        DCN_TRY(dev_alloc(&c->d_aln_block_sums, n_rows / DCN_SCAN_BLOCK + 2, "align scan sums"));
    }
    DCN_TRY(grow(&c->d_aln_work, &c->aln_work_cap, n_work, "align rows"));
    DCN_TRY(grow(&c->d_aln_slots, &c->aln_slots_cap, slot_words, "align run slots"));
    DCN_TRY(grow(&c->d_aln_trace, &c->aln_trace_cap, std::max(std::min(budget, trace_words), largest), "align trace"));
    DCN_HIP(hipMemsetAsync(c->d_aln_n_ops, 0, n_rows * sizeof(uint32_t), st));
    DCN_TRY(staged_h2d(c, c->d_aln_work, work.data(), n_work * sizeof(dcn_align_work)));
    DCN_TRY(stage_done(c)); // (the copy stream's copies are in front of the kernels on the context's stream)

    // pass 2, in groups of rows whose traces fit the buffer: in row order, a group closes when the next row would pass
    // the budget, and holds at least one row
    const dcn_base_store *store = map->store;
    dcn_align_args aa;
    memset(&aa, 0, sizeof(aa));
    aa.items = c->d_vfy_items;
    aa.work = c->d_aln_work;
    aa.s_packed = c->d_packed + DCN_FRONT_PAD;
    aa.s_invmask = c->d_invmask + DCN_FRONT_PAD;
    aa.t_packed = store->d_packed;
    aa.t_invmask = store->d_invmask;
    aa.lds_stride = (2 * d_max + 1 + 3) / 4 * 4;
    aa.trace = c->d_aln_trace;
    aa.slots = c->d_aln_slots;
    aa.n_ops = c->d_aln_n_ops;
    for (uint64_t w0 = 0; w0 < n_work;) {
        uint64_t w1 = w0 + 1, words = dcn_aln_trace_words(work[w0].d);
        while (w1 < n_work && words + dcn_aln_trace_words(work[w1].d) <= budget) words += dcn_aln_trace_words(work[w1++].d);
        aa.w0 = w0;
        aa.w1 = w1;
        aa.trace_origin = work[w0].trace_base;
        DCN_TRY(dcn_launch_align(aa, st)); // (one stream: a group's kernel has read its trace before the next one writes)
        w0 = w1;
    }
    if (left) { // rules N1 - N5 on the runs in their slots: the scan and everything behind it see the result
        DCN_TRY(grow(&c->d_aln_scratch, &c->aln_scratch_cap, slot_words, "left-align scratch"));
        if (!c->d_aln_la_totals) DCN_TRY(dev_alloc(&c->d_aln_la_totals, 4, "left-align totals"));
        DCN_HIP(hipMemsetAsync(c->d_aln_la_totals, 0, 4 * sizeof(unsigned long long), st));
        dcn_left_align_args la;
        memset(&la, 0, sizeof(la));
        la.items = aa.items;
        la.work = aa.work;
        la.n_work = n_work;
        la.s_packed = aa.s_packed;
        la.s_invmask = aa.s_invmask;
        la.t_packed = aa.t_packed;
        la.t_invmask = aa.t_invmask;
        la.slots = c->d_aln_slots;
        la.scratch = c->d_aln_scratch;
        la.n_ops = c->d_aln_n_ops;
        la.totals = c->d_aln_la_totals;
        DCN_TRY(dcn_launch_left_align(la, st));
    }
    DCN_TRY(dcn_launch_offsets_scan(c->d_aln_n_ops, (uint32_t)n_rows, c->d_aln_block_sums, c->d_aln_offsets, st));
    DCN_HIP(hipStreamSynchronize(st));
    if (left) DCN_HIP(hipMemcpy(left, c->d_aln_la_totals, sizeof(*left), hipMemcpyDeviceToHost));
    *n_work_out = n_work;
    return DCN_OK;
}

int dcn_align_gather_runs(dcn_ctx *c, uint64_t n_work, uint64_t total) {
    DCN_TRY(grow(&c->d_aln_cigar, &c->aln_cigar_cap, total, "align runs"));
    dcn_align_gather_args ga;
    memset(&ga, 0, sizeof(ga));
    ga.work = c->d_aln_work;
    ga.n_work = n_work;
    ga.slots = c->d_aln_slots;
    ga.n_ops = c->d_aln_n_ops;
    ga.cigar_offsets = c->d_aln_offsets;
    ga.cigar = c->d_aln_cigar;
    return dcn_launch_align_gather(ga, c->stream);
}

namespace {
// dcn_align_batch, and with `left` dcn_left_align_batch: the same checks, order and messages
int align_batch(dcn_ctx *ctx, const dcn_index *map, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads, const void *params,
                const uint64_t *row_offsets, const void *rows, uint64_t n_rows, uint32_t *edits, uint64_t *cigar_offsets, uint32_t *cigar,
                uint64_t capacity, dcn_la_totals *left, uint64_t *n_aligned) {
    dcn_verify_plan plan;
    DCN_TRY(dcn_verify_walk(ctx, map, bases, offsets, n_reads, params, row_offsets, rows, n_rows, edits, &plan));
    if (!cigar_offsets) return dcn_fail(DCN_ERR_ARG, "cigar_offsets is NULL");
    if (plan.items.empty()) {
        cigar_offsets[0] = 0;
        return DCN_OK;
    }
    DCN_TRY(dcn_align_check_rows(plan));
    dcn_ctx *c = ctx;
    hipStream_t st = c->stream;
    int prof_slot = -1;
    uint64_t n_work = 0;
    DCN_TRY(dcn_align_runs(c, map, bases, offsets, n_reads, plan, edits, &prof_slot, &n_work, left));
    *n_aligned = n_work;
    DCN_HIP(hipMemcpy(cigar_offsets, c->d_aln_offsets, (n_rows + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    const uint64_t total = cigar_offsets[n_rows];
    const bool fits = total <= capacity;
    if (fits && total > 0 && !cigar) {
        DCN_PROF_MARK(DCN_STAGE_FINISH);
        DCN_TRY(finish_run(c, prof_slot));
        return dcn_fail(DCN_ERR_ARG, "cigar is NULL");
    }
    if (fits && total > 0) DCN_TRY(dcn_align_gather_runs(c, n_work, total));
    DCN_PROF_MARK(DCN_STAGE_FINISH);
    DCN_TRY(finish_run(c, prof_slot));
    if (!fits)
        return dcn_fail(DCN_ERR_CAPACITY, "cigar holds " + std::to_string(capacity) + " runs, the rows have " + std::to_string(total) +
                                              " (cigar_offsets is complete: call again with that capacity)");
    if (total > 0) DCN_HIP(hipMemcpy(cigar, c->d_aln_cigar, total * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return DCN_OK;
}
} // namespace

extern "C" int dcn_align_batch(dcn_ctx *ctx, const dcn_index *map, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                               const void *params, const uint64_t *row_offsets, const void *rows, uint64_t n_rows, uint32_t *edits,
                               uint64_t *cigar_offsets, uint32_t *cigar, uint64_t capacity) {
    uint64_t n_aligned = 0;
    return align_batch(ctx, map, bases, offsets, n_reads, params, row_offsets, rows, n_rows, edits, cigar_offsets, cigar, capacity, nullptr,
                       &n_aligned);
}

static_assert(sizeof(dcn_left_align_info) == 40 && sizeof(dcn_la_totals) == 32, "left-align info is ABI");

extern "C" int dcn_left_align_batch(dcn_ctx *ctx, const dcn_index *map, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                                    const void *params, const uint64_t *row_offsets, const void *rows, uint64_t n_rows, uint32_t *edits,
                                    uint64_t *cigar_offsets, uint32_t *cigar, uint64_t capacity, void *info_out) {
    dcn_left_align_info *const info = static_cast<dcn_left_align_info *>(info_out);
    dcn_la_totals t = {0, 0, 0, 0};
    uint64_t n_aligned = 0;
    if (info) memset(info, 0, sizeof(*info));
    const int rc = align_batch(ctx, map, bases, offsets, n_reads, params, row_offsets, rows, n_rows, edits, cigar_offsets, cigar, capacity, &t,
                               &n_aligned);
    // (complete whenever cigar_offsets is: DCN_ERR_CAPACITY included)
    if (info) *info = {n_aligned, t.rows_changed, t.gaps_shifted, t.columns_passed, t.gaps_merged};
    return rc;
}

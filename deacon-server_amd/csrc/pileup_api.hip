// pileup_api.hip -- the C ABI of pileups (dcn_anchor_map_pileup_enable / _reset / _fetch / _call, dcn_pileup_batch, and with
// base qualities dcn_anchor_map_pileup_keep_qualities / _fetch_qualities, dcn_pileup_batch_qual; the strand planes of rule S1,
// dcn_anchor_map_pileup_keep_strands / _fetch_strands;
// kernels in pileup.hip, the shared arithmetic in dcn_pileup.h; a kept insertion ledger, insertions_api.hip, and a kept
// deletion ledger, indels_api.hip, are appended to, emptied and freed here).  dcn_pileup_batch is dcn_align_batch's sequence
// (verify_api.hip's walk, align_api.hip's passes and gather) with the runs left on the device and the pileup kernel behind;
// dcn_pileup_batch_qual is the same sequence with the qualities staged in front of the kernel's quality form.
#include "dcn_ctx.h"
#include "dcn_dump_sweep.h"
#include "dcn_left_align.h"
#include "dcn_pileup.h"
#include "dcn_verify.h"

#include <cstring>

using namespace dcn_impl;

static_assert(sizeof(dcn_pileup_call_params) == 16, "pileup call params are ABI");
static_assert(sizeof(dcn_pileup_qual_params) == 16, "pileup quality params are ABI");
static_assert(DCN_PILEUP_A == DCN_PILE_A && DCN_PILEUP_C == DCN_PILE_C && DCN_PILEUP_G == DCN_PILE_G && DCN_PILEUP_T == DCN_PILE_T &&
                  DCN_PILEUP_N == DCN_PILE_N && DCN_PILEUP_DEL == DCN_PILE_DEL && DCN_PILEUP_INS == DCN_PILE_INS &&
                  DCN_PILEUP_REV == DCN_PILE_REV && DCN_PILEUP_COLUMNS == DCN_PILE_COLUMNS,
              "the columns of the header and of dcn_pileup.h");
static_assert(DCN_PILEUP_SITE_SUB == DCN_PILE_SITE_SUB && DCN_PILEUP_SITE_DEL == DCN_PILE_SITE_DEL &&
                  DCN_PILEUP_SITE_INS == DCN_PILE_SITE_INS && DCN_PILEUP_NO_CODE == DCN_PILE_NO_CODE,
              "the site flags of the header and of dcn_pileup.h");

// (declared in dcn_verify.h, the scratch holder in dcn_ctx.h: genotype_api.hip makes the same checks)
int dcn_pile_api::check_pileup(const dcn_index *map) {
    DCN_TRY(check_store(map));
    if (!map->d_pileup) return dcn_fail(DCN_ERR_ARG, "the map has no pileup (dcn_anchor_map_pileup_enable)");
    return DCN_OK;
}

int dcn_pile_api::check_qsums(const dcn_index *map) {
    DCN_TRY(check_pileup(map));
    if (!map->d_pileup_qsums) return dcn_fail(DCN_ERR_ARG, "the map keeps no quality sums (dcn_anchor_map_pileup_keep_qualities)");
    return DCN_OK;
}

int dcn_pile_api::check_strands(const dcn_index *map) {
    DCN_TRY(check_pileup(map));
    if (!map->d_pileup_strands) return dcn_fail(DCN_ERR_ARG, "the map keeps no strand planes (dcn_anchor_map_pileup_keep_strands)");
    return DCN_OK;
}

using namespace dcn_pile_api;

extern "C" int dcn_anchor_map_pileup_enable(dcn_index *map, int enable) {
    DCN_TRY(check_store(map));
    if (!enable) {
        if (map->d_pileup) {
            DCN_HIP(hipSetDevice(map->device));
            hipFree(map->d_pileup);
            dcn_ins_ledger_free(map->ledger);
            dcn_del_ledger_free(map->del_ledger);
            if (map->d_pileup_qsums) hipFree(map->d_pileup_qsums);
            if (map->d_pileup_strands) hipFree(map->d_pileup_strands);
        }
        map->d_pileup = nullptr;
        map->d_pileup_qsums = nullptr;
        map->d_pileup_strands = nullptr;
        map->pileup_bases = 0;
        map->pileup_rows = 0;
        map->ledger = nullptr;
        map->del_ledger = nullptr;
        map->pileup_left_align = false;
        memset(map->left_align_info, 0, sizeof(map->left_align_info));
        return DCN_OK;
    }
    if (map->d_pileup) return DCN_OK;
    DCN_HIP(hipSetDevice(map->device));
    const uint64_t bases = std::max<uint64_t>(map->store->used, 32); // (whole 32-base groups, as the store counts them)
    DCN_TRY(dev_alloc_zeroed(&map->d_pileup, bases * DCN_PILE_COLUMNS, "pileup counters"));
    map->pileup_bases = bases;
    map->pileup_rows = 0;
    return DCN_OK;
}

extern "C" int dcn_anchor_map_pileup_reset(dcn_index *map) {
    DCN_TRY(check_pileup(map));
    DCN_HIP(hipSetDevice(map->device));
    DCN_HIP(hipMemset(map->d_pileup, 0, map->pileup_bases * DCN_PILE_COLUMNS * sizeof(uint32_t)));
    if (map->d_pileup_qsums) DCN_HIP(hipMemset(map->d_pileup_qsums, 0, map->pileup_bases * DCN_PILE_SUM_COLUMNS * sizeof(uint32_t)));
    if (map->d_pileup_strands)
        DCN_HIP(hipMemset(map->d_pileup_strands, 0, map->pileup_bases * DCN_PILE_STRAND_COLUMNS * sizeof(uint32_t)));
    DCN_HIP(hipDeviceSynchronize()); // (null-stream work must not be overtaken by a context's stream)
    map->pileup_rows = 0;
    if (map->ledger) map->ledger->n_events = map->ledger->n_bases = 0; // (the arrays stay: the next append begins at their start)
    if (map->del_ledger) map->del_ledger->n_events = map->del_ledger->n_deleted = 0;
    memset(map->left_align_info, 0, sizeof(map->left_align_info));
    return DCN_OK;
}

extern "C" int dcn_anchor_map_pileup_left_align(dcn_index *map, int on) {
    DCN_TRY(check_pileup(map));
    if ((on != 0) == map->pileup_left_align) return DCN_OK;
    if (map->pileup_rows != 0) // rule N8
        return dcn_fail(DCN_ERR_ARG, std::to_string(map->pileup_rows) + " rows have added to the pileup since it was enabled or reset: every row of "
                                                                         "a pileup is piled up the same way (dcn_anchor_map_pileup_reset first)");
    map->pileup_left_align = on != 0;
    return DCN_OK;
}

extern "C" int dcn_anchor_map_pileup_left_align_info(const dcn_index *map, void *info) {
    DCN_TRY(check_pileup(map));
    if (!info) return dcn_fail(DCN_ERR_ARG, "info is NULL");
    memcpy(info, map->left_align_info, sizeof(dcn_left_align_info));
    return DCN_OK;
}

extern "C" int dcn_anchor_map_pileup_keep_qualities(dcn_index *map, int keep) {
    DCN_TRY(check_pileup(map));
    if (!keep) {
        if (map->d_pileup_qsums) {
            DCN_HIP(hipSetDevice(map->device));
            hipFree(map->d_pileup_qsums);
        }
        map->d_pileup_qsums = nullptr;
        return DCN_OK;
    }
    if (map->d_pileup_qsums) return DCN_OK;
    if (map->pileup_rows != 0) // rule Q1
        return dcn_fail(DCN_ERR_ARG, std::to_string(map->pileup_rows) + " rows have added to the pileup since it was enabled or reset: the sums "
                                                                         "begin with the counters (dcn_anchor_map_pileup_reset first)");
    DCN_HIP(hipSetDevice(map->device));
    return dev_alloc_zeroed(&map->d_pileup_qsums, map->pileup_bases * DCN_PILE_SUM_COLUMNS, "pileup quality sums");
}

extern "C" int dcn_anchor_map_pileup_keep_strands(dcn_index *map, int keep) {
    DCN_TRY(check_pileup(map));
    if (!keep) {
        if (map->d_pileup_strands) {
            DCN_HIP(hipSetDevice(map->device));
            hipFree(map->d_pileup_strands);
        }
        map->d_pileup_strands = nullptr;
        return DCN_OK;
    }
    if (map->d_pileup_strands) return DCN_OK;
    if (map->pileup_rows != 0) // rule S1
        return dcn_fail(DCN_ERR_ARG, std::to_string(map->pileup_rows) + " rows have added to the pileup since it was enabled or reset: the strand "
                                                                         "planes begin with the counters (dcn_anchor_map_pileup_reset first)");
    DCN_HIP(hipSetDevice(map->device));
    return dev_alloc_zeroed(&map->d_pileup_strands, map->pileup_bases * DCN_PILE_STRAND_COLUMNS, "pileup strand planes");
}

namespace {
// What dcn_pileup_batch and dcn_pileup_batch_qual run behind their checks.  qprm = null: the plain call.
int pileup_run(dcn_ctx *c, dcn_index *map, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint32_t n_reads,
               const dcn_verify_plan &plan, const dcn_pileup_qual_params *qprm, uint32_t *edits, uint64_t *n_added) {
    const uint64_t n_rows = plan.items.size();
    hipStream_t st = c->stream;
    int prof_slot = -1;
    uint64_t n_work = 0, total = 0;
    dcn_la_totals left = {0, 0, 0, 0}; // rule N8: the runs that are piled up are N5's while the map's switch is on
    DCN_TRY(dcn_align_runs(c, map, bases, offsets, n_reads, plan, edits, &prof_slot, &n_work, map->pileup_left_align ? &left : nullptr));
    DCN_HIP(hipMemcpy(&total, c->d_aln_offsets + n_rows, sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (total > 0) { // the runs stay on the device: the buffer grows to what the scan reports
        DCN_TRY(dcn_align_gather_runs(c, n_work, total));
        dcn_pileup_args pa;
        memset(&pa, 0, sizeof(pa));
        pa.items = c->d_vfy_items;
        pa.work = c->d_aln_work;
        pa.n_work = n_work;
        pa.s_packed = c->d_packed + DCN_FRONT_PAD;
        pa.s_invmask = c->d_invmask + DCN_FRONT_PAD;
        pa.n_ops = c->d_aln_n_ops;
        pa.cigar_offsets = c->d_aln_offsets;
        pa.cigar = c->d_aln_cigar;
        pa.counters = map->d_pileup;
        pa.bases = map->pileup_bases;
        if (qprm) { // the qualities, a byte per base, in front of the kernel on the context's stream
            DCN_TRY(grow(&c->d_pile_quals, &c->pile_quals_cap, plan.n_bases, "pileup qualities"));
            DCN_TRY(staged_h2d(c, c->d_pile_quals, quals, plan.n_bases));
            DCN_TRY(stage_done(c));
            dcn_pileup_qual_args qa;
            memset(&qa, 0, sizeof(qa));
            qa.rows = pa;
            qa.quals = c->d_pile_quals;
            qa.sums = map->d_pileup_qsums;
            qa.qual_offset = qprm->qual_offset;
            qa.min_base_qual = qprm->min_base_qual;
            if (map->d_pileup_strands) DCN_TRY(dcn_launch_pileup_qual_strand(qa, map->d_pileup_strands, st)); // rule S2
            else DCN_TRY(dcn_launch_pileup_qual(qa, st));
        } else if (map->d_pileup_strands) {
            DCN_TRY(dcn_launch_pileup_strand(pa, map->d_pileup_strands, st));
        } else {
            DCN_TRY(dcn_launch_pileup(pa, st));
        }
        if (map->ledger) DCN_TRY(dcn_insertions_append(c, map, pa)); // rule L2, behind the same checks
        if (map->del_ledger) DCN_TRY(dcn_deletions_append(c, map, pa)); // rule R2, likewise
    }
    DCN_PROF_MARK(DCN_STAGE_FINISH);
    DCN_TRY(finish_run(c, prof_slot));
    uint64_t added = 0; // rule P2: the rows with an alignment and n > 0
    for (uint64_t row = 0; row < n_rows; ++row) added += edits[row] < DCN_VERIFY_OVER && plan.items[row].n > 0;
    map->pileup_rows += added; // (rules L1, Q1 and N8 ask)
    if (map->pileup_left_align) {
        map->left_align_info[0] += n_work;
        map->left_align_info[1] += left.rows_changed;
        map->left_align_info[2] += left.gaps_shifted;
        map->left_align_info[3] += left.columns_passed;
        map->left_align_info[4] += left.gaps_merged;
    }
    if (n_added) *n_added = added;
    return DCN_OK;
}
} // namespace

extern "C" int dcn_pileup_batch(dcn_ctx *ctx, dcn_index *map, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                                const void *params, const uint64_t *row_offsets, const void *rows, uint64_t n_rows, uint32_t *edits,
                                uint64_t *n_added) {
    dcn_verify_plan plan;
    DCN_TRY(dcn_verify_walk(ctx, map, bases, offsets, n_reads, params, row_offsets, rows, n_rows, edits, &plan));
    if (!map->d_pileup) return dcn_fail(DCN_ERR_ARG, "the map has no pileup (dcn_anchor_map_pileup_enable)");
    if (map->d_pileup_qsums) // rule Q1: sums and counters describe the same rows
        return dcn_fail(DCN_ERR_ARG, "the map keeps quality sums, and these rows have no qualities: dcn_pileup_batch_qual adds to it "
                                     "(or dcn_anchor_map_pileup_keep_qualities(map, 0) first)");
    if (n_added) *n_added = 0;
    if (plan.items.empty()) return DCN_OK;
    DCN_TRY(dcn_align_check_rows(plan));
    return pileup_run(ctx, map, bases, nullptr, offsets, n_reads, plan, nullptr, edits, n_added);
}

extern "C" int dcn_pileup_batch_qual(dcn_ctx *ctx, dcn_index *map, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets,
                                     uint32_t n_reads, const void *params, const void *qual_params, const uint64_t *row_offsets,
                                     const void *rows, uint64_t n_rows, uint32_t *edits, uint64_t *n_added) {
    dcn_verify_plan plan;
    DCN_TRY(dcn_verify_walk(ctx, map, bases, offsets, n_reads, params, row_offsets, rows, n_rows, edits, &plan));
    if (!map->d_pileup) return dcn_fail(DCN_ERR_ARG, "the map has no pileup (dcn_anchor_map_pileup_enable)");
    if (!plan.items.empty()) DCN_TRY(dcn_align_check_rows(plan));
    // (dcn_pileup_batch's checks end here)
    const dcn_pileup_qual_params *qprm = static_cast<const dcn_pileup_qual_params *>(qual_params);
    if (!qprm) return dcn_fail(DCN_ERR_ARG, "qual_params is NULL");
    if (qprm->reserved[0] != 0 || qprm->reserved[1] != 0) return dcn_fail(DCN_ERR_ARG, "qual_params.reserved must be 0");
    if (qprm->qual_offset > 255) return dcn_fail(DCN_ERR_ARG, "qual_params.qual_offset must be 0..255");
    if (qprm->min_base_qual > 255) return dcn_fail(DCN_ERR_ARG, "qual_params.min_base_qual must be 0..255");
    if (!plan.items.empty() && plan.n_bases > 0 && !quals) return dcn_fail(DCN_ERR_ARG, "quals is NULL");
    if (n_added) *n_added = 0;
    if (plan.items.empty()) return DCN_OK;
    return pileup_run(ctx, map, bases, quals, offsets, n_reads, plan, qprm, edits, n_added);
}

extern "C" int dcn_anchor_map_pileup_fetch(const dcn_index *map, uint32_t record, uint64_t start, uint64_t n_bases, uint32_t *counts) {
    DCN_TRY(check_pileup(map));
    uint64_t b0 = 0;
    DCN_TRY(check_range(map, "pileup fetch", record, start, n_bases, &b0));
    if (n_bases == 0) return DCN_OK;
    if (!counts) return dcn_fail(DCN_ERR_ARG, "counts is NULL");
    DCN_HIP(hipSetDevice(map->device));
#if defined(DCN_PILEUP_POSITION_MAJOR)
    DCN_HIP(hipMemcpy(counts, map->d_pileup + b0 * DCN_PILE_COLUMNS, n_bases * DCN_PILE_COLUMNS * sizeof(uint32_t), hipMemcpyDeviceToHost));
#else
    std::vector<uint32_t> plane(n_bases); // column-major on the device: a plane at a time, transposed here
    for (uint32_t col = 0; col < DCN_PILE_COLUMNS; ++col) {
        DCN_HIP(hipMemcpy(plane.data(), map->d_pileup + dcn_pile_index(col, b0, map->pileup_bases), n_bases * sizeof(uint32_t),
                          hipMemcpyDeviceToHost));
        for (uint64_t q = 0; q < n_bases; ++q) counts[q * DCN_PILE_COLUMNS + col] = plane[q];
    }
#endif
    return DCN_OK;
}

extern "C" int dcn_anchor_map_pileup_fetch_qualities(const dcn_index *map, uint32_t record, uint64_t start, uint64_t n_bases, uint32_t *sums) {
    DCN_TRY(check_qsums(map));
    uint64_t b0 = 0;
    DCN_TRY(check_range(map, "pileup fetch", record, start, n_bases, &b0));
    if (n_bases == 0) return DCN_OK;
    if (!sums) return dcn_fail(DCN_ERR_ARG, "sums is NULL");
    DCN_HIP(hipSetDevice(map->device));
#if defined(DCN_PILEUP_POSITION_MAJOR)
    DCN_HIP(hipMemcpy(sums, map->d_pileup_qsums + b0 * DCN_PILE_SUM_COLUMNS, n_bases * DCN_PILE_SUM_COLUMNS * sizeof(uint32_t), hipMemcpyDeviceToHost));
#else
    std::vector<uint32_t> plane(n_bases); // (as dcn_anchor_map_pileup_fetch: a plane at a time, transposed here)
    for (uint32_t col = 0; col < DCN_PILE_SUM_COLUMNS; ++col) {
        DCN_HIP(hipMemcpy(plane.data(), map->d_pileup_qsums + dcn_pile_sum_index(col, b0, map->pileup_bases), n_bases * sizeof(uint32_t),
                          hipMemcpyDeviceToHost));
        for (uint64_t q = 0; q < n_bases; ++q) sums[q * DCN_PILE_SUM_COLUMNS + col] = plane[q];
    }
#endif
    return DCN_OK;
}

extern "C" int dcn_anchor_map_pileup_fetch_strands(const dcn_index *map, uint32_t record, uint64_t start, uint64_t n_bases, uint32_t *rev) {
    DCN_TRY(check_strands(map));
    uint64_t b0 = 0;
    DCN_TRY(check_range(map, "pileup fetch", record, start, n_bases, &b0));
    if (n_bases == 0) return DCN_OK;
    if (!rev) return dcn_fail(DCN_ERR_ARG, "rev is NULL");
    DCN_HIP(hipSetDevice(map->device));
#if defined(DCN_PILEUP_POSITION_MAJOR)
    DCN_HIP(hipMemcpy(rev, map->d_pileup_strands + b0 * DCN_PILE_STRAND_COLUMNS, n_bases * DCN_PILE_STRAND_COLUMNS * sizeof(uint32_t),
                      hipMemcpyDeviceToHost));
#else
    std::vector<uint32_t> plane(n_bases); // (as dcn_anchor_map_pileup_fetch: a plane at a time, transposed here)
    for (uint32_t col = 0; col < DCN_PILE_STRAND_COLUMNS; ++col) {
        DCN_HIP(hipMemcpy(plane.data(), map->d_pileup_strands + dcn_pile_strand_index(col, b0, map->pileup_bases), n_bases * sizeof(uint32_t),
                          hipMemcpyDeviceToHost));
        for (uint64_t q = 0; q < n_bases; ++q) rev[q * DCN_PILE_STRAND_COLUMNS + col] = plane[q];
    }
#endif
    return DCN_OK;
}

extern "C" int dcn_anchor_map_pileup_call(const dcn_index *map, const void *params, uint32_t record, uint64_t start, uint64_t n_bases,
                                          uint8_t *calls, uint64_t *site_pos, uint32_t *site_info, uint64_t capacity, uint64_t *n_sites) {
    const dcn_pileup_call_params *prm = static_cast<const dcn_pileup_call_params *>(params);
    if (!prm) return dcn_fail(DCN_ERR_ARG, "params is NULL");
    if (prm->reserved[0] != 0 || prm->reserved[1] != 0) return dcn_fail(DCN_ERR_ARG, "params.reserved must be 0");
    if (prm->min_permille > 1000) return dcn_fail(DCN_ERR_ARG, "params.min_permille must be 0..1000");
    DCN_TRY(check_pileup(map));
    uint64_t b0 = 0;
    DCN_TRY(check_range(map, "pileup call", record, start, n_bases, &b0));
    if (!n_sites) return dcn_fail(DCN_ERR_ARG, "n_sites is NULL");
    *n_sites = 0;
    if (n_bases == 0) return DCN_OK;
    DCN_HIP(hipSetDevice(map->device));

    const uint32_t blocks = dcn_pileup_call_blocks(n_bases);
    scratch mem;
    dcn_pileup_call_args ca;
    memset(&ca, 0, sizeof(ca));
    uint32_t *d_counts = nullptr;
    uint64_t *d_offsets = nullptr;
    unsigned long long *d_sums = nullptr;
    DCN_TRY(mem.get(&ca.calls, n_bases, "pileup calls"));
    DCN_TRY(mem.get(&d_counts, blocks, "pileup site counts"));
    DCN_TRY(mem.get(&d_offsets, (uint64_t)blocks + 1, "pileup site offsets"));
    DCN_TRY(mem.get(&d_sums, blocks / DCN_SCAN_BLOCK + 2, "pileup scan sums"));
    ca.counters = map->d_pileup;
    ca.bases = map->pileup_bases;
    ca.t_packed = map->store->d_packed;
    ca.t_invmask = map->store->d_invmask;
    ca.base0 = b0;
    ca.n = n_bases;
    ca.pos0 = start;
    ca.min_depth = prm->min_depth;
    ca.min_permille = prm->min_permille;
    ca.block_counts = d_counts;
    ca.block_offsets = d_offsets;
    // count, scan, gather: the shape of dcn_locate_batch and dcn_align_batch (the null stream: a map has none of its own)
    DCN_TRY(dcn_launch_pileup_call(ca, false, nullptr));
    DCN_TRY(dcn_launch_offsets_scan(d_counts, blocks, d_sums, d_offsets, nullptr));
    uint64_t total = 0;
    DCN_HIP(hipMemcpy(&total, d_offsets + blocks, sizeof(uint64_t), hipMemcpyDeviceToHost));
    *n_sites = total;
    if (calls) DCN_HIP(hipMemcpy(calls, ca.calls, n_bases, hipMemcpyDeviceToHost));
    if (total > capacity)
        return dcn_fail(DCN_ERR_CAPACITY, "the sites hold " + std::to_string(capacity) + " entries, the range has " + std::to_string(total) +
                                              " (n_sites and calls are complete: call again with that capacity)");
    if (total == 0) return DCN_OK;
    if (!site_pos || !site_info) return dcn_fail(DCN_ERR_ARG, "site_pos/site_info is NULL");
    DCN_TRY(mem.get(&ca.site_pos, total, "pileup site positions"));
    DCN_TRY(mem.get(&ca.site_info, total, "pileup site info"));
    DCN_TRY(dcn_launch_pileup_call(ca, true, nullptr));
    DCN_HIP(hipMemcpy(site_pos, ca.site_pos, total * sizeof(uint64_t), hipMemcpyDeviceToHost));
    DCN_HIP(hipMemcpy(site_info, ca.site_info, total * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return DCN_OK;
}

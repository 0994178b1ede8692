// phase_api.hip -- the C ABI of phasing (dcn_anchor_map_phase_sites / _info / _links / _solve, dcn_phase_batch of
// include/deacon_hip_phase.h; kernels in phase.hip, the rule in dcn_phase.h).  dcn_phase_batch is dcn_pileup_batch_qual's
// sequence (verify_api.hip's walk, align_api.hip's passes and gather, pileup_api.hip's staging of the qualities) with the
// link kernel in the pileup kernel's place: nothing of a pileup is read or written.  The range calls are blocking, on the
// null stream with scratch of the call, like dcn_anchor_map_genotype (genotype_api.hip), whose scratch holder they share.
#include "../../include/deacon_hip_phase.h"
#include "dcn_ctx.h"
#include "dcn_dump_sweep.h"
#include "dcn_left_align.h"
#include "dcn_phase.h"
#include "dcn_pileup.h"
#include "dcn_verify.h"

#include <cstring>
#include <string>
#include <vector>

using namespace dcn_impl;
using namespace dcn_pile_api;

static_assert(sizeof(dcn_phase_site) == 16 && sizeof(dcn_phase_params) == 16 && sizeof(dcn_phase_result) == 32, "phase structs are ABI");
static_assert(sizeof(dcn_phase_elem) == 16, "scan element");
static_assert(DCN_PHASE_DEC_JOINED != 0 && DCN_PHASE_LINK_BIT > 15, "the alleles' four bits and the link bit");

void dcn_phase_list_free(dcn_phase_list *l) {
    if (!l) return;
    if (l->d_base) hipFree(l->d_base);
    if (l->d_pos) hipFree(l->d_pos);
    if (l->d_alleles) hipFree(l->d_alleles);
    if (l->d_links) hipFree(l->d_links);
    if (l->d_call) hipFree(l->d_call);
    delete l;
}

namespace {
int check_list(const dcn_index *map) {
    DCN_TRY(check_store(map));
    if (!map->phase) return dcn_fail(DCN_ERR_ARG, "the map has no phase sites (dcn_anchor_map_phase_sites)");
    return DCN_OK;
}
} // namespace

extern "C" int dcn_anchor_map_phase_sites(dcn_index *map, const void *sites, uint64_t n_sites) {
    DCN_TRY(check_store(map));
    if (n_sites == 0) {
        if (map->phase) {
            DCN_HIP(hipSetDevice(map->device));
            DCN_HIP(hipDeviceSynchronize());
            dcn_phase_list_free(map->phase);
        }
        map->phase = nullptr;
        return DCN_OK;
    }
    if (!sites) return dcn_fail(DCN_ERR_ARG, "sites is NULL");
    if (n_sites > 0xFFFFFFFEull) return dcn_fail(DCN_ERR_ARG, "a phase site list holds at most 4294967294 sites");
    const dcn_phase_site *in = static_cast<const dcn_phase_site *>(sites);
    const dcn_base_store *store = map->store;
    const uint64_t n_records = store->rec_len.size();
    std::vector<uint64_t> base(n_sites), pos(n_sites);
    std::vector<uint8_t> alleles(n_sites);
    for (uint64_t i = 0; i < n_sites; ++i) {
        const dcn_phase_site &s = in[i];
        const auto bad = [i](const std::string &what) { return dcn_fail(DCN_ERR_ARG, "sites[" + std::to_string(i) + "]: " + what); };
        if (s.reserved[0] != 0 || s.reserved[1] != 0) return bad("reserved must be 0");
        if (s.record >= n_records) return bad("record " + std::to_string(s.record) + " of " + std::to_string(n_records) + " added");
        if (s.pos >= store->rec_len[s.record])
            return bad("pos " + std::to_string(s.pos) + " is outside the record's " + std::to_string(store->rec_len[s.record]) + " bases");
        if (s.a0 > 3 || s.a1 > 3) return bad("a0 and a1 must be 0..3 (A C G T)");
        if (s.a0 == s.a1) return bad("a0 and a1 are the same allele");
        if (i > 0 && (s.record < in[i - 1].record || (s.record == in[i - 1].record && s.pos <= in[i - 1].pos)))
            return bad("does not lie behind the site in front of it (strictly ascending in record, pos)");
        base[i] = store->rec_start[s.record] + s.pos;
        pos[i] = s.pos;
        alleles[i] = (uint8_t)dcn_phase_pack_alleles(s.a0, s.a1);
        // (the link kernel searches the store positions, which ascend with (record, pos) because a store's records begin in
        // the order they were added: checked and not assumed)
        if (i > 0 && base[i] <= base[i - 1])
            return dcn_fail(DCN_ERR_INTERNAL, "sites[" + std::to_string(i) + "]: the base store's records do not begin in ascending order");
        if (i > 0 && s.record == in[i - 1].record) alleles[i - 1] |= (uint8_t)DCN_PHASE_LINK_BIT;
    }
    DCN_HIP(hipSetDevice(map->device));
    DCN_HIP(hipDeviceSynchronize()); // (no context's stream still adds to the list that goes)
    dcn_phase_list *l = new (std::nothrow) dcn_phase_list();
    if (!l) return dcn_fail(DCN_ERR_NOMEM, "host allocation failed");
    int rc = dev_alloc(&l->d_base, n_sites, "phase site bases");
    if (rc == DCN_OK) rc = dev_alloc(&l->d_pos, n_sites, "phase site positions");
    if (rc == DCN_OK) rc = dev_alloc(&l->d_alleles, n_sites, "phase site alleles");
    if (rc == DCN_OK) rc = dev_alloc_zeroed(&l->d_links, n_sites * 4, "phase links");
    if (rc == DCN_OK) rc = dev_alloc_zeroed(&l->d_call, 2, "phase call counters");
    hipError_t e = hipSuccess;
    if (rc == DCN_OK) e = hipMemcpy(l->d_base, base.data(), n_sites * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (rc == DCN_OK && e == hipSuccess) e = hipMemcpy(l->d_pos, pos.data(), n_sites * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (rc == DCN_OK && e == hipSuccess) e = hipMemcpy(l->d_alleles, alleles.data(), n_sites, hipMemcpyHostToDevice);
    if (rc == DCN_OK && e == hipSuccess) e = hipDeviceSynchronize();
    if (rc == DCN_OK && e != hipSuccess) rc = dcn_hip_fail(e, "phase sites");
    if (rc != DCN_OK) {
        dcn_phase_list_free(l);
        return rc;
    }
    l->n = n_sites;
    dcn_phase_list_free(map->phase);
    map->phase = l;
    return DCN_OK;
}

extern "C" int dcn_anchor_map_phase_info(const dcn_index *map, uint64_t info[4]) {
    DCN_TRY(check_store(map));
    if (!info) return dcn_fail(DCN_ERR_ARG, "info is NULL");
    const dcn_phase_list *l = map->phase;
    info[0] = l ? l->n : 0;
    info[1] = l ? l->rows : 0;
    info[2] = l ? l->rows_linking : 0;
    info[3] = l ? l->link_adds : 0;
    return DCN_OK;
}

namespace {
// What dcn_phase_batch runs behind its checks: pileup_run (pileup_api.hip) with the link kernel.  qprm = null: no Q3.
int phase_run(dcn_ctx *c, dcn_index *map, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint32_t n_reads,
              const dcn_verify_plan &plan, const dcn_pileup_qual_params *qprm, uint32_t *edits, uint64_t *n_linking) {
    dcn_phase_list *l = map->phase;
    const uint64_t n_rows = plan.items.size();
    hipStream_t st = c->stream;
    int prof_slot = -1;
    uint64_t n_work = 0, total = 0;
    dcn_la_totals left = {0, 0, 0, 0}; // rule H2: the runs are N5's while the map's switch is on, as for the pileup
    DCN_TRY(dcn_align_runs(c, map, bases, offsets, n_reads, plan, edits, &prof_slot, &n_work, map->pileup_left_align ? &left : nullptr));
    DCN_HIP(hipMemcpy(&total, c->d_aln_offsets + n_rows, sizeof(uint64_t), hipMemcpyDeviceToHost));
    unsigned long long call[2] = {0, 0};
    if (total > 0) {
        DCN_TRY(dcn_align_gather_runs(c, n_work, total));
        dcn_phase_link_args la;
        memset(&la, 0, sizeof(la));
        la.rows.items = c->d_vfy_items;
        la.rows.work = c->d_aln_work;
        la.rows.n_work = n_work;
        la.rows.s_packed = c->d_packed + DCN_FRONT_PAD;
        la.rows.s_invmask = c->d_invmask + DCN_FRONT_PAD;
        la.rows.n_ops = c->d_aln_n_ops;
        la.rows.cigar_offsets = c->d_aln_offsets;
        la.rows.cigar = c->d_aln_cigar;
        la.site_base = l->d_base;
        la.site_alleles = l->d_alleles;
        la.n_sites = l->n;
        la.links = l->d_links;
        la.call = l->d_call;
        if (qprm) { // the qualities, a byte per base, in front of the kernel on the context's stream
            DCN_TRY(grow(&c->d_pile_quals, &c->pile_quals_cap, plan.n_bases, "pileup qualities"));
            DCN_TRY(staged_h2d(c, c->d_pile_quals, quals, plan.n_bases));
            DCN_TRY(stage_done(c));
            la.quals = c->d_pile_quals;
            la.qual_offset = qprm->qual_offset;
            la.min_base_qual = qprm->min_base_qual;
        }
        DCN_HIP(hipMemsetAsync(l->d_call, 0, sizeof(call), st));
        DCN_TRY(dcn_launch_phase_link(la, qprm != nullptr, st));
    }
    DCN_PROF_MARK(DCN_STAGE_FINISH);
    DCN_TRY(finish_run(c, prof_slot));
    if (total > 0) DCN_HIP(hipMemcpy(call, l->d_call, sizeof(call), hipMemcpyDeviceToHost));
    uint64_t counted = 0; // rule P2: the rows with an alignment and n > 0
    for (uint64_t row = 0; row < n_rows; ++row) counted += edits[row] < DCN_VERIFY_OVER && plan.items[row].n > 0;
    l->rows += counted;
    l->rows_linking += call[0];
    l->link_adds += call[1];
    if (n_linking) *n_linking = call[0];
    return DCN_OK;
}
} // namespace

extern "C" int dcn_phase_batch(dcn_ctx *ctx, dcn_index *map, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets,
                               uint32_t n_reads, const void *params, const void *qual_params, const uint64_t *row_offsets, const void *rows,
                               uint64_t n_rows, uint32_t *edits, uint64_t *n_linking) {
    dcn_verify_plan plan;
    DCN_TRY(dcn_verify_walk(ctx, map, bases, offsets, n_reads, params, row_offsets, rows, n_rows, edits, &plan));
    if (!map->phase) return dcn_fail(DCN_ERR_ARG, "the map has no phase sites (dcn_anchor_map_phase_sites)");
    if (!plan.items.empty()) DCN_TRY(dcn_align_check_rows(plan));
    const dcn_pileup_qual_params *qprm = static_cast<const dcn_pileup_qual_params *>(qual_params);
    if (!qprm && quals) return dcn_fail(DCN_ERR_ARG, "qual_params is NULL and quals is not: both or neither");
    if (qprm) {
        if (qprm->reserved[0] != 0 || qprm->reserved[1] != 0) return dcn_fail(DCN_ERR_ARG, "qual_params.reserved must be 0");
        if (qprm->qual_offset > 255) return dcn_fail(DCN_ERR_ARG, "qual_params.qual_offset must be 0..255");
        if (qprm->min_base_qual > 255) return dcn_fail(DCN_ERR_ARG, "qual_params.min_base_qual must be 0..255");
        // (as dcn_pileup_batch_qual: a batch without bases has no quality to point at)
        if (!plan.items.empty() && plan.n_bases > 0 && !quals) return dcn_fail(DCN_ERR_ARG, "quals is NULL and qual_params is not: both or neither");
    }
    if (n_linking) *n_linking = 0;
    if (plan.items.empty()) return DCN_OK;
    return phase_run(ctx, map, bases, quals, offsets, n_reads, plan, qprm, edits, n_linking);
}

extern "C" int dcn_anchor_map_phase_links(const dcn_index *map, uint64_t first, uint64_t n, uint32_t *links) {
    DCN_TRY(check_list(map));
    const dcn_phase_list *l = map->phase;
    if (first > l->n || n > l->n - first)
        return dcn_fail(DCN_ERR_ARG, "phase links: sites [" + std::to_string(first) + ", " + std::to_string(first) + " + " + std::to_string(n) +
                                         ") are past the list's " + std::to_string(l->n));
    if (n == 0) return DCN_OK;
    if (!links) return dcn_fail(DCN_ERR_ARG, "links is NULL");
    DCN_HIP(hipSetDevice(map->device));
    DCN_HIP(hipMemcpy(links, l->d_links + 4 * first, n * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return DCN_OK;
}

extern "C" int dcn_anchor_map_phase_solve(const dcn_index *map, const void *params, void *results) {
    const dcn_phase_params *prm = static_cast<const dcn_phase_params *>(params);
    if (!prm) return dcn_fail(DCN_ERR_ARG, "params is NULL");
    if (prm->reserved[0] != 0 || prm->reserved[1] != 0) return dcn_fail(DCN_ERR_ARG, "params.reserved must be 0");
    if (prm->max_minor_permille > 1000) return dcn_fail(DCN_ERR_ARG, "params.max_minor_permille must be 0..1000");
    DCN_TRY(check_list(map));
    if (!results) return dcn_fail(DCN_ERR_ARG, "results is NULL");
    const dcn_phase_list *l = map->phase;
    DCN_HIP(hipSetDevice(map->device));
    scratch mem;
    dcn_phase_solve_args sa;
    memset(&sa, 0, sizeof(sa));
    dcn_phase_result *d_results = nullptr;
    DCN_TRY(mem.get(&sa.decisions, l->n, "phase decisions"));
    DCN_TRY(mem.get(&sa.aggregates, dcn_phase_solve_blocks(l->n), "phase scan aggregates"));
    DCN_TRY(mem.get(&d_results, l->n, "phase results"));
    sa.site_pos = l->d_pos;
    sa.site_alleles = l->d_alleles;
    sa.links = l->d_links;
    sa.n_sites = l->n;
    sa.min_reads = prm->min_reads;
    sa.max_minor_permille = prm->max_minor_permille;
    sa.results = d_results;
    DCN_TRY(dcn_launch_phase_solve(sa, nullptr));
    DCN_HIP(hipMemcpy(results, d_results, l->n * sizeof(dcn_phase_result), hipMemcpyDeviceToHost));
    return DCN_OK;
}

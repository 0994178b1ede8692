// genotype_api.hip -- the C ABI of genotypes (dcn_anchor_map_genotype; kernel in genotype.hip, the shared arithmetic in
// dcn_genotype.h).  Count, scan, gather on the null stream with scratch of the call: the shape, the checks' style and the
// capacity protocol of dcn_anchor_map_pileup_call (pileup_api.hip), whose checks and scratch holder it shares.
#include "dcn_ctx.h"
#include "dcn_dump_sweep.h"
#include "dcn_genotype.h"
#include "dcn_verify.h"

#include <cstring>

using namespace dcn_impl;
using namespace dcn_pile_api;

static_assert(sizeof(dcn_genotype_params) == 32, "genotype params are ABI");
static_assert(sizeof(dcn_genotype_site) == 48, "genotype sites are ABI");

extern "C" int dcn_anchor_map_genotype(const dcn_index *map, const void *params, uint32_t record, uint64_t start, uint64_t n_bases,
                                       uint8_t *gt, uint8_t *gq, void *sites, uint64_t capacity, uint64_t *n_sites) {
    const dcn_genotype_params *prm = static_cast<const dcn_genotype_params *>(params);
    if (!prm) return dcn_fail(DCN_ERR_ARG, "params is NULL");
    if (prm->reserved[0] != 0 || prm->reserved[1] != 0) return dcn_fail(DCN_ERR_ARG, "params.reserved must be 0");
    if (prm->ploidy != 1 && prm->ploidy != 2) return dcn_fail(DCN_ERR_ARG, "params.ploidy must be 1 or 2");
    if (prm->min_gq > 99) return dcn_fail(DCN_ERR_ARG, "params.min_gq must be 0..99");
    if (prm->err_centi > 100000) return dcn_fail(DCN_ERR_ARG, "params.err_centi must be 0..100000");
    if (prm->het_centi > 100000) return dcn_fail(DCN_ERR_ARG, "params.het_centi must be 0..100000");
    DCN_TRY(check_qsums(map)); // (the map's checks, the pileup's, then the sums')
    uint64_t b0 = 0;
    DCN_TRY(check_range(map, "genotype", record, start, n_bases, &b0));
    if (!n_sites) return dcn_fail(DCN_ERR_ARG, "n_sites is NULL");
    *n_sites = 0;
    if (n_bases == 0) return DCN_OK;
    DCN_HIP(hipSetDevice(map->device));

    const uint32_t blocks = dcn_genotype_blocks(b0, n_bases);
    const uint64_t out_bytes = dcn_genotype_out_bytes(b0, n_bases), pad = b0 & 3u;
    scratch mem;
    dcn_genotype_args ga;
    memset(&ga, 0, sizeof(ga));
    uint32_t *d_counts = nullptr;
    uint64_t *d_offsets = nullptr;
    unsigned long long *d_sums = nullptr;
    DCN_TRY(mem.get(&ga.gt, out_bytes, "genotype gt"));
    DCN_TRY(mem.get(&ga.gq, out_bytes, "genotype gq"));
    DCN_TRY(mem.get(&d_counts, blocks, "genotype site counts"));
    DCN_TRY(mem.get(&d_offsets, (uint64_t)blocks + 1, "genotype site offsets"));
    DCN_TRY(mem.get(&d_sums, blocks / DCN_SCAN_BLOCK + 2, "genotype scan sums"));
    ga.counters = map->d_pileup;
    ga.sums = map->d_pileup_qsums;
    ga.bases = map->pileup_bases;
    ga.t_packed = map->store->d_packed;
    ga.t_invmask = map->store->d_invmask;
    ga.base0 = b0;
    ga.n = n_bases;
    ga.pos0 = start;
    ga.ploidy = prm->ploidy;
    ga.min_depth = prm->min_depth;
    ga.min_gq = prm->min_gq;
    ga.min_qual = prm->min_qual;
    ga.err_centi = prm->err_centi;
    ga.het_centi = prm->het_centi;
    ga.block_counts = d_counts;
    ga.block_offsets = d_offsets;
    DCN_TRY(dcn_launch_genotype(ga, false, nullptr));
    DCN_TRY(dcn_launch_offsets_scan(d_counts, blocks, d_sums, d_offsets, nullptr));
    uint64_t total = 0;
    DCN_HIP(hipMemcpy(&total, d_offsets + blocks, sizeof(uint64_t), hipMemcpyDeviceToHost));
    *n_sites = total;
    if (gt) DCN_HIP(hipMemcpy(gt, ga.gt + pad, n_bases, hipMemcpyDeviceToHost));
    if (gq) DCN_HIP(hipMemcpy(gq, ga.gq + pad, n_bases, hipMemcpyDeviceToHost));
    if (total > capacity)
        return dcn_fail(DCN_ERR_CAPACITY, "the sites hold " + std::to_string(capacity) + " entries, the range has " + std::to_string(total) +
                                              " (n_sites, gt and gq are complete: call again with that capacity)");
    if (total == 0) return DCN_OK;
    if (!sites) return dcn_fail(DCN_ERR_ARG, "sites is NULL");
    dcn_genotype_site *d_sites = nullptr;
    DCN_TRY(mem.get(&d_sites, total, "genotype sites"));
    ga.sites = d_sites;
    DCN_TRY(dcn_launch_genotype(ga, true, nullptr));
    DCN_HIP(hipMemcpy(sites, d_sites, total * sizeof(dcn_genotype_site), hipMemcpyDeviceToHost));
    return DCN_OK;
}

// blocks_api.hip -- the C ABI of reference blocks (dcn_anchor_map_reference_blocks, dcn_reference_blocks_merge of
// include/deacon_hip_blocks.h; kernels in blocks.hip, the rule in dcn_blocks.h).  Classify, breaks, count, scan, fill, reduce
// on the null stream with scratch of the call: the checks' style and the capacity protocol of dcn_anchor_map_genotype
// (genotype_api.hip), whose checks and scratch holder it shares.
#include "../../include/deacon_hip_blocks.h"
#include "dcn_blocks.h"
#include "dcn_ctx.h"
#include "dcn_dump_sweep.h"
#include "dcn_verify.h"

#include <cstring>
#include <string>
#include <vector>

using namespace dcn_impl;
using namespace dcn_pile_api;

static_assert(sizeof(dcn_block_params) == 48, "block params are ABI");
static_assert(sizeof(dcn_reference_block) == 40 && sizeof(dcn_blk_block) == 40, "reference blocks are ABI");
static_assert(DCN_BLOCK_NO_COVERAGE == DCN_BLK_NO_COVERAGE && DCN_BLOCK_UNCALLED == DCN_BLK_UNCALLED && DCN_BLOCK_REF == DCN_BLK_REF &&
                  DCN_BLOCK_VARIANT == DCN_BLK_VARIANT,
              "the classes of the header and of dcn_blocks.h");

extern "C" int dcn_anchor_map_reference_blocks(const dcn_index *map, const void *params, uint32_t record, uint64_t start, uint64_t n_bases,
                                               const uint64_t *breaks, uint64_t n_breaks, uint8_t *cls, void *blocks, uint64_t capacity,
                                               uint64_t *n_blocks) {
    const dcn_block_params *prm = static_cast<const dcn_block_params *>(params);
    if (!prm) return dcn_fail(DCN_ERR_ARG, "params is NULL");
    if (prm->reserved != 0) return dcn_fail(DCN_ERR_ARG, "params.reserved must be 0");
    if (prm->ploidy != 1 && prm->ploidy != 2) return dcn_fail(DCN_ERR_ARG, "params.ploidy must be 1 or 2");
    if (prm->min_gq > 99) return dcn_fail(DCN_ERR_ARG, "params.min_gq must be 0..99");
    if (prm->err_centi > 100000) return dcn_fail(DCN_ERR_ARG, "params.err_centi must be 0..100000");
    if (prm->het_centi > 100000) return dcn_fail(DCN_ERR_ARG, "params.het_centi must be 0..100000");
    if (prm->n_edges > DCN_BLK_MAX_EDGES) return dcn_fail(DCN_ERR_ARG, "params.n_edges must be 0..15");
    for (uint32_t i = 0; i < 16; ++i) {
        const uint32_t e = prm->edges[i];
        const std::string at = "params.edges[" + std::to_string(i) + "]";
        if (i >= prm->n_edges) {
            if (e != 0) return dcn_fail(DCN_ERR_ARG, at + " must be 0: it is not one of the n_edges");
            continue;
        }
        if (e < 1 || e > 99) return dcn_fail(DCN_ERR_ARG, at + " must be 1..99");
        if (i > 0 && e <= prm->edges[i - 1]) return dcn_fail(DCN_ERR_ARG, at + " is not above the edge in front of it");
    }
    DCN_TRY(check_qsums(map)); // (the map's checks, the pileup's, then the sums')
    uint64_t b0 = 0;
    DCN_TRY(check_range(map, "reference blocks", record, start, n_bases, &b0));
    if (n_bases > 0xFFFFFFFFull) return dcn_fail(DCN_ERR_ARG, "reference blocks: a range holds at most 4294967295 positions (a block's len is 32 bits)");
    if (!n_blocks) return dcn_fail(DCN_ERR_ARG, "n_blocks is NULL");
    if (n_breaks > 0 && !breaks) return dcn_fail(DCN_ERR_ARG, "breaks is NULL");
    for (uint64_t i = 0; i < n_breaks; ++i)
        if (breaks[i] < start || breaks[i] - start >= n_bases)
            return dcn_fail(DCN_ERR_ARG, "breaks[" + std::to_string(i) + "] = " + std::to_string(breaks[i]) + " is outside the range [" +
                                             std::to_string(start) + ", " + std::to_string(start + n_bases) + ")");
    *n_blocks = 0;
    if (n_bases == 0) return DCN_OK;
    DCN_HIP(hipSetDevice(map->device));

    const uint32_t groups = dcn_blocks_groups(b0, n_bases);
    const uint64_t out_bytes = dcn_blocks_out_bytes(b0, n_bases), pad = dcn_blocks_pad(b0);
    scratch mem, more;
    dcn_blocks_args ba;
    memset(&ba, 0, sizeof(ba));
    uint32_t *d_counts = nullptr;
    uint64_t *d_offsets = nullptr, *d_breaks = nullptr;
    unsigned long long *d_sums = nullptr;
    DCN_TRY(mem.get(&ba.cls, out_bytes, "block classes"));
    DCN_TRY(mem.get(&ba.gq, out_bytes, "block gq"));
    DCN_TRY(mem.get(&d_counts, groups, "block head counts"));
    DCN_TRY(mem.get(&d_offsets, (uint64_t)groups + 1, "block head offsets"));
    DCN_TRY(mem.get(&d_sums, groups / DCN_SCAN_BLOCK + 2, "block scan sums"));
    if (n_breaks) {
        std::vector<uint64_t> rel(breaks, breaks + n_breaks);
        for (uint64_t &q : rel) q -= start;
        DCN_TRY(mem.get(&d_breaks, n_breaks, "block breaks"));
        DCN_HIP(hipMemcpy(d_breaks, rel.data(), n_breaks * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    const dcn_blk_edges edges = dcn_blocks_pack_edges(prm->edges, prm->n_edges);
    ba.counters = map->d_pileup;
    ba.sums = map->d_pileup_qsums;
    ba.bases = map->pileup_bases;
    ba.t_packed = map->store->d_packed;
    ba.t_invmask = map->store->d_invmask;
    ba.base0 = b0;
    ba.n = n_bases;
    ba.pos0 = start;
    ba.ploidy = prm->ploidy;
    ba.min_depth = prm->min_depth;
    ba.min_gq = prm->min_gq;
    ba.min_qual = prm->min_qual;
    ba.err_centi = prm->err_centi;
    ba.het_centi = prm->het_centi;
    ba.edges_lo = edges.lo;
    ba.edges_hi = edges.hi;
    ba.breaks = d_breaks;
    ba.n_breaks = n_breaks;
    ba.block_counts = d_counts;
    ba.block_offsets = d_offsets;
    DCN_TRY(dcn_launch_blocks_classify(ba, nullptr));
    DCN_TRY(dcn_launch_blocks_breaks(ba, nullptr));
    DCN_TRY(dcn_launch_blocks_heads(ba, false, nullptr));
    DCN_TRY(dcn_launch_offsets_scan(d_counts, groups, d_sums, d_offsets, nullptr));
    uint64_t total = 0;
    DCN_HIP(hipMemcpy(&total, d_offsets + groups, sizeof(uint64_t), hipMemcpyDeviceToHost));
    *n_blocks = total;
    if (cls) DCN_HIP(hipMemcpy(cls, ba.cls + pad, n_bases, hipMemcpyDeviceToHost));
    if (total > capacity)
        return dcn_fail(DCN_ERR_CAPACITY, "the blocks hold " + std::to_string(capacity) + " entries, the range has " + std::to_string(total) +
                                              " (n_blocks and cls are complete: call again with that capacity)");
    if (total == 0) return DCN_OK;
    if (!blocks) return dcn_fail(DCN_ERR_ARG, "blocks is NULL");
    dcn_reference_block *d_blocks = nullptr;
    DCN_TRY(more.get(&d_blocks, total, "reference blocks"));
    ba.blocks = d_blocks;
    ba.n_blocks = total;
    DCN_TRY(dcn_launch_blocks_fill(ba, nullptr));
    DCN_TRY(dcn_launch_blocks_heads(ba, true, nullptr));
    DCN_HIP(hipMemcpy(blocks, d_blocks, total * sizeof(dcn_reference_block), hipMemcpyDeviceToHost));
    return DCN_OK;
}

extern "C" int dcn_reference_blocks_merge(void *blocks, uint64_t n, uint64_t *n_merged) {
    if (!n_merged) return dcn_fail(DCN_ERR_ARG, "n_merged is NULL");
    if (n > 0 && !blocks) return dcn_fail(DCN_ERR_ARG, "blocks is NULL");
    dcn_blk_block *b = static_cast<dcn_blk_block *>(blocks);
    // the checks first, so that an error leaves the array as it was
    uint64_t len = n ? b[0].len : 0;
    for (uint64_t i = 1; i < n; ++i) {
        const dcn_blk_block &p = b[i - 1], &q = b[i];
        if (p.pos + p.len > q.pos || p.pos + p.len < p.pos)
            return dcn_fail(DCN_ERR_ARG, "blocks[" + std::to_string(i) + "] at " + std::to_string(q.pos) + " does not lie behind blocks[" +
                                             std::to_string(i - 1) + "], which ends at " + std::to_string(p.pos + p.len));
        len = dcn_blocks_mergeable(p, q) ? len + q.len : q.len;
        if (len > 0xFFFFFFFFull)
            return dcn_fail(DCN_ERR_ARG, "merging into blocks[" + std::to_string(i) + "] gives a len above 4294967295");
    }
    uint64_t kept = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (kept > 0 && dcn_blocks_mergeable(b[kept - 1], b[i])) dcn_blocks_merge_into(b[kept - 1], b[i]);
        else b[kept++] = b[i];
    }
    *n_merged = kept;
    return DCN_OK;
}

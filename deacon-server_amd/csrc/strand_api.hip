// strand_api.hip -- the C ABI of the read-outs of strand evidence (dcn_anchor_map_strand_evidence,
// dcn_anchor_map_indels_strand; kernels in strand.hip, the rule in dcn_strand.h; the planes' switch and fetch are with the
// pileup's, pileup_api.hip).  Both run on the null stream with scratch of the call, as dcn_anchor_map_genotype does.
#include "dcn_ctx.h"
#include "dcn_indels.h"
#include "dcn_insertions.h"
#include "dcn_strand.h"
#include "dcn_verify.h"

#include <cstring>
#include <vector>

using namespace dcn_impl;
using namespace dcn_pile_api;

static_assert(sizeof(dcn_strand_params) == 16 && sizeof(dcn_strand_query) == 32, "strand params and queries are ABI");
static_assert(sizeof(dcn_strand_site) == sizeof(dcn_strand_site_item), "strand sites are ABI");
static_assert(DCN_STRAND_BIAS == DCN_STRAND_FLAG_BIAS && DCN_STRAND_ONE_SIDED == DCN_STRAND_FLAG_ONE_SIDED,
              "the flags of the header and of dcn_strand.h");
static_assert(DCN_INDEL_DELETION == DCN_INDEL_SITE_DELETION && DCN_INDEL_FRONT == DCN_INDEL_SITE_FRONT, "the site flags of the header");

namespace {
// the record is one of the map's: its first base in the store and its length
int check_record(const dcn_index *map, const char *who, uint32_t record, uint64_t *base0, uint64_t *len) {
    DCN_TRY(check_range(map, who, record, 0, 0, base0));
    *len = map->store->rec_len[record];
    return DCN_OK;
}
} // namespace

extern "C" int dcn_anchor_map_strand_evidence(const dcn_index *map, const void *params, uint32_t record, const void *queries,
                                              uint64_t n_queries, void *out) {
    const dcn_strand_params *prm = static_cast<const dcn_strand_params *>(params);
    if (!prm) return dcn_fail(DCN_ERR_ARG, "params is NULL");
    if (prm->reserved != 0) return dcn_fail(DCN_ERR_ARG, "params.reserved must be 0");
    DCN_TRY(check_strands(map)); // (the map's checks, the pileup's, then the planes')
    uint64_t b0 = 0, len = 0;
    DCN_TRY(check_record(map, "strand evidence", record, &b0, &len));
    if (n_queries == 0) return DCN_OK;
    if (!queries || !out) return dcn_fail(DCN_ERR_ARG, "queries/out is NULL");
    const dcn_strand_query *qs = static_cast<const dcn_strand_query *>(queries);
    std::vector<dcn_strand_query_item> items(n_queries);
    for (uint64_t q = 0; q < n_queries; ++q) {
        const dcn_strand_query &u = qs[q];
        const auto bad = [q](const std::string &what) { return dcn_fail(DCN_ERR_ARG, "query " + std::to_string(q) + ": " + what); };
        if (u.pos >= len) return bad("pos " + std::to_string(u.pos) + " is past the record's " + std::to_string(len) + " bases");
        if (u.kind > 1) return bad("kind must be 0 or 1");
        if (u.reserved != 0) return bad("reserved must be 0");
        if (u.kind == 0) {
            if (u.ref_code > 3) return bad("ref_code must be 0..3");
            if (u.alt_mask == 0) return bad("alt_mask is empty");
            if (u.alt_mask > 15) return bad("alt_mask has bits above 3");
            if (u.alt_mask & (1u << u.ref_code)) return bad("alt_mask holds ref_code");
        } else if (u.count_reverse > u.count) {
            return bad("count_reverse " + std::to_string(u.count_reverse) + " is above count " + std::to_string(u.count));
        }
        items[q] = {b0 + u.pos, u.kind, u.ref_code, u.alt_mask, u.count, u.count_reverse, 0u};
    }
    DCN_HIP(hipSetDevice(map->device));
    scratch mem;
    dcn_strand_query_item *d_items = nullptr;
    dcn_strand_evidence_args sa;
    memset(&sa, 0, sizeof(sa));
    DCN_TRY(mem.get(&d_items, n_queries, "strand queries"));
    DCN_TRY(mem.get(&sa.out, n_queries, "strand sites"));
    DCN_HIP(hipMemcpy(d_items, items.data(), n_queries * sizeof(dcn_strand_query_item), hipMemcpyHostToDevice));
    sa.counters = map->d_pileup;
    sa.strands = map->d_pileup_strands;
    sa.bases = map->pileup_bases;
    sa.queries = d_items;
    sa.n = n_queries;
    sa.max_sb_centi = prm->max_sb_centi;
    sa.min_alt_strand = prm->min_alt_strand;
    sa.min_strand_depth = prm->min_strand_depth;
    DCN_TRY(dcn_launch_strand_evidence(sa, nullptr));
    DCN_HIP(hipMemcpy(out, sa.out, n_queries * sizeof(dcn_strand_site), hipMemcpyDeviceToHost));
    return DCN_OK;
}

extern "C" int dcn_anchor_map_indels_strand(const dcn_index *map, uint32_t record, const void *sites, uint64_t n_sites, const uint8_t *bases,
                                            uint32_t *count_reverse) {
    DCN_TRY(check_pileup(map));
    uint64_t b0 = 0, len = 0;
    DCN_TRY(check_record(map, "indels strand", record, &b0, &len));
    if (n_sites == 0) return DCN_OK;
    if (!sites || !count_reverse) return dcn_fail(DCN_ERR_ARG, "sites/count_reverse is NULL");
    const dcn_indel_site *ss = static_cast<const dcn_indel_site *>(sites);
    std::vector<uint64_t> keys(n_sites), offsets(n_sites);
    std::vector<uint32_t> lens(n_sites);
    uint64_t inserted = 0;
    bool any_ins = false, any_del = false;
    for (uint64_t s = 0; s < n_sites; ++s) {
        const dcn_indel_site &u = ss[s];
        const auto bad = [s](const std::string &what) { return dcn_fail(DCN_ERR_ARG, "site " + std::to_string(s) + ": " + what); };
        if (u.pos >= len) return bad("pos " + std::to_string(u.pos) + " is past the record's " + std::to_string(len) + " bases");
        const bool del = (u.flags & DCN_INDEL_DELETION) != 0;
        keys[s] = dcn_indel_strand_key(b0 + u.pos, del ? 1u : (u.flags & DCN_INDEL_FRONT) ? 0u : 2u);
        if (s > 0 && keys[s] <= keys[s - 1]) return bad("the sites are not in rule I6's order");
        lens[s] = u.len;
        offsets[s] = inserted;
        if (del) {
            if (!map->del_ledger) return bad("the map keeps no deletion ledger (dcn_anchor_map_pileup_keep_deletions)");
            any_del = true;
        } else {
            if (!map->ledger) return bad("the map keeps no insertion ledger (dcn_anchor_map_pileup_keep_insertions)");
            if (u.bases_offset != inserted)
                return bad("bases_offset " + std::to_string(u.bases_offset) + " is not the " + std::to_string(inserted) +
                           " inserted bases of the sites in front");
            if (u.len > 0 && !bases) return dcn_fail(DCN_ERR_ARG, "bases is NULL");
            inserted += u.len;
            any_ins = true;
        }
    }
    DCN_HIP(hipSetDevice(map->device));
    scratch mem;
    dcn_indel_strand_args ia;
    memset(&ia, 0, sizeof(ia));
    uint64_t *d_keys = nullptr, *d_offsets = nullptr;
    uint32_t *d_lens = nullptr;
    uint8_t *d_bases = nullptr;
    DCN_TRY(mem.get(&d_keys, n_sites, "indel strand keys"));
    DCN_TRY(mem.get(&d_offsets, n_sites, "indel strand base offsets"));
    DCN_TRY(mem.get(&d_lens, n_sites, "indel strand lengths"));
    DCN_TRY(mem.get(&d_bases, std::max<uint64_t>(inserted, 1), "indel strand bases"));
    DCN_TRY(mem.get(&ia.count_reverse, n_sites, "indel strand counts"));
    DCN_HIP(hipMemcpy(d_keys, keys.data(), n_sites * sizeof(uint64_t), hipMemcpyHostToDevice));
    DCN_HIP(hipMemcpy(d_offsets, offsets.data(), n_sites * sizeof(uint64_t), hipMemcpyHostToDevice));
    DCN_HIP(hipMemcpy(d_lens, lens.data(), n_sites * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (inserted) DCN_HIP(hipMemcpy(d_bases, bases, inserted, hipMemcpyHostToDevice));
    DCN_HIP(hipMemset(ia.count_reverse, 0, n_sites * sizeof(uint32_t)));
    ia.site_keys = d_keys;
    ia.site_len = d_lens;
    ia.site_bases_offset = d_offsets;
    ia.site_bases = d_bases;
    ia.n_sites = n_sites;
    if (any_ins) { // (only a ledger that has a site is walked)
        ia.ins_events = map->ledger->d_events;
        ia.ins_ledger_bases = map->ledger->d_bases;
        ia.n_ins_events = map->ledger->n_events;
    }
    if (any_del) {
        ia.del_events = map->del_ledger->d_events;
        ia.n_del_events = map->del_ledger->n_events;
    }
    DCN_TRY(dcn_launch_indel_strand(ia, nullptr));
    DCN_HIP(hipMemcpy(count_reverse, ia.count_reverse, n_sites * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return DCN_OK;
}

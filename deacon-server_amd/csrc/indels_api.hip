// indels_api.hip -- the C ABI of deletion ledgers and indel genotypes (dcn_anchor_map_pileup_keep_deletions,
// dcn_anchor_map_deletions_info / _fetch, dcn_anchor_map_indels_genotype) and the append that dcn_pileup_batch and
// dcn_pileup_batch_qual make on a map that keeps a deletion ledger (kernels in indels.hip, the shared arithmetic in
// dcn_indels.h).  The append is insertions_api.hip's with one total and one scan, on the context's stream behind the pileup
// kernel; fetch and genotype run on the null stream with scratch of the call, as dcn_anchor_map_insertions_fetch / _call.
#include "dcn_ctx.h"
#include "dcn_dump_sweep.h"
#include "dcn_indels.h"
#include "dcn_insertions.h"
#include "dcn_ledger_range.h"
#include "dcn_verify.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace dcn_impl;
using namespace dcn_ledger_api;
using dcn_pile_api::check_pileup;

static_assert(sizeof(dcn_deletion) == 16, "ledger events are ABI");
static_assert(sizeof(dcn_indel_params) == 32 && sizeof(dcn_indel_site) == 48, "indel params and sites are ABI");

namespace {
constexpr uint64_t DCN_DEL_LEDGER_INITIAL_EVENTS = 1ull << 20;

// events the ledger starts with: DCN_DELETION_LEDGER_EVENTS, read when the ledger first grows
uint64_t ledger_initial_events() {
    const char *s = std::getenv("DCN_DELETION_LEDGER_EVENTS");
    const uint64_t v = s && *s ? std::strtoull(s, nullptr, 10) : DCN_DEL_LEDGER_INITIAL_EVENTS;
    return std::max<uint64_t>(v, 1);
}

int check_ledger(const dcn_index *map) {
    DCN_TRY(check_pileup(map));
    if (!map->del_ledger) return dcn_fail(DCN_ERR_ARG, "the map keeps no deletion ledger (dcn_anchor_map_pileup_keep_deletions)");
    return DCN_OK;
}

// What fetch and the deletion side of a genotype call share, behind the checks: STARTS of the range from the ledger, its
// scan and the scatter of the range's events into the buckets.  *n_slots = 0: no event begins in the range (ra->counts is
// null then when the ledger is empty).
int del_buckets(const dcn_index *map, const char *who, uint64_t b0, uint64_t start, uint64_t n_bases, scratch &mem, dcn_del_range_args *ra,
                uint64_t *n_slots) {
    *n_slots = 0;
    const dcn_del_ledger *l = map->del_ledger;
    memset(ra, 0, sizeof(*ra));
    if (n_bases == 0 || l->n_events == 0) return DCN_OK;
    ra->base0 = b0;
    ra->n = n_bases;
    ra->pos0 = start;
    ra->events = l->d_events;
    ra->n_events = l->n_events;
    DCN_TRY(mem.get_zeroed(&ra->counts, n_bases, "deletion starts"));
    DCN_TRY(dcn_launch_del_plane(*ra, nullptr));
    uint64_t *d_offsets = nullptr, total = 0;
    DCN_TRY(scan_counts(mem, ra->counts, n_bases, &d_offsets, &total, "deletion bucket offsets"));
    ra->bucket_offsets = d_offsets;
    if (total == 0) return DCN_OK;
    if (total > UINT32_MAX) return too_many(who, total);
    DCN_TRY(mem.get_zeroed(&ra->cursor, n_bases, "deletion cursors"));
    DCN_TRY(mem.get_zeroed(&ra->slots, total, "deletion buckets")); // (every slot is written; event 0 exists)
    DCN_TRY(dcn_launch_del_scatter(*ra, nullptr));
    ra->n_slots = total;
    *n_slots = total;
    return DCN_OK;
}

// The insertion side of a genotype call: dcn_anchor_map_insertions_call's buckets (range_buckets, the plain INS plane) and
// its winner kernel, with "INS > 0" as the flag (rule I1: L6's thresholds do not apply).  *n_flagged = 0: no candidate.
int ins_winners(const dcn_index *map, const char *who, uint32_t record, uint64_t start, uint64_t n_bases, scratch &mem, dcn_ins_range_args *ra,
                uint64_t *n_flagged) {
    *n_flagged = 0;
    uint64_t n_slots = 0, n_all = 0;
    DCN_TRY(range_buckets(map, who, false, record, start, n_bases, 0, 0, mem, ra, &n_slots));
    if (n_slots == 0) return DCN_OK;
    DCN_TRY(mem.get(&ra->flags, n_bases, "insertion flags"));
    DCN_TRY(dcn_launch_indel_flags(ra->counts, ra->flags, n_bases, nullptr));
    uint64_t *d_allele_offsets = nullptr;
    DCN_TRY(scan_counts(mem, ra->flags, n_bases, &d_allele_offsets, &n_all, "insertion allele offsets"));
    ra->allele_offsets = d_allele_offsets;
    ra->n_alleles = n_all;
    DCN_TRY(mem.get_zeroed(&ra->win_event, n_all, "insertion winners"));
    DCN_TRY(mem.get_zeroed(&ra->win_count, n_all, "insertion winner counts"));
    DCN_TRY(mem.get_zeroed(&ra->win_events, n_all, "insertion winner events"));
    DCN_TRY(mem.get_zeroed(&ra->win_len, n_all, "insertion winner lengths"));
    DCN_TRY(mem.get_zeroed(&ra->win_pos, n_all, "insertion winner positions"));
    DCN_TRY(dcn_launch_ins_winner(*ra, nullptr));
    *n_flagged = n_all;
    return DCN_OK;
}
} // namespace

void dcn_del_ledger_free(dcn_del_ledger *l) {
    if (!l) return;
    for (void *p : {(void *)l->d_events, (void *)l->d_row_events, (void *)l->d_event_offsets, (void *)l->d_event_sums, (void *)l->d_totals})
        if (p) hipFree(p);
    delete l;
}

extern "C" int dcn_anchor_map_pileup_keep_deletions(dcn_index *map, int keep) {
    DCN_TRY(check_pileup(map));
    if (!keep) {
        if (map->del_ledger) {
            DCN_HIP(hipSetDevice(map->device));
            dcn_del_ledger_free(map->del_ledger);
        }
        map->del_ledger = nullptr;
        return DCN_OK;
    }
    if (map->del_ledger) return DCN_OK;
    if (map->pileup_rows != 0) // rule R1
        return dcn_fail(DCN_ERR_ARG, std::to_string(map->pileup_rows) + " rows have added to the pileup since it was enabled or reset: a ledger "
                                                                         "begins with the counters (dcn_anchor_map_pileup_reset first)");
    DCN_HIP(hipSetDevice(map->device));
    dcn_del_ledger *l = new (std::nothrow) dcn_del_ledger();
    if (!l) return dcn_fail(DCN_ERR_NOMEM, "host allocation failed");
    const int rc = dev_alloc_zeroed(&l->d_totals, 2, "deletion totals");
    if (rc != DCN_OK) {
        delete l;
        return rc;
    }
    map->del_ledger = l;
    return DCN_OK;
}

int dcn_deletions_append(dcn_ctx *c, dcn_index *map, const dcn_pileup_args &rows) {
    dcn_del_ledger *l = map->del_ledger;
    hipStream_t st = c->stream;
    const uint64_t n_work = rows.n_work;
    if (n_work == 0) return DCN_OK;
    if (l->rows_cap < n_work) {
        uint64_t c0 = 0;
        l->rows_cap = 0;
        DCN_TRY(grow(&l->d_row_events, &c0, n_work, "deletion row events"));
        l->rows_cap = n_work;
    }
    dcn_del_append_args aa;
    memset(&aa, 0, sizeof(aa));
    aa.rows = rows;
    aa.row_events = l->d_row_events;
    aa.totals = l->d_totals;
    DCN_TRY(dcn_launch_del_count(aa, st));
    unsigned long long totals[2] = {0, 0};
    DCN_HIP(hipMemcpyAsync(totals, l->d_totals, sizeof(totals), hipMemcpyDeviceToHost, st));
    DCN_HIP(hipStreamSynchronize(st));
    if (totals[0] == 0) return DCN_OK; // no D run in the batch: one pass and one read-back
    DCN_HIP(hipMemsetAsync(l->d_totals, 0, sizeof(totals), st)); // (zero between calls)
    if (n_work > UINT32_MAX) return dcn_fail(DCN_ERR_INTERNAL, "more than 2^32 - 1 aligned rows"); // (dcn_align_check_rows has refused them)
    if (l->offsets_cap < n_work + 1) {
        uint64_t c0 = 0, c1 = 0;
        l->offsets_cap = 0;
        DCN_TRY(grow(&l->d_event_offsets, &c0, n_work + 1, "deletion event offsets"));
        DCN_TRY(grow(&l->d_event_sums, &c1, n_work / DCN_SCAN_BLOCK + 2, "deletion scan sums"));
        l->offsets_cap = n_work + 1;
    }
    DCN_TRY(dcn_launch_offsets_scan(l->d_row_events, (uint32_t)n_work, l->d_event_sums, l->d_event_offsets, st));
    const uint64_t need = l->n_events + totals[0];
    if (need > l->event_cap) { // geometric; the copy on the context's stream, which is waited for
        const uint64_t cap2 = std::max(need, l->event_cap ? l->event_cap * 2 : ledger_initial_events());
        dcn_del_event *d = nullptr;
        DCN_TRY(dev_alloc(&d, cap2, "deletion events"));
        hipError_t e = hipSuccess;
        if (l->n_events) e = hipMemcpyAsync(d, l->d_events, l->n_events * sizeof(dcn_del_event), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            hipFree(d);
            return dcn_hip_fail(e, "deletion events");
        }
        if (l->d_events) hipFree(l->d_events);
        l->d_events = d;
        l->event_cap = cap2;
    }
    aa.event_offsets = l->d_event_offsets;
    aa.events = l->d_events;
    aa.event0 = l->n_events;
    DCN_TRY(dcn_launch_del_write(aa, st));
    l->n_events += totals[0];
    l->n_deleted += totals[1];
    return DCN_OK;
}

extern "C" int dcn_anchor_map_deletions_info(const dcn_index *map, uint64_t *n_events, uint64_t *n_deleted) {
    DCN_TRY(check_ledger(map));
    if (n_events) *n_events = map->del_ledger->n_events;
    if (n_deleted) *n_deleted = map->del_ledger->n_deleted;
    return DCN_OK;
}

extern "C" int dcn_anchor_map_deletions_fetch(const dcn_index *map, uint32_t record, uint64_t start, uint64_t n_bases, void *events,
                                              uint64_t capacity, uint64_t *n_events) {
    if (!n_events) return dcn_fail(DCN_ERR_ARG, "n_events is NULL");
    DCN_TRY(check_ledger(map));
    *n_events = 0;
    uint64_t b0 = 0;
    DCN_TRY(check_range(map, "deletions fetch", record, start, n_bases, &b0));
    DCN_HIP(hipSetDevice(map->device));
    scratch mem;
    if (n_bases && map->del_ledger->n_events) DCN_TRY(mem.reserve(16 * n_bases + (1u << 16), "deletions fetch scratch")); // starts, offsets, cursors
    dcn_del_range_args ra;
    uint64_t n_slots = 0;
    DCN_TRY(del_buckets(map, "deletions fetch", b0, start, n_bases, mem, &ra, &n_slots));
    *n_events = n_slots;
    if (n_slots == 0) return DCN_OK;
    if (n_slots > capacity)
        return dcn_fail(DCN_ERR_CAPACITY, "the array holds " + std::to_string(capacity) + " events, the range has " + std::to_string(n_slots) +
                                              " (n_events is complete: call again with that capacity)");
    if (!events) return dcn_fail(DCN_ERR_ARG, "events is NULL");
    dcn_deletion *d_out = nullptr;
    DCN_TRY(mem.get(&d_out, n_slots, "deletion events of the range"));
    ra.out_events = d_out;
    DCN_TRY(dcn_launch_del_gather(ra, nullptr));
    dcn_deletion *out = static_cast<dcn_deletion *>(events);
    DCN_HIP(hipMemcpy(out, d_out, n_slots * sizeof(dcn_deletion), hipMemcpyDeviceToHost));
    // rule R4: the buckets are in ascending position; inside one the order is the scatter's, so each is sorted here
    std::sort(out, out + n_slots, [](const dcn_deletion &a, const dcn_deletion &b) {
        if (a.pos != b.pos) return a.pos < b.pos;
        if (a.len != b.len) return a.len < b.len;
        return (a.flags & DCN_DELETION_REVERSE) < (b.flags & DCN_DELETION_REVERSE);
    });
    return DCN_OK;
}

extern "C" int dcn_anchor_map_indels_genotype(const dcn_index *map, const void *params, uint32_t record, uint64_t start, uint64_t n_bases,
                                              void *sites, uint64_t site_capacity, uint8_t *bases, uint64_t base_capacity, uint64_t *n_sites,
                                              uint64_t *n_inserted) {
    const dcn_indel_params *prm = static_cast<const dcn_indel_params *>(params);
    if (!prm) return dcn_fail(DCN_ERR_ARG, "params is NULL");
    if (prm->reserved != 0) return dcn_fail(DCN_ERR_ARG, "params.reserved must be 0");
    if (prm->ploidy != 1 && prm->ploidy != 2) return dcn_fail(DCN_ERR_ARG, "params.ploidy must be 1 or 2");
    if (prm->min_gq > 99) return dcn_fail(DCN_ERR_ARG, "params.min_gq must be 0..99");
    if (prm->indel_centi > 100000) return dcn_fail(DCN_ERR_ARG, "params.indel_centi must be 0..100000");
    if (prm->het_centi > 100000) return dcn_fail(DCN_ERR_ARG, "params.het_centi must be 0..100000");
    if (!n_sites || !n_inserted) return dcn_fail(DCN_ERR_ARG, "n_sites/n_inserted is NULL");
    DCN_TRY(check_pileup(map));
    if (!map->ledger && !map->del_ledger)
        return dcn_fail(DCN_ERR_ARG, "the map keeps neither an insertion ledger nor a deletion ledger (dcn_anchor_map_pileup_keep_insertions, "
                                     "dcn_anchor_map_pileup_keep_deletions)");
    *n_sites = 0;
    *n_inserted = 0;
    uint64_t b0 = 0;
    DCN_TRY(check_range(map, "indels genotype", record, start, n_bases, &b0));
    if (n_bases == 0) return DCN_OK;
    DCN_HIP(hipSetDevice(map->device));

    scratch mem;
    // the arrays sized by the range: 28 bytes a position for the insertion side (counts, flags, two scans, cursors), 24 for the
    // deletion side (starts, their scan, cursors, the winners); the buckets and the sites, sized by totals, mostly fit behind
    DCN_TRY(mem.reserve(56 * n_bases + (1u << 20), "indels genotype scratch"));
    dcn_ins_range_args ia;
    dcn_del_range_args da;
    uint64_t n_ins = 0, n_del = 0;
    memset(&ia, 0, sizeof(ia));
    memset(&da, 0, sizeof(da));
    if (map->ledger) DCN_TRY(ins_winners(map, "indels genotype", record, start, n_bases, mem, &ia, &n_ins));
    if (map->del_ledger) {
        DCN_TRY(del_buckets(map, "indels genotype", b0, start, n_bases, mem, &da, &n_del));
        if (n_del) {
            DCN_TRY(mem.get_zeroed(&da.win_count, n_bases, "deletion winner counts"));
            DCN_TRY(mem.get_zeroed(&da.win_len, n_bases, "deletion winner lengths"));
            DCN_TRY(dcn_launch_del_winner(da, nullptr));
        }
    }
    if (n_ins == 0 && n_del == 0) return DCN_OK; // no candidate in the range

    const uint32_t blocks = dcn_indel_site_blocks(n_bases);
    dcn_indel_site_args sa;
    memset(&sa, 0, sizeof(sa));
    uint32_t *d_counts = nullptr;
    uint64_t *d_offsets = nullptr, total = 0;
    unsigned long long inserted = 0;
    sa.counters = map->d_pileup;
    sa.bases = map->pileup_bases;
    sa.base0 = b0;
    sa.n = n_bases;
    sa.pos0 = start;
    sa.ploidy = prm->ploidy;
    sa.min_depth = prm->min_depth;
    sa.min_gq = prm->min_gq;
    sa.min_qual = prm->min_qual;
    sa.min_count = prm->min_count;
    sa.indel_centi = prm->indel_centi;
    sa.het_centi = prm->het_centi;
    if (n_ins) {
        sa.ins_flags = ia.flags;
        sa.ins_offsets = ia.allele_offsets;
        sa.ins_event = ia.win_event;
        sa.ins_count = ia.win_count;
        sa.ins_events = ia.win_events;
        sa.ins_len = ia.win_len;
        sa.ins_ledger = ia.events;
        sa.ins_ledger_bases = ia.ledger_bases;
    }
    if (n_del) {
        sa.del_starts = da.counts;
        sa.del_count = da.win_count;
        sa.del_len = da.win_len;
    }
    DCN_TRY(mem.get(&d_counts, blocks, "indel site counts"));
    DCN_TRY(mem.get_zeroed(&sa.n_inserted, 1, "indel inserted bases"));
    sa.block_counts = d_counts;
    // count, scan, write: genotype_api.hip's shape
    DCN_TRY(dcn_launch_indel_sites(sa, false, nullptr));
    DCN_TRY(scan_counts(mem, d_counts, blocks, &d_offsets, &total, "indel site offsets"));
    sa.block_offsets = d_offsets;
    DCN_HIP(hipMemcpy(&inserted, sa.n_inserted, sizeof(inserted), hipMemcpyDeviceToHost));
    *n_sites = total;
    *n_inserted = inserted;
    if (total > site_capacity || inserted > base_capacity)
        return dcn_fail(DCN_ERR_CAPACITY, "the arrays hold " + std::to_string(site_capacity) + " sites and " + std::to_string(base_capacity) +
                                              " bases, the range has " + std::to_string(total) + " and " + std::to_string(inserted) +
                                              " (both counts are complete: call again with those capacities)");
    if (total == 0) return DCN_OK;
    if (!sites || (inserted > 0 && !bases)) return dcn_fail(DCN_ERR_ARG, "sites/bases is NULL");
    if (total > UINT32_MAX) return too_many("indels genotype", total); // (never: at most two sites per position of a record)
    dcn_indel_site *d_sites = nullptr;
    uint64_t *d_site_offsets = nullptr, check = 0;
    DCN_TRY(mem.get(&d_sites, total, "indel sites"));
    DCN_TRY(mem.get(&sa.site_lens, total, "indel site lengths"));
    DCN_TRY(mem.get(&sa.site_event, total, "indel site events"));
    sa.sites = d_sites;
    sa.n_sites = total;
    DCN_TRY(dcn_launch_indel_sites(sa, true, nullptr));
    DCN_TRY(scan_counts(mem, sa.site_lens, total, &d_site_offsets, &check, "indel base offsets"));
    if (check != inserted) return dcn_fail(DCN_ERR_INTERNAL, "indels genotype: the two passes disagree on the inserted bases");
    sa.site_offsets = d_site_offsets;
    DCN_TRY(mem.get(&sa.out_bases, inserted, "inserted bases of the sites"));
    DCN_TRY(dcn_launch_indel_bases(sa, nullptr));
    DCN_HIP(hipMemcpy(sites, d_sites, total * sizeof(dcn_indel_site), hipMemcpyDeviceToHost));
    if (inserted) DCN_HIP(hipMemcpy(bases, sa.out_bases, inserted, hipMemcpyDeviceToHost));
    return DCN_OK;
}

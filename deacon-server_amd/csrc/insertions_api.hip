// insertions_api.hip -- the C ABI of insertion ledgers (dcn_anchor_map_pileup_keep_insertions, dcn_anchor_map_insertions_info
// / _fetch / _call) and the append that dcn_pileup_batch makes on a map that keeps one (kernels in insertions.hip, the
// shared arithmetic in dcn_insertions.h).  Both halves are count, scan, gather: the append on the context's stream behind
// the pileup kernel, fetch and call on the null stream with scratch of the call, as dcn_anchor_map_pileup_call.
#include "dcn_ctx.h"
#include "dcn_dump_sweep.h"
#include "dcn_insertions.h"
#include "dcn_ledger_range.h"
#include "dcn_verify.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace dcn_impl;
using namespace dcn_ledger_api;

static_assert(sizeof(dcn_insertion) == 24 && sizeof(dcn_insertion_allele) == 32, "ledger events and alleles are ABI");
static_assert(DCN_INSERTION_FRONT == DCN_INS_FRONT && DCN_INSERTION_REVERSE == DCN_INS_REVERSE, "the flags of the header and of dcn_insertions.h");

namespace {
constexpr uint64_t DCN_LEDGER_INITIAL_EVENTS = 1ull << 20;
constexpr uint64_t DCN_LEDGER_BASES_PER_EVENT = 8; // what the bases array starts with per event: it grows on its own

// events the ledger starts with: DCN_INSERTION_LEDGER_EVENTS, read when the ledger first grows
uint64_t ledger_initial_events() {
    const char *s = std::getenv("DCN_INSERTION_LEDGER_EVENTS");
    const uint64_t v = s && *s ? std::strtoull(s, nullptr, 10) : DCN_LEDGER_INITIAL_EVENTS;
    return std::max<uint64_t>(v, 1);
}

// at least `need` T behind *p, of which the first `used` are kept: geometric, the copy on `stream`, which is waited for
template <typename T>
int ledger_grow(T **p, uint64_t *cap, uint64_t used, uint64_t need, uint64_t initial, const char *what, hipStream_t stream) {
    if (need <= *cap) return DCN_OK;
    const uint64_t cap2 = std::max(need, *cap ? *cap * 2 : initial);
    T *d = nullptr;
    DCN_TRY(dev_alloc(&d, cap2, what));
    hipError_t e = hipSuccess;
    if (used) e = hipMemcpyAsync(d, *p, used * sizeof(T), hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) {
        hipFree(d);
        return dcn_hip_fail(e, what);
    }
    if (*p) hipFree(*p);
    *p = d;
    *cap = cap2;
    return DCN_OK;
}

int check_pileup(const dcn_index *map) {
    DCN_TRY(check_store(map));
    if (!map->d_pileup) return dcn_fail(DCN_ERR_ARG, "the map has no pileup (dcn_anchor_map_pileup_enable)");
    return DCN_OK;
}

int check_ledger(const dcn_index *map) {
    DCN_TRY(check_pileup(map));
    if (!map->ledger) return dcn_fail(DCN_ERR_ARG, "the map keeps no insertion ledger (dcn_anchor_map_pileup_keep_insertions)");
    return DCN_OK;
}

int capacity_error(const char *what, uint64_t events, uint64_t event_capacity, uint64_t bases, uint64_t base_capacity) {
    return dcn_fail(DCN_ERR_CAPACITY, std::string("the arrays hold ") + std::to_string(event_capacity) + " " + what + " and " +
                                          std::to_string(base_capacity) + " bases, the range has " + std::to_string(events) + " and " +
                                          std::to_string(bases) + " (both counts are complete: call again with those capacities)");
}
} // namespace

// ---- dcn_ledger_range.h: shared with indels_api.hip ------------------------------------------------------------------
int dcn_ledger_api::scan_counts(scratch &mem, const uint32_t *d_counts, uint64_t n, uint64_t **d_offsets, uint64_t *total, const char *what) {
    unsigned long long *d_sums = nullptr;
    DCN_TRY(mem.get(d_offsets, n + 1, what));
    DCN_TRY(mem.get(&d_sums, n / DCN_SCAN_BLOCK + 2, "ledger scan sums"));
    DCN_TRY(dcn_launch_offsets_scan(d_counts, (uint32_t)n, d_sums, *d_offsets, nullptr));
    DCN_HIP(hipMemcpy(total, *d_offsets + n, sizeof(uint64_t), hipMemcpyDeviceToHost));
    return DCN_OK;
}

int dcn_ledger_api::too_many(const char *who, uint64_t total) {
    return dcn_fail(DCN_ERR_ARG, std::string(who) + ": the range has " + std::to_string(total) + " events, 2^32 or more: ask for a part of it");
}

// What fetch and call share: the checks behind those of the parameters, the counts of the range (the INS plane, under rule
// L6 for a call), their scan and the scatter of the ledger's events into the buckets.  *n_slots = 0: nothing in the range.
int dcn_ledger_api::range_buckets(const dcn_index *map, const char *who, bool call, uint32_t record, uint64_t start, uint64_t n_bases, uint32_t min_depth,
                                  uint32_t min_permille, scratch &mem, dcn_ins_range_args *ra, uint64_t *n_slots) {
    *n_slots = 0;
    uint64_t b0 = 0;
    DCN_TRY(check_range(map, who, record, start, n_bases, &b0));
    const dcn_ins_ledger *l = map->ledger;
    memset(ra, 0, sizeof(*ra));
    if (n_bases == 0 || l->n_events == 0) return DCN_OK;
    DCN_HIP(hipSetDevice(map->device));
    ra->counters = map->d_pileup;
    ra->bases = map->pileup_bases;
    ra->t_packed = map->store->d_packed;
    ra->t_invmask = map->store->d_invmask;
    ra->base0 = b0;
    ra->n = n_bases;
    ra->pos0 = start;
    ra->min_depth = min_depth;
    ra->min_permille = min_permille;
    ra->events = l->d_events;
    ra->ledger_bases = l->d_bases;
    ra->n_events = l->n_events;
    DCN_TRY(mem.get(&ra->counts, n_bases, "insertion counts"));
    if (call) DCN_TRY(mem.get(&ra->flags, n_bases, "insertion flags"));
    DCN_TRY(dcn_launch_ins_plane(*ra, call, nullptr));
    uint64_t *d_offsets = nullptr, total = 0;
    DCN_TRY(scan_counts(mem, ra->counts, n_bases, &d_offsets, &total, "insertion bucket offsets"));
    ra->bucket_offsets = d_offsets;
    if (total == 0) return DCN_OK;
    if (total > UINT32_MAX) return too_many(who, total);
    DCN_TRY(mem.get(&ra->cursor, n_bases, "insertion cursors"));
    DCN_TRY(mem.get(&ra->slots, total, "insertion buckets"));
    DCN_HIP(hipMemset(ra->cursor, 0, n_bases * sizeof(uint32_t)));
    DCN_HIP(hipMemset(ra->slots, 0, total * sizeof(uint64_t))); // (every slot is written, by L2; event 0 exists)
    DCN_TRY(dcn_launch_ins_scatter(*ra, nullptr));
    ra->n_slots = total;
    *n_slots = total;
    return DCN_OK;
}

void dcn_ins_ledger_free(dcn_ins_ledger *l) {
    if (!l) return;
    for (void *p : {(void *)l->d_events, (void *)l->d_bases, (void *)l->d_row_events, (void *)l->d_row_bases, (void *)l->d_event_offsets,
                    (void *)l->d_base_offsets, (void *)l->d_event_sums, (void *)l->d_base_sums, (void *)l->d_totals})
        if (p) hipFree(p);
    delete l;
}

extern "C" int dcn_anchor_map_pileup_keep_insertions(dcn_index *map, int keep) {
    DCN_TRY(check_pileup(map));
    if (!keep) {
        if (map->ledger) {
            DCN_HIP(hipSetDevice(map->device));
            dcn_ins_ledger_free(map->ledger);
        }
        map->ledger = nullptr;
        return DCN_OK;
    }
    if (map->ledger) return DCN_OK;
    if (map->pileup_rows != 0) // rule L1
        return dcn_fail(DCN_ERR_ARG, std::to_string(map->pileup_rows) + " rows have added to the pileup since it was enabled or reset: a ledger "
                                                                         "begins with the counters (dcn_anchor_map_pileup_reset first)");
    DCN_HIP(hipSetDevice(map->device));
    dcn_ins_ledger *l = new (std::nothrow) dcn_ins_ledger();
    if (!l) return dcn_fail(DCN_ERR_NOMEM, "host allocation failed");
    const int rc = dev_alloc_zeroed(&l->d_totals, 2, "insertion totals");
    if (rc != DCN_OK) {
        delete l;
        return rc;
    }
    map->ledger = l;
    return DCN_OK;
}

int dcn_insertions_append(dcn_ctx *c, dcn_index *map, const dcn_pileup_args &rows) {
    dcn_ins_ledger *l = map->ledger;
    hipStream_t st = c->stream;
    const uint64_t n_work = rows.n_work;
    if (n_work == 0) return DCN_OK;
    if (l->rows_cap < n_work) {
        uint64_t c0 = 0, c1 = 0;
        l->rows_cap = 0;
        DCN_TRY(grow(&l->d_row_events, &c0, n_work, "insertion row events"));
        DCN_TRY(grow(&l->d_row_bases, &c1, n_work, "insertion row bases"));
        l->rows_cap = n_work;
    }
    dcn_ins_append_args aa;
    memset(&aa, 0, sizeof(aa));
    aa.rows = rows;
    aa.row_events = l->d_row_events;
    aa.row_bases = l->d_row_bases;
    aa.totals = l->d_totals;
    DCN_TRY(dcn_launch_ins_count(aa, st));
    unsigned long long totals[2] = {0, 0};
    DCN_HIP(hipMemcpyAsync(totals, l->d_totals, sizeof(totals), hipMemcpyDeviceToHost, st));
    DCN_HIP(hipStreamSynchronize(st));
    if (totals[0] == 0) return DCN_OK; // no I run in the batch: one pass and one read-back
    DCN_HIP(hipMemsetAsync(l->d_totals, 0, sizeof(totals), st)); // (zero between calls)
    if (n_work > UINT32_MAX) return dcn_fail(DCN_ERR_INTERNAL, "more than 2^32 - 1 aligned rows"); // (dcn_align_check_rows has refused them)
    if (l->offsets_cap < n_work + 1) { // the four arrays of the two scans, together
        uint64_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
        l->offsets_cap = 0;
        DCN_TRY(grow(&l->d_event_offsets, &c0, n_work + 1, "insertion event offsets"));
        DCN_TRY(grow(&l->d_base_offsets, &c1, n_work + 1, "insertion base offsets"));
        DCN_TRY(grow(&l->d_event_sums, &c2, n_work / DCN_SCAN_BLOCK + 2, "insertion scan sums"));
        DCN_TRY(grow(&l->d_base_sums, &c3, n_work / DCN_SCAN_BLOCK + 2, "insertion scan sums"));
        l->offsets_cap = n_work + 1;
    }
    DCN_TRY(dcn_launch_offsets_scan(l->d_row_events, (uint32_t)n_work, l->d_event_sums, l->d_event_offsets, st));
    DCN_TRY(dcn_launch_offsets_scan(l->d_row_bases, (uint32_t)n_work, l->d_base_sums, l->d_base_offsets, st));
    const uint64_t initial = ledger_initial_events();
    DCN_TRY(ledger_grow(&l->d_events, &l->event_cap, l->n_events, l->n_events + totals[0], initial, "insertion events", st));
    DCN_TRY(ledger_grow(&l->d_bases, &l->base_cap, l->n_bases, l->n_bases + totals[1], initial * DCN_LEDGER_BASES_PER_EVENT, "inserted bases", st));
    aa.event_offsets = l->d_event_offsets;
    aa.base_offsets = l->d_base_offsets;
    aa.events = l->d_events;
    aa.bases = l->d_bases;
    aa.event0 = l->n_events;
    aa.base0 = l->n_bases;
    DCN_TRY(dcn_launch_ins_write(aa, st));
    l->n_events += totals[0];
    l->n_bases += totals[1];
    return DCN_OK;
}

extern "C" int dcn_anchor_map_insertions_info(const dcn_index *map, uint64_t *n_events, uint64_t *n_bases) {
    DCN_TRY(check_ledger(map));
    if (n_events) *n_events = map->ledger->n_events;
    if (n_bases) *n_bases = map->ledger->n_bases;
    return DCN_OK;
}

extern "C" int dcn_anchor_map_insertions_fetch(const dcn_index *map, uint32_t record, uint64_t start, uint64_t n_bases, void *events,
                                               uint64_t event_capacity, uint8_t *bases, uint64_t base_capacity, uint64_t *n_events,
                                               uint64_t *n_inserted) {
    if (!n_events || !n_inserted) return dcn_fail(DCN_ERR_ARG, "n_events/n_inserted is NULL");
    DCN_TRY(check_ledger(map));
    *n_events = 0;
    *n_inserted = 0;
    scratch mem;
    dcn_ins_range_args ra;
    uint64_t n_slots = 0, n_ins = 0;
    DCN_TRY(range_buckets(map, "insertions fetch", false, record, start, n_bases, 0, 0, mem, &ra, &n_slots));
    *n_events = n_slots;
    if (n_slots == 0) return DCN_OK;
    uint64_t *d_slot_offsets = nullptr;
    DCN_TRY(mem.get(&ra.slot_lens, n_slots, "insertion lengths"));
    DCN_TRY(dcn_launch_ins_slot_lens(ra, nullptr));
    DCN_TRY(scan_counts(mem, ra.slot_lens, n_slots, &d_slot_offsets, &n_ins, "insertion base offsets"));
    ra.slot_offsets = d_slot_offsets;
    *n_inserted = n_ins;
    if (n_slots > event_capacity || n_ins > base_capacity) return capacity_error("events", n_slots, event_capacity, n_ins, base_capacity);
    if (!events || (n_ins > 0 && !bases)) return dcn_fail(DCN_ERR_ARG, "events/bases is NULL");
    dcn_insertion *d_out = nullptr;
    DCN_TRY(mem.get(&d_out, n_slots, "insertion events of the range"));
    DCN_TRY(mem.get(&ra.out_bases, n_ins, "inserted bases of the range"));
    ra.out_events = d_out;
    DCN_TRY(dcn_launch_ins_gather(ra, nullptr));
    std::vector<dcn_insertion> got(n_slots);
    std::vector<uint8_t> got_bases(std::max<uint64_t>(n_ins, 1));
    DCN_HIP(hipMemcpy(got.data(), d_out, n_slots * sizeof(dcn_insertion), hipMemcpyDeviceToHost));
    if (n_ins) DCN_HIP(hipMemcpy(got_bases.data(), ra.out_bases, n_ins, hipMemcpyDeviceToHost));
    // rule L4: the buckets are in ascending position; inside one the order is the scatter's, so each is sorted here
    std::sort(got.begin(), got.end(), [&](const dcn_insertion &a, const dcn_insertion &b) {
        if (a.pos != b.pos) return a.pos < b.pos;
        const uint32_t fa = a.flags & DCN_INSERTION_FRONT, fb = b.flags & DCN_INSERTION_FRONT;
        if (fa != fb) return fa < fb;
        if (a.len != b.len) return a.len < b.len;
        const int c = memcmp(got_bases.data() + a.bases_offset, got_bases.data() + b.bases_offset, a.len);
        if (c != 0) return c < 0;
        return (a.flags & DCN_INSERTION_REVERSE) < (b.flags & DCN_INSERTION_REVERSE);
    });
    dcn_insertion *out = static_cast<dcn_insertion *>(events);
    uint64_t at = 0;
    for (uint64_t s = 0; s < n_slots; ++s) {
        out[s] = got[s];
        out[s].bases_offset = at;
        memcpy(bases + at, got_bases.data() + got[s].bases_offset, got[s].len);
        at += got[s].len;
    }
    return DCN_OK;
}

extern "C" int dcn_anchor_map_insertions_call(const dcn_index *map, const void *params, uint32_t record, uint64_t start, uint64_t n_bases,
                                              void *alleles, uint64_t allele_capacity, uint8_t *bases, uint64_t base_capacity,
                                              uint64_t *n_alleles, uint64_t *n_inserted) {
    const dcn_pileup_call_params *prm = static_cast<const dcn_pileup_call_params *>(params);
    if (!prm) return dcn_fail(DCN_ERR_ARG, "params is NULL");
    if (prm->reserved[0] != 0 || prm->reserved[1] != 0) return dcn_fail(DCN_ERR_ARG, "params.reserved must be 0");
    if (prm->min_permille > 1000) return dcn_fail(DCN_ERR_ARG, "params.min_permille must be 0..1000");
    if (!n_alleles || !n_inserted) return dcn_fail(DCN_ERR_ARG, "n_alleles/n_inserted is NULL");
    DCN_TRY(check_ledger(map));
    *n_alleles = 0;
    *n_inserted = 0;
    scratch mem;
    dcn_ins_range_args ra;
    uint64_t n_slots = 0, n_all = 0, n_ins = 0;
    DCN_TRY(range_buckets(map, "insertions call", true, record, start, n_bases, prm->min_depth, prm->min_permille, mem, &ra, &n_slots));
    if (n_slots == 0) return DCN_OK;
    uint64_t *d_allele_offsets = nullptr, *d_win_offsets = nullptr;
    DCN_TRY(scan_counts(mem, ra.flags, n_bases, &d_allele_offsets, &n_all, "insertion allele offsets"));
    ra.allele_offsets = d_allele_offsets;
    ra.n_alleles = n_all;
    DCN_TRY(mem.get(&ra.win_event, n_all, "insertion winners"));
    DCN_TRY(mem.get(&ra.win_count, n_all, "insertion winner counts"));
    DCN_TRY(mem.get(&ra.win_events, n_all, "insertion winner events"));
    DCN_TRY(mem.get(&ra.win_len, n_all, "insertion winner lengths"));
    DCN_TRY(mem.get(&ra.win_pos, n_all, "insertion winner positions"));
    DCN_HIP(hipMemset(ra.win_event, 0, n_all * sizeof(uint64_t)));
    DCN_HIP(hipMemset(ra.win_len, 0, n_all * sizeof(uint32_t)));
    DCN_TRY(dcn_launch_ins_winner(ra, nullptr));
    DCN_TRY(scan_counts(mem, ra.win_len, n_all, &d_win_offsets, &n_ins, "insertion allele base offsets"));
    ra.win_offsets = d_win_offsets;
    *n_alleles = n_all;
    *n_inserted = n_ins;
    if (n_all > allele_capacity || n_ins > base_capacity) return capacity_error("alleles", n_all, allele_capacity, n_ins, base_capacity);
    if (!alleles || (n_ins > 0 && !bases)) return dcn_fail(DCN_ERR_ARG, "alleles/bases is NULL");
    dcn_insertion_allele *d_out = nullptr;
    DCN_TRY(mem.get(&d_out, n_all, "insertion alleles of the range"));
    DCN_TRY(mem.get(&ra.out_bases, n_ins, "inserted bases of the range"));
    ra.out_alleles = d_out;
    DCN_TRY(dcn_launch_ins_alleles(ra, nullptr));
    DCN_HIP(hipMemcpy(alleles, d_out, n_all * sizeof(dcn_insertion_allele), hipMemcpyDeviceToHost));
    if (n_ins) DCN_HIP(hipMemcpy(bases, ra.out_bases, n_ins, hipMemcpyDeviceToHost));
    return DCN_OK;
}

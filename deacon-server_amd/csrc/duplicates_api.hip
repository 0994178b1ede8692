// duplicates_api.hip -- the C ABI of duplicate marking (dcn_anchor_map_duplicates_enable / _reset / _info,
// dcn_mark_duplicates_batch; kernels in duplicates.hip, the arithmetic of rules D3 and D4 in dcn_duplicates.h).  The checks
// of the rows are dcn_verify_batch's (rows_stride_check, rows_shape_check and rows_walk of dcn_verify.h, in its order and
// with its messages), without a context: the call takes no bases.  While it checks the rows the walk picks the first placed
// row of every read, so that what crosses the link is 40 bytes per read whatever the rows' stride and number.  Host
// pointers, blocking, on the null stream, as dcn_anchor_map_genotype.
#include "dcn_ctx.h"
#include "dcn_duplicates.h"
#include "dcn_verify.h"

#include <cstdlib>
#include <cstring>

using namespace dcn_impl;

static_assert(sizeof(dcn_duplicate_params) == 16, "duplicate params are ABI");

namespace {
constexpr uint64_t DUP_INITIAL_SLOTS = 1ull << 20;
constexpr uint64_t DUP_INITIAL_LOG = 1ull << 16;

int check_map(const dcn_index *map) {
    if (!map) return dcn_fail(DCN_ERR_ARG, "map is NULL");
    if (!map->d_anchor) return dcn_fail(DCN_ERR_ARG, "the index is not an anchor map (dcn_anchor_map_create)");
    return DCN_OK;
}

int check_dup_set(const dcn_index *map) {
    DCN_TRY(check_map(map));
    if (!map->dups) return dcn_fail(DCN_ERR_ARG, "the map keeps no duplicate set (dcn_anchor_map_duplicates_enable)");
    return DCN_OK;
}

uint64_t pow2_at_least(uint64_t v) {
    uint64_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

// slots the table starts with: DUP_INITIAL_SLOTS, or the test hook DCN_DUPLICATE_TABLE_SLOTS, read when the set first grows
uint64_t initial_slots() {
    const char *s = std::getenv("DCN_DUPLICATE_TABLE_SLOTS");
    const uint64_t v = s && *s ? std::strtoull(s, nullptr, 10) : DUP_INITIAL_SLOTS;
    return pow2_at_least(std::min<uint64_t>(std::max<uint64_t>(v, 2), 1ull << 40));
}

// the log holds `need` keys: geometric, the keys so far copied over
int log_reserve(dcn_dup_set *d, uint64_t need) {
    if (need <= d->log_cap) return DCN_OK;
    const uint64_t cap = std::max<uint64_t>(std::max<uint64_t>(need, 2 * d->log_cap), DUP_INITIAL_LOG);
    dcn_dup_key *p = nullptr;
    DCN_TRY(dev_alloc(&p, cap, "duplicate key log"));
    hipError_t e = d->seen ? hipMemcpy(p, d->d_log, d->seen * sizeof(dcn_dup_key), hipMemcpyDeviceToDevice) : hipSuccess;
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        hipFree(p);
        return dcn_hip_fail(e, "duplicate key log");
    }
    if (d->d_log) hipFree(d->d_log);
    d->d_log = p;
    d->log_cap = cap;
    return DCN_OK;
}

// the table has at least `need` slots: a new table, at least twice the old one, and the old one's ordinals rehashed into it
int table_reserve(dcn_dup_set *d, uint64_t need) {
    if (d->d_slots && need <= d->n_slots) return DCN_OK;
    const uint64_t n = std::max<uint64_t>(pow2_at_least(need), d->d_slots ? 2 * d->n_slots : initial_slots());
    unsigned long long *p = nullptr;
    DCN_TRY(dev_alloc(&p, n, "duplicate table"));
    hipError_t e = hipMemset(p, 0xFF, n * sizeof(unsigned long long)); // DCN_DUP_EMPTY
    int rc = DCN_OK;
    if (e == hipSuccess && d->d_slots && d->keys) {
        dcn_dup_args ra;
        memset(&ra, 0, sizeof(ra));
        ra.log = d->d_log;
        ra.slots = p;
        ra.mask = n - 1;
        rc = dcn_launch_dup_rehash(ra, d->d_slots, d->n_slots, nullptr);
    }
    if (e == hipSuccess && rc == DCN_OK) e = hipDeviceSynchronize();
    if (e != hipSuccess || rc != DCN_OK) {
        hipFree(p);
        return rc != DCN_OK ? rc : dcn_hip_fail(e, "duplicate table");
    }
    if (d->d_slots) hipFree(d->d_slots);
    d->d_slots = p;
    d->n_slots = n;
    return DCN_OK;
}
} // namespace

void dcn_dup_set_free(dcn_dup_set *d) {
    if (!d) return;
    if (d->d_log) hipFree(d->d_log);
    if (d->d_slots) hipFree(d->d_slots);
    if (d->d_items) hipFree(d->d_items);
    if (d->d_dup) hipFree(d->d_dup);
    if (d->d_first) hipFree(d->d_first);
    if (d->d_n_dup) hipFree(d->d_n_dup);
    delete d;
}

extern "C" int dcn_anchor_map_duplicates_enable(dcn_index *map, int enable) {
    DCN_TRY(check_map(map));
    if (!enable) {
        if (map->dups) {
            DCN_HIP(hipSetDevice(map->device));
            dcn_dup_set_free(map->dups);
            map->dups = nullptr;
        }
        return DCN_OK;
    }
    if (map->dups) return DCN_OK;
    map->dups = new (std::nothrow) dcn_dup_set();
    if (!map->dups) return dcn_fail(DCN_ERR_NOMEM, "host allocation failed");
    return DCN_OK; // (no device memory until the first call hands units in)
}

extern "C" int dcn_anchor_map_duplicates_reset(dcn_index *map) {
    DCN_TRY(check_dup_set(map));
    dcn_dup_set *d = map->dups;
    if (d->d_slots) {
        DCN_HIP(hipSetDevice(map->device));
        DCN_HIP(hipMemset(d->d_slots, 0xFF, d->n_slots * sizeof(unsigned long long)));
        DCN_HIP(hipDeviceSynchronize());
    }
    d->seen = d->keyed = d->keys = 0;
    return DCN_OK;
}

extern "C" int dcn_anchor_map_duplicates_info(const dcn_index *map, uint64_t *seen, uint64_t *keyed, uint64_t *keys) {
    DCN_TRY(check_dup_set(map));
    if (seen) *seen = map->dups->seen;
    if (keyed) *keyed = map->dups->keyed;
    if (keys) *keys = map->dups->keys;
    return DCN_OK;
}

extern "C" int dcn_mark_duplicates_batch(dcn_index *map, const uint64_t *offsets, uint32_t n_reads, const void *params,
                                         const uint64_t *row_offsets, const void *rows, uint64_t n_rows, uint8_t *dup, uint64_t *first,
                                         uint64_t *n_duplicates) {
    const dcn_duplicate_params *prm = static_cast<const dcn_duplicate_params *>(params);
    if (!prm) return dcn_fail(DCN_ERR_ARG, "params is NULL");
    if (prm->reserved != 0) return dcn_fail(DCN_ERR_ARG, "params.reserved must be 0");
    if (prm->paired > 1) return dcn_fail(DCN_ERR_ARG, "params.paired must be 0 or 1");
    if (prm->both_ends > 1) return dcn_fail(DCN_ERR_ARG, "params.both_ends must be 0 or 1");
    DCN_TRY(rows_stride_check(prm->row_stride));
    DCN_TRY(check_dup_set(map));
    if (prm->paired && n_reads % 2 != 0) return dcn_fail(DCN_ERR_ARG, "in paired mode unit u is reads 2u and 2u + 1: n_reads must be even");
    const dcn_row_call call = {nullptr, map, nullptr, offsets, n_reads, 0, 0, prm->row_stride, row_offsets, rows, n_rows};
    bool run = false;
    uint64_t n_bases = 0;
    DCN_TRY(rows_shape_check(call, &run, &n_bases));
    if (n_reads == 0) {
        if (n_duplicates) *n_duplicates = 0;
        return DCN_OK;
    }

    // the walk: every placed row checked, the first of each read kept (rows come read by read, so `row` only ascends)
    std::vector<dcn_dup_item> items(n_reads);
    for (dcn_dup_item &it : items) {
        memset(&it, 0, sizeof(it));
        it.record = DCN_DUP_NO_RECORD;
    }
    if (run) {
        uint32_t r = 0;
        const int rc = rows_walk(call, [&](uint64_t row, const dcn_placement &p, uint64_t, uint64_t read_len, uint64_t, uint64_t) {
            if (p.record == UINT32_MAX) return;
            if (row_offsets)
                while (row >= row_offsets[r + 1]) ++r;
            else r = (uint32_t)row;
            dcn_dup_item &it = items[r];
            if (it.record != DCN_DUP_NO_RECORD) return;
            it.record = p.record;
            it.reverse = p.reverse;
            it.read_start = p.read_start;
            it.read_end = p.read_end;
            it.read_len = (uint32_t)read_len;
            it.ref_start = p.ref_start;
            it.ref_end = p.ref_end;
        });
        DCN_TRY(rc);
    }
    const uint32_t per = prm->paired ? 2 : 1;
    const uint64_t n_units = n_reads / per;
    uint64_t keyed = 0;
    for (uint64_t u = 0; u < n_units; ++u)
        keyed += items[per * u].record != DCN_DUP_NO_RECORD || (per == 2 && items[2 * u + 1].record != DCN_DUP_NO_RECORD);

    // nothing of the set has changed so far; from here only a device failure ends the call early
    dcn_dup_set *d = map->dups;
    DCN_HIP(hipSetDevice(map->device));
    DCN_TRY(log_reserve(d, d->seen + n_units));
    DCN_TRY(table_reserve(d, 2 * (d->keys + n_units))); // (an upper bound on the keys behind this call: no read-back first)
    DCN_TRY(grow(&d->d_items, &d->items_cap, n_reads, "duplicate items"));
    DCN_TRY(grow(&d->d_dup, &d->dup_cap, n_units, "duplicate flags"));
    DCN_TRY(grow(&d->d_first, &d->first_cap, n_units, "duplicate firsts"));
    if (!d->d_n_dup) DCN_TRY(dev_alloc(&d->d_n_dup, 1, "duplicate count"));
    DCN_HIP(hipMemcpy(d->d_items, items.data(), (uint64_t)n_reads * sizeof(dcn_dup_item), hipMemcpyHostToDevice));
    DCN_HIP(hipMemset(d->d_n_dup, 0, sizeof(unsigned long long)));
    dcn_dup_args a;
    memset(&a, 0, sizeof(a));
    a.items = d->d_items;
    a.n_units = n_units;
    a.ord0 = d->seen;
    a.paired = prm->paired;
    a.both_ends = prm->both_ends;
    a.log = d->d_log;
    a.slots = d->d_slots;
    a.mask = d->n_slots - 1;
    a.dup = d->d_dup;
    a.first = d->d_first;
    a.n_dup = d->d_n_dup;
    DCN_TRY(dcn_launch_dup_keys(a, nullptr));
    DCN_TRY(dcn_launch_dup_insert(a, nullptr));
    DCN_TRY(dcn_launch_dup_lookup(a, nullptr));
    unsigned long long n_dup = 0;
    DCN_HIP(hipMemcpy(&n_dup, d->d_n_dup, sizeof(n_dup), hipMemcpyDeviceToHost));
    if (dup) DCN_HIP(hipMemcpy(dup, d->d_dup, n_units, hipMemcpyDeviceToHost));
    if (first) DCN_HIP(hipMemcpy(first, d->d_first, n_units * sizeof(uint64_t), hipMemcpyDeviceToHost));
    d->seen += n_units;
    d->keyed += keyed;
    d->keys += keyed - n_dup;
    if (n_duplicates) *n_duplicates = n_dup;
    return DCN_OK;
}

// place_api.hip -- the C ABI of anchor maps (dcn_anchor_map_*), dcn_place_batch, dcn_place_split_batch and
// dcn_place_pair_batch (kernels in place.hip, place_vote.hip, place_split.hip and place_pair.hip; the batch calls run the
// dump front end of ctx.hip on a filter context).
#include "dcn_ctx.h"
#include "dcn_place.h"
#include "dcn_verify.h"

#include <cstdlib>
#include <cstring>
#include <type_traits>

using namespace dcn_impl;

static_assert(sizeof(dcn_place_params) == 24 && sizeof(dcn_placement) == 48, "place structs are ABI");
static_assert(sizeof(dcn_place_split_params) == 32 && sizeof(dcn_split_placement) == 64 && sizeof(dcn_split_round) == 32,
              "split place structs are ABI");
static_assert(sizeof(dcn_place_pair_params) == 40 && sizeof(dcn_pair_placement) == 80, "pair place structs are ABI");

namespace {
int check_map(const dcn_index *map) {
    if (!map) return dcn_fail(DCN_ERR_ARG, "map is NULL");
    if (!map->d_anchor) return dcn_fail(DCN_ERR_ARG, "the index is not an anchor map (dcn_anchor_map_create)");
    return DCN_OK;
}

// a test hook of the vote: `name` as a number within [lo, hi], else `dflt`
uint32_t env_u32(const char *name, uint32_t dflt, uint32_t lo, uint32_t hi) {
    const char *s = std::getenv(name);
    if (!s || !*s) return dflt;
    const unsigned long long v = std::strtoull(s, nullptr, 10);
    return (uint32_t)std::min<unsigned long long>(std::max<unsigned long long>(v, lo), hi);
}

// the dump front end over a staged batch, and the fields of `pa` that both sweeps read
int front_end(dcn_ctx *c, const dcn_index *map, uint32_t n_reads, uint64_t n_bases, uint64_t prefix_length, int *prof_slot,
              dcn_place_args *pa) {
    memset(pa, 0, sizeof(*pa));
    DCN_TRY(dump_front_end(c, map, c->d_ascii, c->d_offsets, nullptr, n_reads, n_reads, n_bases, prefix_length, false, prof_slot,
                           &pa->dump));
    pa->table = map->view();
    pa->anchor = map->d_anchor;
    pa->n_slots = map->n_groups * DCN_GROUP_SLOTS;
    pa->k = map->k;
    pa->packed = c->d_packed + DCN_FRONT_PAD;
    pa->status = c->d_status;
    pa->offsets = c->d_offsets;
    pa->n_reads = n_reads;
    return DCN_OK;
}

// ---- what dcn_place_batch, dcn_place_split_batch and dcn_place_pair_batch share --------------------------------------
// the parameters every placement call has (max_placements: the split and the pair call)
template <typename P>
int check_vote_params(const P *prm) {
    if (!prm) return dcn_fail(DCN_ERR_ARG, "params is NULL");
    for (const uint32_t v : prm->reserved)
        if (v != 0) return dcn_fail(DCN_ERR_ARG, "params.reserved must be 0");
    if (prm->band_bases == 0) return dcn_fail(DCN_ERR_ARG, "params.band_bases must be at least 1");
    if (prm->min_votes == 0) return dcn_fail(DCN_ERR_ARG, "params.min_votes must be at least 1");
    if constexpr (!std::is_same_v<P, dcn_place_params>)
        if (prm->max_placements == 0 || prm->max_placements > DCN_PLACE_SPLIT_MAX)
            return dcn_fail(DCN_ERR_ARG, "params.max_placements must be 1.." + std::to_string(DCN_PLACE_SPLIT_MAX));
    return DCN_OK;
}

int check_target(const dcn_ctx *ctx, const dcn_index *map) {
    if (!ctx) return dcn_fail(DCN_ERR_ARG, "ctx is NULL");
    DCN_TRY(check_map(map));
    return check_ctx_matches(ctx, map, "the map");
}

// a batch of n_reads > 0 reads; `out_is_null` names the output the call cannot do without (null: it has it)
int check_batch(const dcn_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads, const char *out_is_null,
                uint64_t *n_bases) {
    if (!offsets) return dcn_fail(DCN_ERR_ARG, "offsets is NULL");
    if (out_is_null) return dcn_fail(DCN_ERR_ARG, out_is_null);
    DCN_TRY(validate_host_batch(ctx, offsets, n_reads)); // (a read of 2^32 bases or more is refused here)
    *n_bases = offsets[n_reads];
    if (*n_bases > 0 && !bases) return dcn_fail(DCN_ERR_ARG, "bases is NULL");
    return DCN_OK;
}

// a buffer of the context that grows to the largest need so far
template <typename T>
int grow(T **buf, uint64_t *cap, uint64_t need, const char *what) {
    if (need <= *cap) return DCN_OK;
    if (*buf) hipFree(*buf);
    *buf = nullptr;
    *cap = 0;
    DCN_TRY(dev_alloc(buf, need, what));
    *cap = need;
    return DCN_OK;
}

// which buffers a call needs beside those of the mark sweep and the work list
enum place_mode {
    PLACE_SINGLE, // the placements; no remaining-hits bitmap, rounds or counts
    PLACE_SPLIT,  // the rounds' buffers and the CSR tail's
    PLACE_PAIR,   // the rounds' buffers
};

// What the three calls do before the vote: the buffers of the context (allocated when a call first needs them), the
// staged batch, the dump front end, the mark sweep (DISTINCT ends behind it) and, for the rounds, the copy of the anchor
// bitmap that they clear.  `sa` is ready for dcn_launch_place_vote (sa.p) / dcn_launch_place_split_rounds / _rows.
template <typename P>
int place_prepare(dcn_ctx *c, const dcn_index *map, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                  uint64_t n_bases, const P *prm, place_mode mode, int *prof_slot_out, dcn_place_split_args *sa_out) {
    uint32_t N = 0;
    if constexpr (!std::is_same_v<P, dcn_place_params>) N = prm->max_placements;
    DCN_HIP(hipSetDevice(c->device));
    DCN_TRY(ensure_dump_buffers(c));
    DCN_TRY(ensure_position_bitmap(c));
    const uint64_t bitmap_words = (c->max_bases + 31) / 32 + 1;
    if (!c->d_plc_abits) DCN_TRY(dev_alloc(&c->d_plc_abits, bitmap_words, "anchor bitmap"));
    if (!c->d_plc_words) DCN_TRY(dev_alloc(&c->d_plc_words, c->max_bases + 2, "placement words"));
    if (!c->d_plc_big) DCN_TRY(dev_alloc(&c->d_plc_big, c->max_reads, "placement work list"));
    if (!c->d_plc_n_big) DCN_TRY(dev_alloc(&c->d_plc_n_big, 1, "placement work list length"));
    if (mode == PLACE_SINGLE) {
        if (!c->d_plc_out) DCN_TRY(dev_alloc(&c->d_plc_out, c->max_reads, "placements"));
    } else {
        if (!c->d_pls_rbits) DCN_TRY(dev_alloc(&c->d_pls_rbits, bitmap_words, "remaining anchor bitmap"));
        if (!c->d_pls_n_rounds) DCN_TRY(dev_alloc(&c->d_pls_n_rounds, c->max_reads, "placement round counts"));
        if (!c->d_pls_read_counts) DCN_TRY(dev_alloc(&c->d_pls_read_counts, (uint64_t)c->max_reads * 2, "placement read counts"));
        if (!c->d_pls_counts) DCN_TRY(dev_alloc(&c->d_pls_counts, c->max_reads, "placement counts"));
        if (mode == PLACE_SPLIT) {
            if (!c->d_pls_block_sums)
                DCN_TRY(dev_alloc(&c->d_pls_block_sums, (uint64_t)c->max_reads / DCN_SCAN_BLOCK + 1, "placement block sums"));
            if (!c->d_pls_offsets) DCN_TRY(dev_alloc(&c->d_pls_offsets, (uint64_t)c->max_reads + 1, "placement offsets"));
        }
        DCN_TRY(grow(&c->d_pls_rounds, &c->pls_round_cap, (uint64_t)n_reads * (N + 1), "placement rounds"));
        if (mode == PLACE_SPLIT) DCN_TRY(grow(&c->d_pls_out, &c->pls_out_cap, (uint64_t)n_reads * N, "split placements"));
    }
    DCN_TRY(stage_batch(c, bases, n_bases, offsets, n_reads, nullptr));
    hipStream_t st = c->stream;
    const uint64_t batch_words = (n_bases + 31) / 32 + 1;
    DCN_HIP(hipMemsetAsync(c->d_status, 0, sizeof(dcn_status), st));
    DCN_HIP(hipMemsetAsync(c->d_loc_bits, 0, batch_words * sizeof(uint32_t), st));
    DCN_HIP(hipMemsetAsync(c->d_plc_abits, 0, batch_words * sizeof(uint32_t), st));
    DCN_HIP(hipMemsetAsync(c->d_plc_n_big, 0, sizeof(uint32_t), st));
    int prof_slot = -1;
    dcn_place_split_args &sa = *sa_out;
    memset(&sa, 0, sizeof(sa));
    dcn_place_args &pa = sa.p;
    DCN_TRY(front_end(c, map, n_reads, n_bases, prm->prefix_length, &prof_slot, &pa));
    *prof_slot_out = prof_slot;
    pa.band = prm->band_bases;
    pa.min_votes = prm->min_votes;
    pa.lane_bases = env_u32("DCN_PLACE_LANE_BASES", DCN_PLC_LANE_BASES, 0, 0xFFFFFFFFu);
    pa.lds_cells = env_u32("DCN_PLACE_LDS_CELLS", DCN_PLC_LDS_CELLS, DCN_PLC_LDS_CELLS_MIN, DCN_PLC_LDS_CELLS);
    // (the offsets are the host's: whether any read takes the workgroup path is known before the launch)
    for (uint32_t r = 0; r < n_reads && !pa.any_big; ++r) pa.any_big = offsets[r + 1] - offsets[r] > pa.lane_bases ? 1u : 0u;
    pa.bits = c->d_loc_bits;
    pa.abits = c->d_plc_abits;
    pa.words = c->d_plc_words;
    pa.big = c->d_plc_big;
    pa.n_big = c->d_plc_n_big;
    pa.out = c->d_plc_out; // (null unless dcn_place_batch ran on the context; only its vote writes it)
    sa.rbits = c->d_pls_rbits;
    sa.max_placements = N;
    sa.rounds = c->d_pls_rounds;
    sa.n_rounds = c->d_pls_n_rounds;
    sa.read_counts = c->d_pls_read_counts;
    sa.counts = c->d_pls_counts;
    sa.block_sums = c->d_pls_block_sums;
    sa.place_offsets = c->d_pls_offsets;
    sa.out = c->d_pls_out;
    DCN_TRY(dcn_launch_place_mark(pa, st));
    DCN_PROF_MARK(DCN_STAGE_DISTINCT);
    if (mode != PLACE_SINGLE)
        DCN_HIP(hipMemcpyAsync(c->d_pls_rbits, c->d_plc_abits, batch_words * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    return DCN_OK;
}
} // namespace

extern "C" int dcn_anchor_map_create(const dcn_index *index, dcn_index **out) {
    if (!out) return dcn_fail(DCN_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!index) return dcn_fail(DCN_ERR_ARG, "index is NULL");
    dcn_index *map = nullptr;
    DCN_TRY(dcn_index_clone(index, index->device, &map)); // (a plain index over the keys, on the same device)
    const uint64_t words = map->n_groups * DCN_GROUP_SLOTS + 1;
    const hipError_t e = hipSetDevice(map->device);
    const int rc = e == hipSuccess ? dev_alloc_zeroed(&map->d_anchor, words, "anchor words") : dcn_hip_fail(e, "anchor words");
    if (rc != DCN_OK) {
        dcn_index_destroy(map);
        return rc;
    }
    map->anchor_records = 0;
    *out = map;
    return DCN_OK;
}

extern "C" int dcn_anchor_map_add(dcn_index *map, dcn_ctx *ctx, const uint8_t *bases, const uint64_t *offsets,
                                  uint32_t n_records, uint32_t *first_record) {
    DCN_TRY(check_map(map));
    if (map->d_pileup)
        return dcn_fail(DCN_ERR_ARG, "the map has a pileup, which covers the records added before it was enabled and does not grow: "
                                     "dcn_anchor_map_pileup_enable(map, 0) first");
    if (!ctx) return dcn_fail(DCN_ERR_ARG, "ctx is NULL");
    DCN_TRY(check_ctx_matches(ctx, map, "the map"));
    if (first_record) *first_record = map->anchor_records;
    if (n_records == 0) return DCN_OK;
    if (!offsets) return dcn_fail(DCN_ERR_ARG, "offsets is NULL");
    if ((uint64_t)map->anchor_records + n_records > DCN_ANCHOR_MAX_RECORDS)
        return dcn_fail(DCN_ERR_ARG, "an anchor map holds at most 2^31 - 1 records");
    DCN_TRY(validate_host_batch(ctx, offsets, n_records));
    for (uint32_t r = 0; r < n_records; ++r)
        if (offsets[r + 1] - offsets[r] > DCN_ANCHOR_MAX_RECORD_BASES)
            return dcn_fail(DCN_ERR_ARG, "a record of an anchor map has at most 2^32 - 1 bases");
    const uint64_t n_bases = offsets[n_records];
    if (n_bases > 0 && !bases) return dcn_fail(DCN_ERR_ARG, "bases is NULL");
    dcn_ctx *c = ctx;
    DCN_HIP(hipSetDevice(c->device));
    DCN_TRY(ensure_dump_buffers(c));
    DCN_TRY(stage_batch(c, bases, n_bases, offsets, n_records, nullptr));
    hipStream_t st = c->stream;
    DCN_HIP(hipMemsetAsync(c->d_status, 0, sizeof(dcn_status), st));
    int prof_slot = -1;
    dcn_place_args pa;
    DCN_TRY(front_end(c, map, n_records, n_bases, 0, &prof_slot, &pa));
    pa.first_record = map->anchor_records;
    DCN_TRY(dcn_launch_anchor_add(pa, st));
    DCN_PROF_MARK(DCN_STAGE_DISTINCT);
    // kept bases: the front end's packed stream and mask go behind what the store holds, whole words
    uint64_t store_start = 0;
    if (map->store)
        DCN_TRY(dcn_base_store_append(map->store, c->d_packed + DCN_FRONT_PAD, c->d_invmask + DCN_FRONT_PAD, n_bases, st, &store_start));
    DCN_PROF_MARK(DCN_STAGE_FINISH);
    DCN_TRY(finish_run(c, prof_slot));
    if (map->store) dcn_base_store_commit(map->store, store_start, offsets, n_records);
    map->anchor_records += n_records;
    return DCN_OK;
}

extern "C" int dcn_anchor_map_info(const dcn_index *map, uint32_t *n_records, uint64_t *n_keys, uint64_t *n_anchors,
                                   uint64_t *n_repeats) {
    DCN_TRY(check_map(map));
    DCN_HIP(hipSetDevice(map->device));
    unsigned long long h[2] = {};
    if (n_anchors || n_repeats)
        DCN_TRY(dcn_device_tally(2, h, "anchor map info", [&](unsigned long long *d) { return dcn_anchor_tally(map, d, 0); }));
    if (n_records) *n_records = map->anchor_records;
    if (n_keys) *n_keys = map->n_keys;
    if (n_anchors) *n_anchors = h[0];
    if (n_repeats) *n_repeats = h[1];
    return DCN_OK;
}

extern "C" int dcn_anchor_map_anchors(const dcn_index *map, uint64_t *keys, uint32_t *records, uint32_t *positions,
                                      uint64_t capacity, uint64_t *n) {
    DCN_TRY(check_map(map));
    if (!n) return dcn_fail(DCN_ERR_ARG, "n is NULL");
    *n = 0;
    if ((!keys || !records || !positions) && capacity > 0) return dcn_fail(DCN_ERR_ARG, "keys/records/positions is NULL");
    DCN_HIP(hipSetDevice(map->device));
    unsigned long long h[2] = {};
    DCN_TRY(dcn_device_tally(2, h, "anchors", [&](unsigned long long *d) { return dcn_anchor_tally(map, d, 0); }));
    const uint64_t total = h[0];
    *n = total;
    if (total > capacity)
        return dcn_fail(DCN_ERR_CAPACITY, "anchors: " + std::to_string(total) + " anchors, capacity " + std::to_string(capacity));
    if (total == 0) return DCN_OK;
    const char *what = "anchors";
    DevMem d_n, d_keys, d_rec, d_pos;
    DCN_TRY(d_n.alloc(sizeof(unsigned long long), true, what));
    DCN_TRY(d_keys.alloc(total * sizeof(uint64_t), false, what));
    DCN_TRY(d_rec.alloc(total * sizeof(uint32_t), false, what));
    DCN_TRY(d_pos.alloc(total * sizeof(uint32_t), false, what));
    DCN_TRY(dcn_anchor_export(map, d_keys.as<uint64_t>(), d_rec.as<uint32_t>(), d_pos.as<uint32_t>(), total,
                              d_n.as<unsigned long long>(), 0));
    unsigned long long written = 0;
    DCN_TRY(read_count(d_n, what, &written));
    if (written != total)
        return dcn_fail(DCN_ERR_INTERNAL, "anchors: the map changed between the count and the copy (an add call in flight?)");
    DCN_TRY(d_keys.read(keys, total * sizeof(uint64_t), what));
    DCN_TRY(d_rec.read(records, total * sizeof(uint32_t), what));
    return d_pos.read(positions, total * sizeof(uint32_t), what);
}

extern "C" int dcn_place_batch(dcn_ctx *ctx, const dcn_index *map, const uint8_t *bases, const uint64_t *offsets,
                               uint32_t n_reads, const void *params, void *placements) {
    const dcn_place_params *prm = static_cast<const dcn_place_params *>(params);
    // (the parameters first: what is wrong with them does not depend on the context or the map)
    DCN_TRY(check_vote_params(prm));
    DCN_TRY(check_target(ctx, map));
    if (n_reads == 0) return DCN_OK;
    uint64_t n_bases = 0;
    DCN_TRY(check_batch(ctx, bases, offsets, n_reads, placements ? nullptr : "placements is NULL", &n_bases));
    dcn_ctx *c = ctx;
    int prof_slot = -1;
    dcn_place_split_args sa;
    DCN_TRY(place_prepare(c, map, bases, offsets, n_reads, n_bases, prm, PLACE_SINGLE, &prof_slot, &sa));
    hipStream_t st = c->stream;
    DCN_TRY(dcn_launch_place_vote(sa.p, st));
    DCN_PROF_MARK(DCN_STAGE_FINISH);
    DCN_TRY(finish_run(c, prof_slot));
    DCN_HIP(hipMemcpy(placements, c->d_plc_out, (uint64_t)n_reads * sizeof(dcn_placement), hipMemcpyDeviceToHost));
    return DCN_OK;
}

extern "C" int dcn_place_split_batch(dcn_ctx *ctx, const dcn_index *map, const uint8_t *bases, const uint64_t *offsets,
                                     uint32_t n_reads, const void *params, uint64_t *place_offsets, void *placements,
                                     uint64_t capacity, uint32_t *read_counts) {
    const dcn_place_split_params *prm = static_cast<const dcn_place_split_params *>(params);
    DCN_TRY(check_vote_params(prm));
    if (!place_offsets) return dcn_fail(DCN_ERR_ARG, "place_offsets is NULL");
    DCN_TRY(check_target(ctx, map));
    place_offsets[0] = 0;
    if (n_reads == 0) return DCN_OK;
    uint64_t n_bases = 0;
    DCN_TRY(check_batch(ctx, bases, offsets, n_reads, !placements && capacity > 0 ? "placements is NULL" : nullptr, &n_bases));
    dcn_ctx *c = ctx;
    int prof_slot = -1;
    dcn_place_split_args sa;
    DCN_TRY(place_prepare(c, map, bases, offsets, n_reads, n_bases, prm, PLACE_SPLIT, &prof_slot, &sa));
    hipStream_t st = c->stream;
    DCN_TRY(dcn_launch_place_split_vote(sa, st));
    DCN_PROF_MARK(DCN_STAGE_FINISH);
    DCN_TRY(finish_run(c, prof_slot));
    DCN_HIP(hipMemcpy(place_offsets, c->d_pls_offsets, ((uint64_t)n_reads + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (read_counts)
        DCN_HIP(hipMemcpy(read_counts, c->d_pls_read_counts, (uint64_t)n_reads * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    const uint64_t total = place_offsets[n_reads];
    if (total > capacity)
        return dcn_fail(DCN_ERR_CAPACITY,
                        "place split: " + std::to_string(total) + " placements, capacity " + std::to_string(capacity));
    if (total) DCN_HIP(hipMemcpy(placements, c->d_pls_out, total * sizeof(dcn_split_placement), hipMemcpyDeviceToHost));
    return DCN_OK;
}

extern "C" int dcn_place_pair_batch(dcn_ctx *ctx, const dcn_index *map, const uint8_t *bases, const uint64_t *offsets,
                                    uint32_t n_reads, const void *params, void *rows, uint64_t *tlen_hist) {
    const dcn_place_pair_params *prm = static_cast<const dcn_place_pair_params *>(params);
    DCN_TRY(check_vote_params(prm));
    if (prm->max_insert == 0) return dcn_fail(DCN_ERR_ARG, "params.max_insert must be at least 1");
    if (prm->hist_bin_bases == 0) return dcn_fail(DCN_ERR_ARG, "params.hist_bin_bases must be at least 1");
    if (n_reads % 2 != 0) return dcn_fail(DCN_ERR_ARG, "n_reads must be even: reads 2u and 2u + 1 are the mates of pair u");
    DCN_TRY(check_target(ctx, map));
    if (n_reads == 0) {
        if (tlen_hist) memset(tlen_hist, 0, DCN_PAIR_HIST_BINS * sizeof(uint64_t));
        return DCN_OK;
    }
    uint64_t n_bases = 0;
    DCN_TRY(check_batch(ctx, bases, offsets, n_reads, rows ? nullptr : "rows is NULL", &n_bases));
    dcn_ctx *c = ctx;
    DCN_HIP(hipSetDevice(c->device));
    if (!c->d_ppr_out) DCN_TRY(dev_alloc(&c->d_ppr_out, c->max_reads, "pair placements"));
    if (!c->d_ppr_hist) DCN_TRY(dev_alloc(&c->d_ppr_hist, DCN_PAIR_HIST_BINS, "insert histogram"));
    int prof_slot = -1;
    dcn_place_split_args sa;
    DCN_TRY(place_prepare(c, map, bases, offsets, n_reads, n_bases, prm, PLACE_PAIR, &prof_slot, &sa));
    hipStream_t st = c->stream;
    DCN_TRY(dcn_launch_place_split_rounds(sa, st));
    dcn_place_pair_args pp;
    memset(&pp, 0, sizeof(pp));
    pp.rounds = sa.rounds;
    pp.n_rounds = sa.n_rounds;
    pp.read_counts = sa.read_counts;
    pp.counts = sa.counts;
    pp.n_pairs = n_reads / 2;
    pp.max_placements = prm->max_placements;
    pp.k = map->k;
    pp.min_votes = prm->min_votes;
    pp.max_insert = prm->max_insert;
    pp.hist_bin_bases = prm->hist_bin_bases;
    pp.out = c->d_ppr_out;
    pp.hist = tlen_hist ? c->d_ppr_hist : nullptr; // (NULL: the kernel skips its LDS counters)
    if (tlen_hist) DCN_HIP(hipMemsetAsync(c->d_ppr_hist, 0, DCN_PAIR_HIST_BINS * sizeof(unsigned long long), st));
    DCN_TRY(dcn_launch_place_pair(pp, st));
    DCN_PROF_MARK(DCN_STAGE_FINISH);
    DCN_TRY(finish_run(c, prof_slot));
    DCN_HIP(hipMemcpy(rows, c->d_ppr_out, (uint64_t)n_reads * sizeof(dcn_pair_placement), hipMemcpyDeviceToHost));
    if (tlen_hist) DCN_HIP(hipMemcpy(tlen_hist, c->d_ppr_hist, DCN_PAIR_HIST_BINS * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return DCN_OK;
}

// dcn_ctx.h -- the filter context and what the files that implement the C ABI's host side share (internal, like
// dcn_internal.h): api.hip (errors, indexes), ctx.hip (context, device-pointer batches, the stage builders, the dump
// front end and the tail of a batch call), host_batch.hip (submit / wait), dump.hip (minimizer dump, hash seam, index
// build), and the dump's consumers, which all run dump_front_end .. finish_run of ctx.hip around kernels that sweep
// the dump as dcn_dump_sweep.h says: classify_api.hip (index sets; depth counters with depth_api.hip), locate_api.hip
// (segments), track_api.hip (depth tracks), place_api.hip (anchor maps, placement).
#pragma once

#include "dcn_dump_sweep.h"
#include "dcn_internal.h"
#include "dcn_plan.h"

#include <algorithm>
#include <functional>
#include <vector>

struct dcn_split_round; // (dcn_place.h)
struct dcn_verify_item; // (dcn_verify.h)
struct dcn_align_work;  // (dcn_verify.h)
struct dcn_extend_item;   // (dcn_verify.h)
struct dcn_extend_result; // (dcn_verify.h)

// One pipeline step of a host batch: reads [r0, r1) = units [u0, u1) = bases [b0, b1) of the batch stream.
// groups [g0, g1) of the invalid-base mask that crossed the link as their non-zero words only: n (group, word) pairs at
// pairs_off of the slot's pair buffer; the range is cleared and the pairs scattered in front of the chunk's kernels
struct dcn_mask_range {
    uint64_t g0 = 0, g1 = 0, pairs_off = 0;
    uint32_t n = 0;
};

struct dcn_chunk {
    uint32_t r0 = 0, r1 = 0, u0 = 0, u1 = 0;
    uint64_t b0 = 0, b1 = 0;
    uint64_t max_len = 0; // longest read of the chunk
    std::vector<dcn_mask_range> mask_ranges;
};

// One host batch in flight (dcn_filter_batch_submit .. dcn_filter_batch_wait).  Everything a later batch's copies
// could overwrite while this batch's kernels still read it is per slot; the compute scratch (tiles, per-unit state,
// hit records) is shared, because all kernels of a context run on one stream.  Slot 0 uses the context's own
// buffers, slot 1 is allocated when a second batch is first submitted while slot 0 is busy.
struct dcn_slot {
    bool allocated = false, busy = false, owns_buffers = false;
    uint64_t ticket = 0;
    // device inputs / outputs
    uint8_t *d_ascii = nullptr;
    uint32_t *d_packed = nullptr, *d_invmask = nullptr;
    uint64_t *d_offsets = nullptr;
    // offsets of a batch of < 2^32 bases cross the link as u32 (4 instead of 8 bytes per read: 6 % of a packed call's bytes)
    // and are widened into d_offsets by a kernel in front of each chunk's own kernels
    uint32_t *d_off32 = nullptr, *h_off32 = nullptr;
    bool off32 = false;
    bool lean = false; // submitted on one stream, plain forms of everything (see submit_impl)
    // The invalid-base mask of a packed stream is a third of its bytes and almost all zero (a word per 32 bases, non-zero
    // only where a base is not ACGT): its non-zero words cross the link as (group, word) pairs, the rest is a memset on the
    // device.  A chunk whose pairs do not fit (one group in 16 non-zero, over the batch) goes whole.
    uint2 *d_mask_pairs = nullptr, *h_mask_pairs = nullptr;
    uint64_t mask_pairs_cap = 0, mask_pairs_used = 0;
    uint32_t *d_unit_id = nullptr;
    uint8_t *d_keep = nullptr;
    uint32_t *d_hits = nullptr, *d_total = nullptr;
    dcn_batch_report *d_report = nullptr;
    // page-locked result staging (used when the caller's output arrays are pageable)
    uint8_t *h_keep = nullptr;
    uint32_t *h_hits = nullptr, *h_total = nullptr;
    dcn_batch_report *h_report = nullptr;
    hipEvent_t done = nullptr;
    std::vector<hipEvent_t> ev_h2d, ev_comp; // one pair per chunk, grown on demand
    // the submitted batch, kept for result delivery and for the re-run after a record overflow
    dcn_params params = {};
    bool device_pack = false; // ASCII crossed the link: the pack kernel runs, read ends are probed for a newline
    bool has_units = false, counts = false;
    uint32_t n_reads = 0, n_units = 0;
    uint64_t n_bases = 0;
    uint8_t *u_keep = nullptr;
    uint32_t *u_hits = nullptr, *u_total = nullptr;
    bool keep_direct = false, hits_direct = false, total_direct = false; // caller's arrays are page-locked: copied into directly
    std::vector<dcn_chunk> chunks;
};

struct dcn_ctx {
    const dcn_index *index = nullptr;
    int device = 0;
    hipStream_t stream = nullptr, copy_stream = nullptr, d2h_stream = nullptr;
    // device-pointer API, pack one batch ahead (ensure_pack_ahead): a second packed stream + mask, the pack kernel's own
    // status words and stream, and per buffer "packed" / "free again" events
    hipStream_t pack_stream = nullptr;
    uint32_t *d_packed_b = nullptr, *d_invmask_b = nullptr;
    dcn_status *d_pack_status = nullptr; // [2]
    hipEvent_t pack_done[2] = {}, buf_free[2] = {}, plan_done = nullptr;
    int pack_buf = 0, pack_ahead_state = 0; // 0 = not tried yet, 1 = ready, -1 = off (DCN_NO_PACK_AHEAD, or no memory for it)
    static constexpr int N_STAGE = 3, N_EV = 8, N_SLOTS = 2;
    hipEvent_t copy_done = nullptr, stage_free[N_STAGE] = {};
    hipEvent_t ev_h2d[N_EV] = {}, ev_comp[N_EV] = {};
    int ev_next = 0, stage_next = 0;
    uint64_t max_bases = 0;
    uint32_t max_reads = 0;
    uint32_t tile_windows = 256; // long reads: 12 % faster scan than 512 (fewer mid-scan flushes per wave), 128 and 1024 slower (profiles/r02_tile_sweep.txt)
    uint32_t max_tiles = 0;
    uint64_t chunk_bases = 0; // pipeline granularity of the host API (DCN_CHUNK_BASES)
    // device inputs (host API staging targets of slot 0; also used by the minimizer dump and the index build)
    uint8_t *d_ascii = nullptr;
    uint64_t *d_offsets = nullptr;
    uint32_t *d_unit_id = nullptr;
    // packed stream
    uint32_t *d_packed = nullptr, *d_invmask = nullptr; // allocations (views skip DCN_FRONT_PAD words)
    // plan
    uint32_t *d_read_tiles = nullptr, *d_read_tile_first = nullptr;
    uint32_t *d_unit_first_read = nullptr, *d_unit_tile_first = nullptr, *d_unit_tile_count = nullptr;
    dcn_tile *d_tiles = nullptr;
    // per-unit results / scratch
    uint8_t *d_keep = nullptr, *d_unit_state = nullptr;
    uint32_t *d_hits = nullptr, *d_total = nullptr;
    uint32_t *d_unit_scratch = nullptr; // g_total | g_hitcnt | g_distinct | g_zero, max_reads each; zero between batches
    bool scratch_dirty = false;         // a run was enqueued up to, but not including, its finish kernel
    uint32_t *d_caps = nullptr, *d_set_off = nullptr;
    // hit records + distinct sets
    // hit runs of the units the scan does not finish (one slot per base, see scan.hip) + global sets of the few
    // units whose hits do not fit the LDS set of the distinct pass (4 slots per record of capacity)
    uint64_t *d_rec_hash = nullptr;
    uint32_t rec_shift = 0;      // one slot of d_rec_hash per 2^rec_shift bases (dcn_scan_args::rec_shift)
    char *d_slab = nullptr;      // DCN_CTX_SLAB: one allocation behind the fixed-size buffers above
    uint64_t slab_bytes = 0;
    uint32_t *d_tile_hits = nullptr, *d_pending = nullptr;
    uint2 *d_big = nullptr; // work items of the distinct pass B: at most one per 64 tiles + one per unit
    uint64_t rec_capacity = 0;
    uint64_t *d_set_slots = nullptr;
    dcn_status *d_status = nullptr;
    // short batches (scan.hip, scan_short): what each wave of the scan kernel kept, one word per 64 reads (kept reads << 32 |
    // kept bases); every wave of such a batch writes its word and the finish kernel sums them
    unsigned long long *d_wave_kept = nullptr;
    bool short_fused = true;       // DCN_NO_SHORT_FUSED unset: batches of short unpaired reads are packed inside the scan kernel
    bool last_batch_short = false; // ... and whether the last batch waited for was one (dcn_ctx_last_batch_short)
    dcn_batch_report *d_report = nullptr; // device-pointer API: counters + sticky overflow since the last synchronize
    dcn_batch_report *h_report = nullptr; // page-locked
    uint64_t host_stats[DCN_N_STATS] = {}; // counters of completed host batches
    // pinned host staging (pageable inputs)
    uint8_t *h_stage[N_STAGE] = {};
    uint64_t stage_bytes = 0;
    dcn_slot slots[N_SLOTS];
    uint64_t next_ticket = 1;
    // dump mode buffers (lazy)
    uint64_t *d_dump_hash = nullptr;
    uint32_t *d_dump_pos = nullptr, *d_dump_count = nullptr, *d_tile_read_pos = nullptr;
    uint8_t *d_dump_valid = nullptr;
    // classification buffers (lazy, first dcn_classify_batch*): work list of the workgroup kernel + its length, and the
    // host form's outputs (hits: cls_hits_members per unit)
    uint32_t *d_cls_big = nullptr, *d_cls_n_big = nullptr;
    uint32_t *d_cls_match = nullptr, *d_cls_hits = nullptr, *d_cls_total = nullptr;
    uint32_t cls_hits_members = 0;
    // what the dump's consumers mark positions in (lazy: ensure_position_bitmap / ensure_position_words): a bit per base
    // (locate's hits, the positions of track, place and the depth sweep) and a word per base (locate's labels on a set,
    // track's values)
    uint32_t *d_loc_bits = nullptr, *d_loc_labels = nullptr;
    // locate buffers (lazy, first dcn_locate_batch): per-read counts / offsets with the scan's block sums, the work list
    // of the wave kernel, and the segment buffer (loc_seg_cap entries, grown to the largest count)
    uint32_t *d_loc_counts = nullptr, *d_loc_big = nullptr, *d_loc_n_big = nullptr;
    unsigned long long *d_loc_block_sums = nullptr;
    uint64_t *d_loc_seg_offsets = nullptr;
    dcn_segment *d_loc_segs = nullptr;
    uint64_t loc_seg_cap = 0;
    // depth track buffers (lazy, first dcn_depth_track_batch): per-read bin and piece offsets, computed on the host, and
    // the bins (trk_bin_cap entries, grown to the largest batch's count)
    uint64_t *d_trk_bin_offsets = nullptr, *d_trk_piece_offsets = nullptr;
    dcn_track_bin *d_trk_bins = nullptr;
    uint64_t trk_bin_cap = 0;
    // placement buffers (lazy, first dcn_place_batch): the anchor bitmap, one word per base (dcn_place.h), the work list
    // of the workgroup kernel with its length, and the placements
    uint64_t *d_plc_words = nullptr;
    uint32_t *d_plc_abits = nullptr, *d_plc_big = nullptr, *d_plc_n_big = nullptr;
    dcn_placement *d_plc_out = nullptr;
    // split placement buffers (lazy, first dcn_place_split_batch; dcn_place.h): the copy of the anchor bitmap that the
    // rounds clear, per read the round count, the two counts, the placement count and the CSR offsets with the scan's
    // block sums; the rounds and the rows grow to the largest n_reads * (max_placements + 1) and n_reads * max_placements
    uint32_t *d_pls_rbits = nullptr, *d_pls_n_rounds = nullptr, *d_pls_read_counts = nullptr, *d_pls_counts = nullptr;
    unsigned long long *d_pls_block_sums = nullptr;
    uint64_t *d_pls_offsets = nullptr;
    dcn_split_round *d_pls_rounds = nullptr;
    dcn_split_placement *d_pls_out = nullptr;
    uint64_t pls_round_cap = 0, pls_out_cap = 0;
    // paired placement buffers (lazy, first dcn_place_pair_batch): one row per read and the insert histogram
    dcn_pair_placement *d_ppr_out = nullptr;
    unsigned long long *d_ppr_hist = nullptr;
    // verify buffers (lazy, first dcn_verify_batch; dcn_verify.h): one item and one result per row, grown to the largest n_rows
    dcn_verify_item *d_vfy_items = nullptr;
    uint32_t *d_vfy_out = nullptr;
    uint64_t vfy_items_cap = 0, vfy_out_cap = 0;
    // align buffers (lazy, first dcn_align_batch; each grows to the largest call's need): the aligned rows, per row the
    // number of runs and their CSR offsets with the scan's scratch, the trace of one group of rows (words; at most the
    // budget of DCN_ALIGN_TRACE_BYTES, or one row's trace when that is larger), the run slots and the compact runs
    dcn_align_work *d_aln_work = nullptr;
    uint32_t *d_aln_n_ops = nullptr, *d_aln_trace = nullptr, *d_aln_slots = nullptr, *d_aln_cigar = nullptr;
    uint64_t *d_aln_offsets = nullptr;
    unsigned long long *d_aln_block_sums = nullptr;
    uint64_t aln_work_cap = 0, aln_rows_cap = 0, aln_offsets_cap = 0, aln_trace_cap = 0, aln_slots_cap = 0, aln_cigar_cap = 0;
    // left-align buffers (lazy, first call that left-aligns): a second slot array and the four totals of a call
    uint32_t *d_aln_scratch = nullptr;
    uint64_t aln_scratch_cap = 0;
    unsigned long long *d_aln_la_totals = nullptr;
    // extend buffers (lazy, first dcn_extend_batch; dcn_verify.h): two items and two results per row, grown to the largest n_rows
    dcn_extend_item *d_ext_items = nullptr;
    dcn_extend_result *d_ext_out = nullptr;
    uint64_t ext_items_cap = 0, ext_out_cap = 0;
    // quality buffer (lazy, first dcn_pileup_batch_qual): one byte per base, grown to the largest such batch
    uint8_t *d_pile_quals = nullptr;
    uint64_t pile_quals_cap = 0;
    // deferred state of the last enqueued device-API batch
    bool batch_pending = false;
    bool lean = false; // a small host batch is being submitted: copies and result copies go on `stream` itself (submit_impl)
    // optional per-stage timing: a ring of event sets, one per batch in flight
    static constexpr int PROF_RING = 64;
    int profiling = 0; // 0 off, 1 every stage, 2 the scan stage only (two events per run instead of six)
    hipEvent_t prof_ev[PROF_RING][DCN_N_STAGES + 1] = {};
    bool prof_used[PROF_RING] = {}, prof_scan_only[PROF_RING] = {};
    int prof_next = 0;
    double prof_ms[DCN_N_STAGES] = {};
    uint64_t prof_batches = 0;
};

// host_pack.cpp: the host-side 2-bit packer
bool dcn_host_pack_is_wide();
bool dcn_host_pack_groups(const uint8_t *ascii, uint64_t n_bases, uint64_t g0, uint64_t g1, uint32_t *packed,
                          uint32_t *mask); // true: a '\n' byte was seen

#define DCN_TRY(expr)              \
    do {                           \
        int _rc = (expr);          \
        if (_rc != DCN_OK) return _rc; \
    } while (0)

// (a timed event is a marker packet the stream stops at: six per run cost the headline step ~2.5 %, which is why
// the scan-only level exists: the end of the plan stage is the start of the scan stage)
#define DCN_PROF_MARK(stage)                                                                                      \
    do {                                                                                                          \
        if (prof_slot >= 0 && (c->profiling == 1 || (stage) == DCN_STAGE_PLAN || (stage) == DCN_STAGE_SCAN))      \
            DCN_HIP(hipEventRecord(c->prof_ev[prof_slot][(stage) + 1], st));                                      \
    } while (0)

// Helpers that cross the files above.  None of them is part of the shared object's exported surface.
#pragma GCC visibility push(hidden)
namespace dcn_impl {

template <typename T>
int dev_alloc(T **p, uint64_t count, const char *what) {
    hipError_t e = hipMalloc((void **)p, std::max<uint64_t>(count, 1) * sizeof(T));
    if (e != hipSuccess) {
        *p = nullptr;
        return dcn_fail(DCN_ERR_NOMEM, std::string("hipMalloc ") + what + ": " + hipGetErrorString(e));
    }
    return DCN_OK;
}

// a device buffer of a context that only grows: at least `need` T behind *p, *cap of them
template <typename T>
int grow(T **p, uint64_t *cap, uint64_t need, const char *what) {
    if (need <= *cap && *p) return DCN_OK;
    if (*p) hipFree(*p);
    *p = nullptr;
    *cap = 0;
    DCN_TRY(dev_alloc(p, need, what));
    *cap = need;
    return DCN_OK;
}

// `count` zeroed T on the current device, there when the call returns (state that lives with an index: a set's labels,
// coverage bits and depth counters, a map's words); *p is null when it fails
template <typename T>
int dev_alloc_zeroed(T **p, uint64_t count, const char *what) {
    *p = nullptr;
    T *d = nullptr;
    hipError_t e = hipMalloc((void **)&d, count * sizeof(T));
    if (e == hipSuccess) e = hipMemset(d, 0, count * sizeof(T));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        if (d) hipFree(d);
        return dcn_hip_fail(e, what);
    }
    *p = d;
    return DCN_OK;
}
} // namespace dcn_impl

// device memory of one range call over a pileup (pileup_api.hip, genotype_api.hip), freed when the call ends
namespace dcn_pile_api {
struct scratch {
    static constexpr int SLOTS = 6; // dcn_anchor_map_genotype and dcn_anchor_map_reference_blocks fill all of them
    void *p[SLOTS] = {};
    int n = 0;
    template <typename T>
    int get(T **out, uint64_t count, const char *what) {
        if (n == SLOTS) return dcn_fail(DCN_ERR_INTERNAL, std::string("no scratch slot left for ") + what);
        DCN_TRY(dcn_impl::dev_alloc(out, count, what));
        p[n++] = *out;
        return DCN_OK;
    }
    ~scratch() {
        for (int i = 0; i < n; ++i) hipFree(p[i]);
    }
};
} // namespace dcn_pile_api

namespace dcn_impl {
// device scratch that goes back on every way out
struct DevMem {
    void *p = nullptr;
    ~DevMem() {
        if (p) hipFree(p);
    }
    int alloc(uint64_t bytes, bool zero, const char *what) {
        hipError_t e = hipMalloc(&p, std::max<uint64_t>(bytes, 8));
        if (e == hipSuccess && zero) e = hipMemset(p, 0, std::max<uint64_t>(bytes, 8));
        return e == hipSuccess ? DCN_OK : dcn_hip_fail(e, what);
    }
    int clear(const char *what) { // the first 8 bytes: a counter between two sweeps
        const hipError_t e = hipMemset(p, 0, 8);
        return e == hipSuccess ? DCN_OK : dcn_hip_fail(e, what);
    }
    int read(void *h, uint64_t bytes, const char *what) const { // (the copy waits for the null stream)
        const hipError_t e = hipMemcpy(h, p, bytes, hipMemcpyDeviceToHost);
        return e == hipSuccess ? DCN_OK : dcn_hip_fail(e, what);
    }
    template <typename T>
    T *as() const {
        return (T *)p;
    }
};

// the counter of a sweep, after the sweep
inline int read_count(const DevMem &d_n, const char *what, unsigned long long *n) { return d_n.read(n, sizeof(*n), what); }

inline uint64_t packed_words(uint64_t max_bases) { return DCN_FRONT_PAD + 2 * ((max_bases + 31) / 32) + DCN_TAIL_PAD; }
inline uint64_t mask_words(uint64_t max_bases) { return DCN_FRONT_PAD + (max_bases + 31) / 32 + DCN_TAIL_PAD; }

// What one run of the device pipeline works on: a whole batch of the device-pointer API, or one chunk of a host
// batch.  Base offsets in d_offsets are positions in the batch stream (d_ascii / d_packed are the stream's
// origin); read and unit indices are local to the view (arrays already point at the view's first entry).
struct BatchView {
    const uint8_t *d_ascii = nullptr;  // null: the stream arrived packed (no pack kernel, no newline probe)
    uint32_t *d_packed = nullptr, *d_invmask = nullptr; // allocation starts (DCN_FRONT_PAD words in front of base 0)
    const uint64_t *d_offsets = nullptr;
    const uint32_t *d_unit_id = nullptr;
    uint32_t unit_base = 0;
    uint32_t n_reads = 0, n_units = 0;
    uint64_t b0 = 0, b1 = 0; // bases of the stream this view covers
    uint64_t stream_bases = 0; // bases of the whole stream
    uint8_t *d_keep = nullptr;
    uint32_t *d_hits = nullptr, *d_total = nullptr;
    dcn_batch_report *d_report = nullptr;
};

// ---- api.hip ----
int same_params(const dcn_index *a, const dcn_index *b); // k, w, device and minimizer rule agree (else DCN_ERR_ARG)
int check_kw(uint8_t k, uint8_t w);                      // the k / w rule every index is made under (else DCN_ERR_ARG)

// ---- dump.hip: the chunk loop both index builds share ----
constexpr uint32_t DCN_BUILD_MAX_PIECES = 1u << 16;
uint64_t build_chunk_bases(); // 2^27, or DCN_BUILD_CHUNK_BASES (>= 4096)
using build_sweep_fn = std::function<int(uint64_t nb, bool continues)>;
// DCN_INDEX_TIMING: where a build's time goes, one stderr line when it ends.  Host seconds here; the device stages come
// from the context's stage events (dcn_ctx_profile), the sweep -- reserve included -- in the DISTINCT slot.
struct build_times {
    double front_end_s = 0, staging_s = 0, growth_s = 0, finish_s = 0, finish_table_s = 0;
};
double build_now(); // seconds on a steady clock
int build_timing_begin(dcn_ctx *c); // (turns the context's stage events on)
int build_times_print(const char *which, dcn_ctx *c, const build_times &t);
// times: null, or a build that runs under build_timing_begin (staging is then waited for, chunk by chunk)
int build_run_chunks(dcn_ctx *c, const dcn_index *idx, const uint8_t *bases, const uint64_t *offsets, uint32_t n_seqs,
                     uint64_t chunk_bases, const build_sweep_fn &sweep, build_times *times = nullptr);

// ---- classify_api.hip ----
int check_set(const dcn_index *set); // not NULL and a labelled set (else DCN_ERR_ARG)

// ---- ctx.hip: context plumbing ----
int alloc_records(dcn_ctx *c, uint64_t n_records);
void free_slot_buffers(dcn_slot &sl);
int prof_begin(dcn_ctx *c, int *slot);
int check_params(const dcn_params *p);
int enqueue_batch(dcn_ctx *c, const BatchView &v, const dcn_params *params, bool pack_ahead = false);
int grow_run_slots(dcn_ctx *c);
int overflow_error(const dcn_ctx *c, uint64_t need);
int sync_and_check(dcn_ctx *c, uint64_t *needed_records);
bool is_pinned_host(const void *p);
int staged_h2d(dcn_ctx *c, void *d_dst, const void *h_src, uint64_t bytes, int pinned = -1);
int slots_busy(const dcn_ctx *c);

// ---- ctx.hip: argument checks shared by entry points (codes and messages are what callers see) ----
int check_idle(const dcn_ctx *c); // no host batch in a slot, no device-pointer batch since the last synchronize
// the context's index reads sequences as `other` does (k, w, minimizer rule), on its device, and the context is idle;
// `noun` names `other` in the messages ("the set", "the map")
int check_ctx_matches(const dcn_ctx *c, const dcn_index *other, const char *noun);
int check_device_batch(const dcn_ctx *c, uint32_t n_reads, uint64_t n_bases, uint32_t n_units, const uint32_t *d_unit_id);
// offsets[0] == 0, non-decreasing, no entry over 2^32: `noun` names the array, `too_long` is that last message whole
int check_offsets_walk(const uint64_t *offsets, uint32_t n, const char *noun, const char *too_long);
// a host batch run whole on an idle context (minimizer dump, classification): limits, idle, offsets
int validate_host_batch(const dcn_ctx *c, const uint64_t *offsets, uint32_t n_reads);

// ---- ctx.hip: one builder per stage.  Each writes the fields every caller sets alike; what differs between callers
// is set at the call site, and a field a caller leaves out stays zero. ----
int ensure_dump_buffers(dcn_ctx *c); // the four arrays of a dump-mode scan, allocated on first use
int ensure_position_bitmap(dcn_ctx *c); // d_loc_bits: a bit per base of the largest batch (+ a word), on first use
int ensure_position_words(dcn_ctx *c);  // d_loc_labels: a word per base, on first use
struct UnitScratch { // d_unit_scratch, max_reads words each
    uint32_t *g_total, *g_hitcnt, *g_distinct, *g_zero;
};
UnitScratch unit_scratch(const dcn_ctx *c);
// into the context's d_ascii / d_offsets / d_unit_id on the copy stream; the compute stream then waits for copy_done
int stage_batch(dcn_ctx *c, const uint8_t *bases, uint64_t n_bases, const uint64_t *offsets, uint32_t n_reads,
                const uint32_t *unit_id_or_null);
int stage_done(dcn_ctx *c); // that record / wait tail alone, for a caller that stages piecewise
// Left to the caller: unit_base, read_tiles / read_tile_first, tile_read_pos, unit_state / unit_scratch / scratch_stride,
// newline_flag, and check_offsets + stream_bases + max_tiles (the plan kernel's own check of the offsets).
dcn_plan_args plan_args(const dcn_ctx *c, const dcn_index *index, const uint8_t *d_ascii, const uint64_t *d_offsets,
                        const uint32_t *d_unit_id, uint32_t n_reads, uint32_t n_units, uint64_t prefix_length);
// a scan of the context's packed stream in dump mode; left to the caller: tile_read_pos, dump_abs
dcn_scan_args dump_scan_args(const dcn_ctx *c, const dcn_index *index, uint64_t n_bases);
uint32_t tile_bound(const dcn_ctx *c, uint32_t n_reads, uint64_t n_bases); // launch bound of a scan: tiles the plan can cut
// the plan and the dump that a dump-mode scan of the context leaves, as the kernels of dcn_dump_sweep.h take them
dcn_dump_view dump_view(const dcn_ctx *c, uint32_t max_tiles, uint64_t n_bases);

// ---- ctx.hip: a batch call that consumes the minimizer dump (classify, depth, locate, track, anchor add, place) ----
// Begins the run's profile slot (*prof_slot, -1: none) and enqueues pack -> plan -> scan in dump mode with batch-absolute
// positions on c->stream; *view is what the scan leaves.  The batch is device memory; d_unit_id may be null.
// plan_checks_offsets: the host has not walked the offsets, the plan kernel does (classification).
int dump_front_end(dcn_ctx *c, const dcn_index *index, const uint8_t *d_ascii, const uint64_t *d_offsets,
                   const uint32_t *d_unit_id, uint32_t n_reads, uint32_t n_units, uint64_t n_bases, uint64_t prefix_length,
                   bool plan_checks_offsets, int *prof_slot, dcn_dump_view *view);
// what follows the last kernel of such a call: the profile slot is in use, and the events a later device-pointer filter
// batch waits for stand after this run ...
int record_run_end(dcn_ctx *c, int prof_slot);
// ... then the wait, and what the device reported
int finish_run(dcn_ctx *c, int prof_slot);
dcn_distinct_args distinct_args(const dcn_ctx *c, uint32_t n_units, const dcn_params *params, const uint64_t *rec_hash,
                                uint32_t rec_shift, uint32_t *g_total_or_null);
dcn_finish_args finish_args(const dcn_ctx *c, uint32_t n_units, const dcn_params *params, const uint32_t *unit_first_read,
                            const uint64_t *offsets, uint8_t *keep, uint32_t *hits, uint32_t *total, dcn_batch_report *report);

} // namespace dcn_impl
#pragma GCC visibility pop

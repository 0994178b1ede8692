// ctx.hip -- the filter context: its buffers, streams and staging, the device-pointer filter path, and the order in
// which the kernels of the batch pipeline are enqueued.
//
// One batch on the context's compute stream:
//   memset(per-unit scratch) -> pack (K1) -> plan (one launch) -> scan (K2-K5, fused)
//   -> distinct pass for multi-wave units -> finish (decision + six counters, K6)
// Host batches are staged through pinned buffers and copied with hipMemcpyAsync on a side stream while the host fills
// the next buffer; the compute stream waits on the copy's event (host_batch.hip).
//
// The stage builders at the end fill the argument structs of plan, scan (dump mode), distinct and finish for every
// caller: this file's enqueue_batch, dump.hip and classify_api.hip.
#include "dcn_ctx.h"
#include "dcn_host_pool.h"

#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>

using dcn_host::HostPool;

uint32_t dcn_cu_count() {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    // DCN_GRID_CUS, read at call time: a test hook that lowers the count (never raises it), so that a few hundred items
    // already make every capped grid loop.  Unset, empty, 0 or not a number: the device's count.
    const char *s = std::getenv("DCN_GRID_CUS");
    char *end = nullptr;
    unsigned long long cap = s && *s ? std::strtoull(s, &end, 10) : 0;
    if (end && *end) cap = 0; // (something behind the digits: not a number)
    if (cap >= 1) cus = (int)std::min<unsigned long long>(cap, (unsigned long long)std::max(cus, 1));
    return (uint32_t)std::max(cus, 1);
}

namespace dcn_impl {

int alloc_records(dcn_ctx *c, uint64_t n_records) {
    n_records = (n_records + 63) / 64 * 64;
    if (n_records > (1ull << 29)) return dcn_fail(DCN_ERR_CAPACITY, "more than 2^29 hit records in global sets per batch: use smaller batches");
    if (c->d_set_slots) hipFree(c->d_set_slots);
    c->d_set_slots = nullptr;
    c->rec_capacity = 0;
    DCN_TRY(dev_alloc(&c->d_set_slots, 4 * n_records + 64, "set_slots"));
    c->rec_capacity = n_records;
    return DCN_OK;
}

void free_slot_buffers(dcn_slot &sl) {
    if (sl.owns_buffers) {
        void *dev[] = {sl.d_ascii, sl.d_packed, sl.d_invmask, sl.d_offsets, sl.d_unit_id, sl.d_keep, sl.d_hits, sl.d_total};
        for (void *p : dev)
            if (p) hipFree(p);
    }
    if (sl.d_report) hipFree(sl.d_report);
    if (sl.d_off32) hipFree(sl.d_off32);
    if (sl.d_mask_pairs) hipFree(sl.d_mask_pairs);
    void *host[] = {sl.h_keep, sl.h_hits, sl.h_total, sl.h_report, sl.h_off32, sl.h_mask_pairs};
    for (void *p : host)
        if (p) hipHostFree(p);
    if (sl.done) hipEventDestroy(sl.done);
    for (hipEvent_t e : sl.ev_h2d) hipEventDestroy(e);
    for (hipEvent_t e : sl.ev_comp) hipEventDestroy(e);
    sl = dcn_slot();
}

static void free_ctx(dcn_ctx *c) {
    if (!c) return;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    if (c->copy_stream) hipStreamSynchronize(c->copy_stream);
    if (c->d2h_stream) hipStreamSynchronize(c->d2h_stream);
    if (c->pack_stream) {
        hipStreamSynchronize(c->pack_stream);
        hipStreamDestroy(c->pack_stream);
    }
    for (int i = 0; i < 2; ++i) {
        if (c->pack_done[i]) hipEventDestroy(c->pack_done[i]);
        if (c->buf_free[i]) hipEventDestroy(c->buf_free[i]);
    }
    if (c->plan_done) hipEventDestroy(c->plan_done);
    if (c->d_packed_b) hipFree(c->d_packed_b);
    if (c->d_invmask_b) hipFree(c->d_invmask_b);
    if (c->d_pack_status) hipFree(c->d_pack_status);
    for (auto &sl : c->slots) free_slot_buffers(sl);
    void *dev[] = {c->d_ascii, c->d_offsets, c->d_unit_id, c->d_packed, c->d_invmask,
                   c->d_read_tiles, c->d_read_tile_first, c->d_unit_first_read, c->d_unit_tile_first, c->d_unit_tile_count, c->d_tiles,
                   c->d_keep, c->d_unit_state, c->d_hits, c->d_total, c->d_unit_scratch, c->d_caps,
                   c->d_set_off, c->d_tile_hits, c->d_pending, c->d_big, c->d_rec_hash, c->d_set_slots, c->d_status, c->d_wave_kept, c->d_report, c->d_dump_hash,
                   c->d_dump_pos, c->d_dump_count, c->d_dump_valid, c->d_tile_read_pos,
                   c->d_cls_big, c->d_cls_n_big, c->d_cls_match, c->d_cls_hits, c->d_cls_total,
                   c->d_loc_bits, c->d_loc_labels, c->d_loc_counts, c->d_loc_big, c->d_loc_n_big, c->d_loc_block_sums,
                   c->d_loc_seg_offsets, c->d_loc_segs, c->d_trk_bin_offsets, c->d_trk_piece_offsets, c->d_trk_bins,
                   c->d_plc_words, c->d_plc_abits, c->d_plc_big, c->d_plc_n_big, c->d_plc_out,
                   c->d_pls_rbits, c->d_pls_n_rounds, c->d_pls_read_counts, c->d_pls_counts, c->d_pls_block_sums,
                   c->d_pls_offsets, c->d_pls_rounds, c->d_pls_out, c->d_ppr_out, c->d_ppr_hist, c->d_vfy_items, c->d_vfy_out,
                   c->d_aln_work, c->d_aln_n_ops, c->d_aln_trace, c->d_aln_slots, c->d_aln_cigar, c->d_aln_offsets, c->d_aln_block_sums,
                   c->d_ext_items, c->d_ext_out, c->d_pile_quals, c->d_aln_scratch, c->d_aln_la_totals};
    for (void *p : dev)
        if (p && !((char *)p >= c->d_slab && (char *)p < c->d_slab + c->slab_bytes)) hipFree(p);
    if (c->d_slab) hipFree(c->d_slab);
    for (int i = 0; i < dcn_ctx::N_STAGE; ++i) {
        if (c->h_stage[i]) hipHostFree(c->h_stage[i]);
        if (c->stage_free[i]) hipEventDestroy(c->stage_free[i]);
    }
    for (int i = 0; i < dcn_ctx::N_EV; ++i) {
        if (c->ev_h2d[i]) hipEventDestroy(c->ev_h2d[i]);
        if (c->ev_comp[i]) hipEventDestroy(c->ev_comp[i]);
    }
    if (c->h_report) hipHostFree(c->h_report);
    for (int i = 0; i < dcn_ctx::PROF_RING; ++i)
        for (int j = 0; j <= DCN_N_STAGES; ++j)
            if (c->prof_ev[i][j]) hipEventDestroy(c->prof_ev[i][j]);
    if (c->copy_done) hipEventDestroy(c->copy_done);
    if (c->stream) hipStreamDestroy(c->stream);
    if (c->copy_stream) hipStreamDestroy(c->copy_stream);
    if (c->d2h_stream) hipStreamDestroy(c->d2h_stream);
    delete c;
}

// fold the event pairs of every completed batch into the per-stage accumulators
static int prof_harvest(dcn_ctx *c, int only_slot = -1) {
    for (int i = 0; i < dcn_ctx::PROF_RING; ++i) {
        if (!c->prof_used[i] || (only_slot >= 0 && i != only_slot)) continue;
        const int first = c->prof_scan_only[i] ? DCN_STAGE_SCAN : 0, last = c->prof_scan_only[i] ? DCN_STAGE_SCAN : DCN_N_STAGES - 1;
        DCN_HIP(hipEventSynchronize(c->prof_ev[i][last + 1]));
        for (int j = first; j <= last; ++j) {
            float ms = 0.f;
            DCN_HIP(hipEventElapsedTime(&ms, c->prof_ev[i][j], c->prof_ev[i][j + 1]));
            c->prof_ms[j] += ms;
        }
        c->prof_batches++;
        c->prof_used[i] = false;
    }
    return DCN_OK;
}

// returns the event slot for this batch (or -1 when profiling is off) after recording its first event
int prof_begin(dcn_ctx *c, int *slot) {
    *slot = -1;
    if (!c->profiling) return DCN_OK;
    int i = c->prof_next;
    c->prof_next = (i + 1) % dcn_ctx::PROF_RING;
    if (c->prof_used[i]) DCN_TRY(prof_harvest(c, i));
    for (int j = 0; j <= DCN_N_STAGES; ++j)
        if (!c->prof_ev[i][j]) DCN_HIP(hipEventCreate(&c->prof_ev[i][j]));
    c->prof_scan_only[i] = c->profiling == 2;
    if (c->profiling == 1) DCN_HIP(hipEventRecord(c->prof_ev[i][0], c->stream));
    *slot = i;
    return DCN_OK;
}

int check_params(const dcn_params *p) {
    if (!p) return dcn_fail(DCN_ERR_ARG, "params is NULL");
    if (p->reserved != 0) return dcn_fail(DCN_ERR_ARG, "params.reserved must be 0");
    if (p->deplete > 1) return dcn_fail(DCN_ERR_ARG, "params.deplete must be 0 or 1");
    return DCN_OK;
}

// Device-pointer API, experiment kept behind DCN_PACK_AHEAD=1: the pack kernel of batch i+1 runs beside the scan kernel of
// batch i.  The pack is a streaming kernel (1 B/bp in, 0.375 out: 0.39 ms of a 3.7 ms step at 1.5 Gbp) and the scan kernel
// moves only 38 % of HBM's peak, so batch i+1's stream is packed into a SECOND buffer on a side stream once the batch that
// last read that buffer (i-1) has finished and batch i's plan kernel is through, instead of in front of its own scan.
// Costs 0.375 B per base of context; everything else of a batch stays in order on the context's stream.
static bool ensure_pack_ahead(dcn_ctx *c) {
    if (c->pack_ahead_state != 0) return c->pack_ahead_state > 0;
    c->pack_ahead_state = -1;
    // OFF unless asked for (DCN_PACK_AHEAD=1): measured in round 4 (profiles/r04_ab.txt section 4), it buys nothing.  The two
    // kernels do run side by side (kernel trace), and the scan kernel then takes longer by exactly the pack's time (3.30 ->
    // 3.67 ms, step 3.85 -> 3.88): what the scan kernel leaves of HBM's bandwidth is not spare -- its scattered sectors and
    // the pack's stream wait for the same DRAM cycles.
    if (!getenv("DCN_PACK_AHEAD") || getenv("DCN_NO_PACK_AHEAD")) return false;
    // (highest priority: the scan kernel's grid is 150 k workgroups deep, and a queue of ordinary priority only gets its
    // turn when that grid has drained)
    int prio_low = 0, prio_high = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_low, &prio_high);
    bool ok = hipStreamCreateWithPriority(&c->pack_stream, hipStreamNonBlocking, prio_high) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->plan_done, hipEventDisableTiming) == hipSuccess;
    for (int i = 0; ok && i < 2; ++i)
        ok = hipEventCreateWithFlags(&c->pack_done[i], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&c->buf_free[i], hipEventDisableTiming) == hipSuccess;
    ok = ok && hipMalloc((void **)&c->d_packed_b, packed_words(c->max_bases) * sizeof(uint32_t)) == hipSuccess &&
         hipMalloc((void **)&c->d_invmask_b, mask_words(c->max_bases) * sizeof(uint32_t)) == hipSuccess &&
         hipMalloc((void **)&c->d_pack_status, 2 * sizeof(dcn_status)) == hipSuccess;
    if (ok) { // (pads in front of and behind the stream are read by the scan kernel: zero, as in the first buffer)
        ok = hipMemset(c->d_packed_b, 0, packed_words(c->max_bases) * sizeof(uint32_t)) == hipSuccess &&
             hipMemset(c->d_invmask_b, 0, mask_words(c->max_bases) * sizeof(uint32_t)) == hipSuccess &&
             hipDeviceSynchronize() == hipSuccess; // null-stream memsets must not overtake the first pack
    }
    if (!ok) {
        (void)hipGetLastError(); // no memory for a second stream: batches are packed in line, as before
        if (c->d_packed_b) hipFree(c->d_packed_b);
        if (c->d_invmask_b) hipFree(c->d_invmask_b);
        if (c->d_pack_status) hipFree(c->d_pack_status);
        c->d_packed_b = c->d_invmask_b = nullptr;
        c->d_pack_status = nullptr;
        return false;
    }
    c->pack_ahead_state = 1;
    return true;
}

static dcn_scan_args scan_args(const dcn_ctx *c, const dcn_index *index, uint32_t *packed, uint32_t *invmask, uint64_t stream_bases);

// enqueue the whole device pipeline for one view on the context's compute stream
int enqueue_batch(dcn_ctx *c, const BatchView &v, const dcn_params *params, bool pack_ahead) {
    hipStream_t st = c->stream;
    const dcn_index *idx = c->index;
    // the per-unit scratch words are zero between batches (finish_kernel leaves them so); a run that did not get as
    // far as enqueueing its finish kernel may have left some behind
    if (c->scratch_dirty) DCN_HIP(hipMemsetAsync(c->d_unit_scratch, 0, (uint64_t)c->max_reads * 4 * sizeof(uint32_t), st));
    c->scratch_dirty = true;
    // per-run scratch: the status words (the per-unit state and scratch words are cleared by the plan kernel)
    DCN_HIP(hipMemsetAsync(c->d_status, 0, sizeof(dcn_status), st));

    int prof_slot = -1;
    DCN_TRY(prof_begin(c, &prof_slot));
    uint32_t *packed = v.d_packed + DCN_FRONT_PAD, *invmask = v.d_invmask + DCN_FRONT_PAD;
    int ahead_buf = -1;
    const uint32_t *newline_flag = nullptr;
    bool short_fused = false;
    static const bool no_early_out = getenv("DCN_NO_EARLY_OUT") != nullptr, no_early_out_pairs = getenv("DCN_NO_EARLY_OUT_PAIRS") != nullptr;
    // (the decisions-only instantiation of the scan kernel has no short path)
    const bool decisions_only_call = !v.d_hits && !v.d_total && params->abs_threshold >= 1 && params->abs_threshold <= 4 && !no_early_out;
    // (per-stage profiling wants the stages one after the other on one stream: in line then)
    if (v.d_ascii && pack_ahead && c->profiling != 1 && ensure_pack_ahead(c)) {
        ahead_buf = c->pack_buf;
        c->pack_buf ^= 1;
        if (ahead_buf == 1) {
            packed = c->d_packed_b + DCN_FRONT_PAD;
            invmask = c->d_invmask_b + DCN_FRONT_PAD;
        }
        dcn_status *ps = c->d_pack_status + ahead_buf;
        DCN_HIP(hipStreamWaitEvent(c->pack_stream, c->buf_free[ahead_buf], 0)); // (never recorded yet: no wait)
        // ... and not before the previous batch's plan kernel is through: its buffer is free from the moment the batch
        // before that one finished, which is just when the previous batch's (small, latency-bound) plan kernel starts --
        // packing beside THAT only delays the scan kernel behind it (kernel trace: plan 0.10 -> 0.47 ms)
        if (!getenv("DCN_PACK_AHEAD_EARLY")) DCN_HIP(hipStreamWaitEvent(c->pack_stream, c->plan_done, 0));
        DCN_HIP(hipMemsetAsync(ps, 0, sizeof(dcn_status), c->pack_stream));
        DCN_TRY(dcn_launch_pack_beside(v.d_ascii, v.b0, v.b1, packed, invmask, ps, c->pack_stream));
        DCN_HIP(hipEventRecord(c->pack_done[ahead_buf], c->pack_stream));
        DCN_HIP(hipStreamWaitEvent(st, c->pack_done[ahead_buf], 0));
        newline_flag = &ps->any_newline;
    } else if (v.d_ascii) {
        // a batch that may be all short reads: the shape kernel decides on the device, and if it says so the pack kernel below
        // returns at once and the scan kernel packs its own bases (scan.hip, scan_short).  Everything else is the classic path.
        short_fused = c->short_fused && !v.d_unit_id && params->prefix_length == 0 && v.b0 == 0 && v.b1 == v.stream_bases &&
                      v.n_reads == v.n_units && c->tile_windows >= dcn_short_lmax() && idx->variant == DCN_VARIANT_DEFAULT &&
                      dcn_scan_has_short_path(idx->k, idx->w) && !decisions_only_call;
        if (short_fused) DCN_TRY(dcn_launch_shape(v.d_offsets, v.n_reads, v.stream_bases, dcn_short_lmax(), c->d_status, st));
        DCN_TRY(dcn_launch_pack(v.d_ascii, v.b0, v.b1, packed, invmask, c->d_status, st));
    }
    DCN_PROF_MARK(DCN_STAGE_PACK);

    const uint32_t n_reads = v.n_reads, n_units = v.n_units;
    dcn_plan_args pa = plan_args(c, idx, v.d_ascii, v.d_offsets, v.d_unit_id, n_reads, n_units, params->prefix_length);
    pa.unit_base = v.unit_base;
    pa.unit_state = c->d_unit_state; // (per-read tile ranges stay null: only the dump-mode callers need them)
    pa.unit_scratch = c->d_unit_scratch;
    pa.scratch_stride = c->max_reads;
    pa.newline_flag = newline_flag;
    pa.stream_bases = v.stream_bases;
    pa.check_offsets = 1;
    pa.max_tiles = c->max_tiles;
    pa.short_armed = short_fused ? 1u : 0u;
    DCN_TRY(dcn_launch_plan(pa, st));
    if (pack_ahead && c->pack_ahead_state == 1) DCN_HIP(hipEventRecord(c->plan_done, st));
    DCN_PROF_MARK(DCN_STAGE_PLAN);

    const UnitScratch us = unit_scratch(c);
    dcn_scan_args sa = scan_args(c, idx, packed, invmask, v.stream_bases);
    sa.unit_tile_first = c->d_unit_tile_first;
    sa.unit_tile_count = c->d_unit_tile_count;
    sa.abs_threshold = params->abs_threshold;
    sa.rel_threshold = params->rel_threshold;
    sa.deplete = params->deplete;
    // decisions only: largest list length whose required hits still equal abs_threshold (dcn_required_hits is
    // monotone in the total); the scan kernel's lanes then stop at abs_threshold distinct hits (scan.hip)
    sa.early_out_max_items = 0;
    if (decisions_only_call) {
        uint32_t lo = 0, hi = 65535; // required(lo) == abs always holds for lo = 0
        while (lo < hi) {
            uint32_t mid = (lo + hi + 1) / 2;
            if (dcn_required_hits(params->abs_threshold, params->rel_threshold, mid) == params->abs_threshold) lo = mid;
            else hi = mid - 1;
        }
        sa.early_out_max_items = lo;
        sa.early_out_pairs = no_early_out_pairs ? 0u : 1u;
    }
    sa.keep = v.d_keep;
    sa.hits = v.d_hits;
    sa.total = v.d_total;
    sa.unit_state = c->d_unit_state;
    sa.g_total = us.g_total;
    sa.g_hitcnt = us.g_hitcnt;
    sa.g_zero = us.g_zero;
    sa.rec_hash = c->d_rec_hash;
    sa.rec_shift = c->rec_shift;
    sa.tile_windows = c->tile_windows;
    sa.tile_hits = c->d_tile_hits;
    sa.pending = c->d_pending;
    sa.status = c->d_status;
    sa.ascii = short_fused ? v.d_ascii : nullptr;
    sa.offsets = v.d_offsets;
    sa.n_reads = n_reads;
    sa.wave_kept = c->d_wave_kept;
    DCN_TRY(dcn_launch_scan(sa, tile_bound(c, n_reads, v.b1 - v.b0), false, st));
    DCN_PROF_MARK(DCN_STAGE_SCAN);

    const bool decisions_only = !v.d_hits && !v.d_total && !getenv("DCN_NO_EARLY_OUT");
    const dcn_distinct_args da = distinct_args(c, n_units, params, c->d_rec_hash, c->rec_shift, decisions_only ? us.g_total : nullptr);
    DCN_TRY(dcn_launch_distinct(da, st));
    DCN_PROF_MARK(DCN_STAGE_DISTINCT);

    dcn_finish_args fa = finish_args(c, n_units, params, v.d_unit_id ? c->d_unit_first_read : nullptr, v.d_offsets, v.d_keep,
                                     v.d_hits, v.d_total, v.d_report);
    fa.short_counted = short_fused ? 1u : 0u;
    fa.pending = c->d_pending;
    fa.wave_kept = c->d_wave_kept;
    DCN_TRY(dcn_launch_finish(fa, st));
    c->scratch_dirty = false;
    // the next pack into the buffer this batch read may start (a batch packed in line between packed-ahead ones -- per-stage
    // profiling -- read the first buffer)
    if (pack_ahead && c->pack_ahead_state == 1) DCN_HIP(hipEventRecord(c->buf_free[ahead_buf >= 0 ? ahead_buf : 0], st));
    DCN_PROF_MARK(DCN_STAGE_FINISH);
    if (prof_slot >= 0) c->prof_used[prof_slot] = true;
    return DCN_OK;
}

// a run overflowed (dcn_status::run_overflow): from now on the context keeps one slot of the record array per window
int grow_run_slots(dcn_ctx *c) {
    // (a batch that was in flight beside the one that made the context switch over reports the same overflow, from its
    // run under the old geometry: it is simply run again)
    if (c->rec_shift == 0) return DCN_OK;
    // The old array goes first (the caller has synchronized the stream: nothing reads it any more), so the peak is the
    // new 8 B per base and not 8 + 2: on a context sized close to the card the larger array alone may still fit.
    const bool in_slab = c->d_rec_hash && (char *)c->d_rec_hash >= c->d_slab && (char *)c->d_rec_hash < c->d_slab + c->slab_bytes;
    if (c->d_rec_hash && !in_slab) hipFree(c->d_rec_hash);
    c->d_rec_hash = nullptr;
    const uint32_t old_shift = c->rec_shift;
    c->rec_shift = 0;
    int rc = dev_alloc(&c->d_rec_hash, c->max_bases + 128, "rec_hash (one slot per window)");
    if (rc != DCN_OK) { // back to an array of the old geometry, so that the context stays usable for batches that fit it
        c->rec_shift = old_shift;
        int rc2 = dev_alloc(&c->d_rec_hash, (c->max_bases >> old_shift) + 256, "rec_hash");
        return rc2 != DCN_OK ? rc2 : rc;
    }
    static std::atomic<bool> said{false};
    if (!said.exchange(true) && getenv("DCN_QUIET") == nullptr)
        std::fprintf(stderr, "deacon-hip: a unit's hits outgrew its run of the record array; this context now keeps one slot per window "
                             "(%.2f GB instead of %.2f GB of device memory)\n", (c->max_bases + 128) * 8e-9,
                     ((c->max_bases >> old_shift) + 256) * 8e-9);
    return DCN_OK;
}

int overflow_error(const dcn_ctx *c, uint64_t need) {
    return dcn_fail(DCN_ERR_CAPACITY, "hit-record scratch overflow: need " + std::to_string(need) +
                                          " records, have " + std::to_string(c->rec_capacity) +
                                          " (dcn_ctx_reserve_records)");
}

// Wait for the compute stream and surface deferred errors of the device-pointer API.  The overflow word is
// sticky across batches (the per-run status words are not): an overflow in ANY batch enqueued since the last
// synchronize is reported here, however many smaller batches followed it.
int sync_and_check(dcn_ctx *c, uint64_t *needed_records) {
    DCN_HIP(hipStreamSynchronize(c->stream));
    if (needed_records) *needed_records = 0;
    if (c->profiling) DCN_TRY(prof_harvest(c));
    if (!c->batch_pending) return DCN_OK;
    c->batch_pending = false;
    DCN_HIP(hipMemcpy(c->h_report, c->d_report, sizeof(dcn_batch_report), hipMemcpyDeviceToHost));
    c->last_batch_short = c->h_report->short_batch != 0;
    if (c->h_report->bounds) {
        DCN_HIP(hipMemsetAsync(c->d_report, 0, offsetof(dcn_batch_report, stats), c->stream));
        return dcn_fail(DCN_ERR_INTERNAL, "scan kernel: index out of range in phase B (DCN_DEBUG_BOUNDS build)");
    }
    if (c->h_report->bad_offsets) {
        DCN_HIP(hipMemsetAsync(c->d_report, 0, offsetof(dcn_batch_report, stats), c->stream));
        return dcn_fail(DCN_ERR_ARG, "d_offsets of a batch since the last synchronize were not non-decreasing within [0, n_bases] when the "
                                     "device read them (were they written, and ordered before the context's stream, when "
                                     "dcn_filter_batch_device was called?): the outputs and counters of those batches are undefined");
    }
    if (c->h_report->overflow) {
        const uint64_t need = c->h_report->need;
        const bool runs = (c->h_report->overflow & 2u) != 0, sets = (c->h_report->overflow & 1u) != 0;
        DCN_HIP(hipMemsetAsync(c->d_report, 0, offsetof(dcn_batch_report, stats), c->stream)); // re-arm, ordered before the next batch
        if (runs) DCN_TRY(grow_run_slots(c)); // (the stream is idle: nothing reads the old array any more)
        if (needed_records) *needed_records = sets ? need : 0;
        if (!sets)
            return dcn_fail(DCN_ERR_CAPACITY, "a unit had more hits in one wave than its run of the record array holds; the context "
                                              "now keeps one slot per window: enqueue the batches since the last synchronize again");
        return overflow_error(c, need);
    }
    return DCN_OK;
}

// page-locked host memory (hipHostMalloc / hipHostRegister, e.g. from dcn_host_alloc) needs no staging
bool is_pinned_host(const void *p) {
    if (!p) return false;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError(); // plain malloc memory: not an error for us
        return false;
    }
    return attr.type == hipMemoryTypeHost;
}

// Copy `bytes` to the device on the copy stream.  Page-locked sources go straight over the link; anything else is
// cut into pieces that pass through the ring of pinned staging buffers (the host fills one while earlier ones are
// in flight).  `fill(dst, first, n)` produces bytes [first, first + n) of the payload in the staging buffer:
// a (threaded) memcpy, or the host-side 2-bit pack.
template <typename Fill>
static int staged_h2d_fill(dcn_ctx *c, void *d_dst, uint64_t bytes, uint64_t piece_align, Fill fill) {
    uint8_t *dst = (uint8_t *)d_dst;
    const uint64_t piece = c->stage_bytes / piece_align * piece_align;
    for (uint64_t off = 0; off < bytes; off += piece) {
        const int which = c->stage_next;
        c->stage_next = (which + 1) % dcn_ctx::N_STAGE;
        const uint64_t m = std::min<uint64_t>(piece, bytes - off);
        DCN_HIP(hipEventSynchronize(c->stage_free[which])); // previous copy out of this buffer finished
        fill(c->h_stage[which], off, m);
        DCN_HIP(hipMemcpyAsync(dst + off, c->h_stage[which], m, hipMemcpyHostToDevice, c->copy_stream));
        DCN_HIP(hipEventRecord(c->stage_free[which], c->copy_stream));
    }
    return DCN_OK;
}

int staged_h2d(dcn_ctx *c, void *d_dst, const void *h_src, uint64_t bytes, int pinned) {
    if (bytes == 0) return DCN_OK;
    if (pinned < 0) pinned = is_pinned_host(h_src) ? 1 : 0;
    if (pinned) {
        DCN_HIP(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, c->copy_stream));
        return DCN_OK;
    }
    const uint8_t *src = (const uint8_t *)h_src;
    return staged_h2d_fill(c, d_dst, bytes, 64, [&](uint8_t *stage, uint64_t first, uint64_t n) {
        HostPool::get().copy(stage, src + first, n);
    });
}


int slots_busy(const dcn_ctx *c) {
    int n = 0;
    for (const auto &sl : c->slots) n += sl.busy ? 1 : 0;
    return n;
}

// devices of this process that have a live context: the host pool is sized by them (HostPool::ensure_devices)
static std::mutex g_ctx_devices_mu;
static int g_ctx_per_device[64] = {0};
static void note_ctx_device(int device, int delta) {
    int n_devices = 0;
    {
        std::lock_guard<std::mutex> g(g_ctx_devices_mu);
        if (device >= 0 && device < 64) g_ctx_per_device[device] += delta;
        for (int d = 0; d < 64; ++d) n_devices += g_ctx_per_device[d] > 0;
    }
    if (delta > 0) HostPool::get().ensure_devices(n_devices);
}

// ---- argument checks shared by entry points ----
int check_idle(const dcn_ctx *c) {
    if (slots_busy(c) || c->batch_pending) return dcn_fail(DCN_ERR_ARG, "batches are in flight on this context: wait for them first");
    return DCN_OK;
}

int check_ctx_matches(const dcn_ctx *c, const dcn_index *other, const char *noun) {
    const dcn_index *ix = c->index;
    const std::string n = noun;
    if (ix->k != other->k || ix->w != other->w)
        return dcn_fail(DCN_ERR_ARG, "the context's index (k=" + std::to_string((int)ix->k) + ", w=" + std::to_string((int)ix->w) +
                                         ") and " + n + " (k=" + std::to_string((int)other->k) + ", w=" + std::to_string((int)other->w) +
                                         ") differ");
    if (ix->device != other->device) return dcn_fail(DCN_ERR_ARG, "the context and " + n + " live on different devices");
    if (ix->variant != other->variant)
        return dcn_fail(DCN_ERR_ARG, "the context's index and " + n + " were created under different minimizer rules");
    return check_idle(c);
}

int check_device_batch(const dcn_ctx *c, uint32_t n_reads, uint64_t n_bases, uint32_t n_units, const uint32_t *d_unit_id) {
    if (n_reads > c->max_reads) return dcn_fail(DCN_ERR_CAPACITY, "n_reads exceeds the context's max_batch_reads");
    if (n_bases > c->max_bases) return dcn_fail(DCN_ERR_CAPACITY, "n_bases exceeds the context's max_batch_bases");
    if (n_units == 0 || n_units > n_reads || (!d_unit_id && n_units != n_reads))
        return dcn_fail(DCN_ERR_ARG, "n_units inconsistent with n_reads / d_unit_id");
    return DCN_OK;
}

int check_offsets_walk(const uint64_t *offsets, uint32_t n, const char *noun, const char *too_long) {
    if (offsets[0] != 0) return dcn_fail(DCN_ERR_ARG, std::string(noun) + "[0] must be 0");
    for (uint32_t r = 0; r < n; ++r) {
        if (offsets[r + 1] < offsets[r]) return dcn_fail(DCN_ERR_ARG, std::string(noun) + " must be non-decreasing");
        if (offsets[r + 1] - offsets[r] > 0xFFFFFFF0ull) return dcn_fail(DCN_ERR_ARG, too_long);
    }
    return DCN_OK;
}

int validate_host_batch(const dcn_ctx *c, const uint64_t *offsets, uint32_t n_reads) {
    if (n_reads > c->max_reads) return dcn_fail(DCN_ERR_CAPACITY, "n_reads exceeds the context's max_batch_reads");
    DCN_TRY(check_idle(c));
    DCN_TRY(check_offsets_walk(offsets, n_reads, "offsets", "read longer than 2^32 bases"));
    if (offsets[n_reads] > c->max_bases) return dcn_fail(DCN_ERR_CAPACITY, "batch exceeds the context's max_batch_bases");
    return DCN_OK;
}

// ---- stage builders (dcn_ctx.h says what each leaves to its caller) ----
int ensure_dump_buffers(dcn_ctx *c) {
    if (c->d_dump_hash) return DCN_OK;
    DCN_TRY(dev_alloc(&c->d_dump_hash, c->max_bases + 2, "dump_hash"));
    DCN_TRY(dev_alloc(&c->d_dump_pos, c->max_bases + 2, "dump_pos"));
    DCN_TRY(dev_alloc(&c->d_dump_valid, c->max_bases + 2, "dump_valid"));
    DCN_TRY(dev_alloc(&c->d_dump_count, c->max_tiles, "dump_count"));
    return DCN_OK;
}

int ensure_position_bitmap(dcn_ctx *c) {
    if (c->d_loc_bits) return DCN_OK;
    return dev_alloc(&c->d_loc_bits, (c->max_bases + 31) / 32 + 1, "position bitmap");
}

int ensure_position_words(dcn_ctx *c) {
    if (c->d_loc_labels) return DCN_OK;
    return dev_alloc(&c->d_loc_labels, c->max_bases + 2, "position words");
}

UnitScratch unit_scratch(const dcn_ctx *c) {
    uint32_t *const s = c->d_unit_scratch;
    const uint64_t n = c->max_reads;
    return {s, s + n, s + 2 * n, s + 3 * n};
}

int stage_done(dcn_ctx *c) {
    DCN_HIP(hipEventRecord(c->copy_done, c->copy_stream));
    DCN_HIP(hipStreamWaitEvent(c->stream, c->copy_done, 0));
    return DCN_OK;
}

int stage_batch(dcn_ctx *c, const uint8_t *bases, uint64_t n_bases, const uint64_t *offsets, uint32_t n_reads,
                const uint32_t *unit_id_or_null) {
    DCN_TRY(staged_h2d(c, c->d_ascii, bases, n_bases));
    DCN_TRY(staged_h2d(c, c->d_offsets, offsets, (uint64_t)(n_reads + 1) * sizeof(uint64_t)));
    if (unit_id_or_null) DCN_TRY(staged_h2d(c, c->d_unit_id, unit_id_or_null, (uint64_t)n_reads * sizeof(uint32_t)));
    return stage_done(c);
}

dcn_plan_args plan_args(const dcn_ctx *c, const dcn_index *index, const uint8_t *d_ascii, const uint64_t *d_offsets,
                        const uint32_t *d_unit_id, uint32_t n_reads, uint32_t n_units, uint64_t prefix_length) {
    dcn_plan_args pa = {};
    pa.ascii = d_ascii;
    pa.offsets = d_offsets;
    pa.unit_id = d_unit_id;
    pa.n_reads = n_reads;
    pa.n_units = n_units;
    pa.k = index->k;
    pa.w = index->w;
    pa.prefix_length = prefix_length;
    pa.tile_windows = c->tile_windows;
    pa.unit_first_read = c->d_unit_first_read;
    pa.unit_tile_first = c->d_unit_tile_first;
    pa.unit_tile_count = c->d_unit_tile_count;
    pa.tile_cursor = &c->d_status->n_tiles;
    pa.tiles = c->d_tiles;
    pa.status = c->d_status;
    return pa;
}

// the fields of a scan that do not depend on its mode
static dcn_scan_args scan_args(const dcn_ctx *c, const dcn_index *index, uint32_t *packed, uint32_t *invmask, uint64_t stream_bases) {
    dcn_scan_args sa;
    memset(&sa, 0, sizeof(sa));
    sa.packed = packed;
    sa.invmask = invmask;
    sa.tiles = c->d_tiles;
    sa.n_tiles = &c->d_status->n_tiles;
    sa.table = index->view();
    sa.k = index->k;
    sa.variant = index->variant;
    sa.w = index->w;
    sa.stream_bases = stream_bases;
    sa.status = c->d_status;
    return sa;
}

dcn_scan_args dump_scan_args(const dcn_ctx *c, const dcn_index *index, uint64_t n_bases) {
    dcn_scan_args sa = scan_args(c, index, c->d_packed + DCN_FRONT_PAD, c->d_invmask + DCN_FRONT_PAD, n_bases);
    sa.dump_hash = c->d_dump_hash;
    sa.dump_pos = c->d_dump_pos;
    sa.dump_valid = c->d_dump_valid;
    sa.dump_count = c->d_dump_count;
    return sa;
}

uint32_t tile_bound(const dcn_ctx *c, uint32_t n_reads, uint64_t n_bases) {
    return (uint32_t)std::min<uint64_t>((uint64_t)n_reads + n_bases / c->tile_windows + 1, c->max_tiles);
}

dcn_dump_view dump_view(const dcn_ctx *c, uint32_t max_tiles, uint64_t n_bases) {
    dcn_dump_view v = {};
    v.tiles = c->d_tiles;
    v.n_tiles = &c->d_status->n_tiles;
    v.hash = c->d_dump_hash;
    v.valid = c->d_dump_valid;
    v.pos = c->d_dump_pos;
    v.count = c->d_dump_count;
    v.max_tiles = max_tiles;
    v.n_bases = n_bases;
    return v;
}

int dump_front_end(dcn_ctx *c, const dcn_index *index, const uint8_t *d_ascii, const uint64_t *d_offsets,
                   const uint32_t *d_unit_id, uint32_t n_reads, uint32_t n_units, uint64_t n_bases, uint64_t prefix_length,
                   bool plan_checks_offsets, int *prof_slot_out, dcn_dump_view *view) {
    hipStream_t st = c->stream;
    int prof_slot = -1;
    DCN_TRY(prof_begin(c, &prof_slot));
    *prof_slot_out = prof_slot;
    DCN_TRY(dcn_launch_pack(d_ascii, 0, n_bases, c->d_packed + DCN_FRONT_PAD, c->d_invmask + DCN_FRONT_PAD, c->d_status, st));
    DCN_PROF_MARK(DCN_STAGE_PACK);
    dcn_plan_args pa = plan_args(c, index, d_ascii, d_offsets, d_unit_id, n_reads, n_units, prefix_length);
    pa.read_tiles = c->d_read_tiles;
    pa.read_tile_first = c->d_read_tile_first;
    if (plan_checks_offsets) { // (else check_offsets stays 0: validate_host_batch has walked the offsets on the host)
        pa.stream_bases = n_bases;
        pa.check_offsets = 1;
        pa.max_tiles = c->max_tiles;
    }
    DCN_TRY(dcn_launch_plan(pa, st));
    DCN_PROF_MARK(DCN_STAGE_PLAN);
    dcn_scan_args sa = dump_scan_args(c, index, n_bases);
    sa.dump_abs = 1;
    const uint32_t max_tiles = tile_bound(c, n_reads, n_bases);
    DCN_TRY(dcn_launch_scan(sa, max_tiles, true, st));
    DCN_PROF_MARK(DCN_STAGE_SCAN);
    *view = dump_view(c, max_tiles, n_bases);
    return DCN_OK;
}

int record_run_end(dcn_ctx *c, int prof_slot) {
    if (prof_slot >= 0) c->prof_used[prof_slot] = true;
    // a later device-pointer filter batch packs one batch ahead into these packed buffers on its own stream, after the
    // events below: they now stand after this run
    if (c->pack_ahead_state == 1) {
        DCN_HIP(hipEventRecord(c->plan_done, c->stream));
        for (int i = 0; i < 2; ++i) DCN_HIP(hipEventRecord(c->buf_free[i], c->stream));
    }
    return DCN_OK;
}

int finish_run(dcn_ctx *c, int prof_slot) {
    DCN_TRY(record_run_end(c, prof_slot));
    return sync_and_check(c, nullptr);
}

dcn_distinct_args distinct_args(const dcn_ctx *c, uint32_t n_units, const dcn_params *params, const uint64_t *rec_hash,
                                uint32_t rec_shift, uint32_t *g_total_or_null) {
    const UnitScratch us = unit_scratch(c);
    dcn_distinct_args da = {};
    da.tiles = c->d_tiles;
    da.n_tiles = &c->d_status->n_tiles;
    da.unit_tile_first = c->d_unit_tile_first;
    da.unit_tile_count = c->d_unit_tile_count;
    da.unit_state = c->d_unit_state;
    da.tile_hits = c->d_tile_hits;
    da.pending = c->d_pending;
    da.rec_hash = rec_hash;
    da.rec_shift = rec_shift;
    da.g_hitcnt = us.g_hitcnt;
    da.g_distinct = us.g_distinct;
    da.set_off = c->d_set_off;
    da.set_slots = c->d_set_slots;
    da.set_capacity = 4 * c->rec_capacity + 64;
    da.n_units = n_units;
    da.status = c->d_status;
    da.caps = c->d_caps;
    da.big = c->d_big;
    da.g_total = g_total_or_null;
    da.abs_threshold = params->abs_threshold;
    da.rel_threshold = params->rel_threshold;
    return da;
}

dcn_finish_args finish_args(const dcn_ctx *c, uint32_t n_units, const dcn_params *params, const uint32_t *unit_first_read,
                            const uint64_t *offsets, uint8_t *keep, uint32_t *hits, uint32_t *total, dcn_batch_report *report) {
    const UnitScratch us = unit_scratch(c);
    dcn_finish_args fa = {};
    fa.n_units = n_units;
    fa.unit_first_read = unit_first_read;
    fa.offsets = offsets;
    fa.unit_state = c->d_unit_state;
    fa.g_total = us.g_total;
    fa.g_hitcnt = us.g_hitcnt;
    fa.g_distinct = us.g_distinct;
    fa.g_zero = us.g_zero;
    fa.abs_threshold = params->abs_threshold;
    fa.rel_threshold = params->rel_threshold;
    fa.deplete = params->deplete;
    fa.keep = keep;
    fa.hits = hits;
    fa.total = total;
    fa.report = report;
    fa.status = c->d_status;
    return fa;
}

} // namespace dcn_impl

using namespace dcn_impl;

extern "C" int dcn_ctx_create(const dcn_index *index, uint64_t max_batch_bases, uint32_t max_batch_reads,
                              dcn_ctx **out) {
    if (!out) return dcn_fail(DCN_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!index) return dcn_fail(DCN_ERR_ARG, "index is NULL");
    if (max_batch_bases == 0 || max_batch_reads == 0) return dcn_fail(DCN_ERR_ARG, "batch limits must be > 0");
    if (max_batch_reads > 0xFFFFFF00u) return dcn_fail(DCN_ERR_ARG, "max_batch_reads too large");
    dcn_ctx *c = new (std::nothrow) dcn_ctx();
    if (!c) return dcn_fail(DCN_ERR_NOMEM, "host allocation failed");
    c->index = index;
    c->device = index->device;
    c->max_bases = max_batch_bases;
    c->max_reads = max_batch_reads;
    if (const char *tw = getenv("DCN_TILE_WINDOWS")) {
        long v = strtol(tw, nullptr, 10);
        if (v >= 16 && v <= (long)DCN_MAX_TILE_WINDOWS) c->tile_windows = (uint32_t)v;
    }
    uint64_t mt = (uint64_t)max_batch_reads + max_batch_bases / c->tile_windows + 1;
    if (mt > 0xFFFFFF00ull) {
        delete c;
        return dcn_fail(DCN_ERR_ARG, "batch limits imply more than 2^32 tiles");
    }
    c->max_tiles = (uint32_t)mt;
    c->chunk_bases = 64ull << 20;
    if (const char *cb = getenv("DCN_CHUNK_BASES")) {
        long long v = atoll(cb);
        if (v >= 1024) c->chunk_bases = (uint64_t)v;
    }
    int rc = DCN_OK;
    auto fail = [&](int code) {
        free_ctx(c);
        return code;
    };
    if (hipSetDevice(c->device) != hipSuccess) return fail(dcn_fail(DCN_ERR_HIP, "hipSetDevice failed"));
    bool ok = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess &&
              hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking) == hipSuccess &&
              hipStreamCreateWithFlags(&c->d2h_stream, hipStreamNonBlocking) == hipSuccess &&
              hipEventCreateWithFlags(&c->copy_done, hipEventDisableTiming) == hipSuccess;
    for (int i = 0; ok && i < dcn_ctx::N_STAGE; ++i)
        ok = hipEventCreateWithFlags(&c->stage_free[i], hipEventDisableTiming) == hipSuccess;
    for (int i = 0; ok && i < dcn_ctx::N_EV; ++i)
        ok = hipEventCreateWithFlags(&c->ev_h2d[i], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&c->ev_comp[i], hipEventDisableTiming) == hipSuccess;
    if (!ok) return fail(dcn_fail(DCN_ERR_HIP, "stream/event creation failed"));
    // Runs of the record array: one slot per four windows (2 B per base of the batch instead of 8).  A unit would need a hit
    // in more than every fourth window of a wave to fill its run -- real sequence has a minimizer in every eighth -- and a
    // batch that does (w = 1, say) is run again with one slot per window (grow_run_slots).  DCN_REC_SHIFT = 0..3 fixes it.
    c->rec_shift = 2;
    // ... unless the index's window makes that likely from the start: the density of minimizers is 2 / (w + 1), and low-
    // complexity sequence ties its way to a hit in every window or two (leftmost / rightmost alternate); from w <= 7 on
    // (2 / (w + 1) >= 1/4) the context starts with one slot per window instead of finding out in mid-run
    if (index->w <= 7) c->rec_shift = 0;
    c->short_fused = getenv("DCN_NO_SHORT_FUSED") == nullptr; // (A/B baseline and escape hatch: every batch takes the classic path)
    if (const char *rs = getenv("DCN_REC_SHIFT")) c->rec_shift = (uint32_t)std::min(3, std::max(0, atoi(rs)));
    uint64_t MR = max_batch_reads;
    // DCN_CTX_SLAB=1 (experiment, profiles/placement_order.py): the fixed-size buffers below come out of ONE allocation,
    // each on a 2 MB boundary, instead of 24 separate ones
    const bool slab = getenv("DCN_CTX_SLAB") != nullptr;
    uint64_t slab_off = 0;
    for (int pass = slab ? 0 : 1; pass < 2; ++pass) {
        if (slab && pass == 1) {
            c->slab_bytes = slab_off;
            if (hipMalloc((void **)&c->d_slab, c->slab_bytes) != hipSuccess) {
                c->d_slab = nullptr;
                c->slab_bytes = 0;
                return fail(dcn_fail(DCN_ERR_NOMEM, "hipMalloc of the context slab failed"));
            }
            slab_off = 0;
        }
#define A(ptr, count, what)                                                                                   \
    if (slab) {                                                                                               \
        if (pass == 1) c->ptr = reinterpret_cast<decltype(c->ptr)>(c->d_slab + slab_off);                     \
        slab_off += (std::max<uint64_t>((count), 1) * sizeof(*c->ptr) + (2u << 20) - 1) / (2u << 20) * (2u << 20); \
    } else if ((rc = dev_alloc(&c->ptr, (count), what)) != DCN_OK)                                            \
        return fail(rc)
    A(d_ascii, max_batch_bases + 64, "ascii");
    A(d_offsets, MR + 1, "offsets");
    A(d_unit_id, MR, "unit_id");
    A(d_packed, packed_words(max_batch_bases), "packed");
    A(d_invmask, mask_words(max_batch_bases), "invmask");
    A(d_read_tiles, MR, "read_tiles");
    A(d_read_tile_first, MR + 1, "read_tile_first");
    A(d_unit_first_read, MR + 1, "unit_first_read");
    A(d_unit_tile_first, MR + 1, "unit_tile_first");
    A(d_unit_tile_count, MR + 1, "unit_tile_count");
    A(d_tiles, mt, "tiles");
    A(d_keep, MR, "keep");
    A(d_unit_state, MR, "unit_state");
    A(d_hits, MR, "hits");
    A(d_total, MR, "total");
    A(d_unit_scratch, MR * 4, "unit_scratch");
    A(d_caps, MR, "caps");
    A(d_set_off, MR + 1, "set_off");
    A(d_tile_hits, mt, "tile_hits");
    A(d_pending, MR, "pending");
    A(d_big, MR + mt / 64 + 1, "big");
    A(d_rec_hash, (max_batch_bases >> c->rec_shift) + 256, "rec_hash");
    A(d_status, 1, "status");
    A(d_wave_kept, MR / DCN_WAVE + 1, "wave_kept");
    A(d_report, 1, "report");
#undef A
    }
    // global sets of the distinct pass (only units with more hits than its LDS set holds use them): sized for the
    // expected long-read density, grown on demand by the host API / dcn_ctx_reserve_records
    uint64_t recs = std::min<uint64_t>(std::max<uint64_t>(max_batch_bases / 16, 1u << 16), 1ull << 29);
    if (const char *rc_env = getenv("DCN_RECORD_CAPACITY")) recs = std::min<uint64_t>(std::max<uint64_t>(strtoull(rc_env, nullptr, 10), 64), 1ull << 29); // tests: force the growth path
    if ((rc = alloc_records(c, recs)) != DCN_OK) return fail(rc);
    c->stage_bytes = std::min<uint64_t>(std::max<uint64_t>(max_batch_bases + 64, 4096), 32ull << 20);
    if (const char *sb = getenv("DCN_STAGE_BYTES")) // tests: small staging buffers, so that one chunk needs many pieces
        c->stage_bytes = std::min<uint64_t>(std::max<uint64_t>(strtoull(sb, nullptr, 10), 4096), 32ull << 20);
    for (int i = 0; i < dcn_ctx::N_STAGE; ++i)
        if (hipHostMalloc((void **)&c->h_stage[i], c->stage_bytes, hipHostMallocDefault) != hipSuccess)
            return fail(dcn_fail(DCN_ERR_NOMEM, "pinned staging allocation failed"));
    if (hipHostMalloc((void **)&c->h_report, sizeof(dcn_batch_report), hipHostMallocDefault) != hipSuccess)
        return fail(dcn_fail(DCN_ERR_NOMEM, "pinned status allocation failed"));
    // zero padding in front of / behind the packed stream is written once; pack only touches the middle
    if (hipMemset(c->d_packed, 0, packed_words(max_batch_bases) * sizeof(uint32_t)) != hipSuccess ||
        hipMemset(c->d_invmask, 0, mask_words(max_batch_bases) * sizeof(uint32_t)) != hipSuccess ||
        hipMemset(c->d_status, 0, sizeof(dcn_status)) != hipSuccess ||
        hipMemset(c->d_unit_scratch, 0, (uint64_t)max_batch_reads * 4 * sizeof(uint32_t)) != hipSuccess ||
        hipMemset(c->d_report, 0, sizeof(dcn_batch_report)) != hipSuccess ||
        // hipMemset runs on the null stream and does not wait for the host; the context's streams are non-blocking
        // and do not wait for the null stream: without this, the first batch's copies into the packed stream can
        // be overtaken by the memset above (seen as an all-'A' first chunk, once in a few hundred runs)
        hipDeviceSynchronize() != hipSuccess)
        return fail(dcn_fail(DCN_ERR_HIP, "hipMemset failed"));
    note_ctx_device(c->device, +1);
    *out = c;
    return DCN_OK;
}

extern "C" void dcn_ctx_destroy(dcn_ctx *ctx) {
    if (ctx) note_ctx_device(ctx->device, -1);
    free_ctx(ctx);
}

extern "C" void *dcn_ctx_stream(dcn_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

extern "C" int dcn_ctx_reserve_records(dcn_ctx *ctx, uint64_t n_records) {
    if (!ctx) return dcn_fail(DCN_ERR_ARG, "ctx is NULL");
    if (slots_busy(ctx)) return dcn_fail(DCN_ERR_ARG, "host batches are in flight: wait for them first");
    DCN_HIP(hipSetDevice(ctx->device));
    DCN_HIP(hipStreamSynchronize(ctx->stream));
    if (n_records <= ctx->rec_capacity) return DCN_OK;
    return alloc_records(ctx, n_records);
}

extern "C" int dcn_ctx_last_batch_short(dcn_ctx *ctx, uint32_t *was_short) {
    if (!ctx || !was_short) return dcn_fail(DCN_ERR_ARG, "ctx/was_short is NULL");
    *was_short = ctx->last_batch_short ? 1u : 0u;
    return DCN_OK;
}

extern "C" int dcn_ctx_synchronize(dcn_ctx *ctx) {
    if (!ctx) return dcn_fail(DCN_ERR_ARG, "ctx is NULL");
    DCN_HIP(hipSetDevice(ctx->device));
    return sync_and_check(ctx, nullptr);
}

extern "C" int dcn_filter_batch_device(dcn_ctx *ctx, const uint8_t *d_bases, const uint64_t *d_offsets,
                                       const uint32_t *d_unit_id, uint32_t n_reads, uint64_t n_bases,
                                       uint32_t n_units, const dcn_params *params, uint8_t *d_keep, uint32_t *d_hits,
                                       uint32_t *d_total) {
    if (!ctx) return dcn_fail(DCN_ERR_ARG, "ctx is NULL");
    DCN_TRY(check_params(params));
    if (n_reads == 0) return DCN_OK;
    if (!d_bases || !d_offsets || !d_keep) return dcn_fail(DCN_ERR_ARG, "d_bases/d_offsets/d_keep is NULL");
    DCN_TRY(check_device_batch(ctx, n_reads, n_bases, n_units, d_unit_id));
    // the packed stream of slot 0 is this path's pack target and a host batch's copy target
    if (ctx->slots[0].busy) return dcn_fail(DCN_ERR_ARG, "a host batch is in flight on this context: wait for it first");
    DCN_HIP(hipSetDevice(ctx->device));
    BatchView v;
    v.d_ascii = d_bases;
    v.d_packed = ctx->d_packed;
    v.d_invmask = ctx->d_invmask;
    v.d_offsets = d_offsets;
    v.d_unit_id = d_unit_id;
    v.n_reads = n_reads;
    v.n_units = n_units;
    v.b0 = 0;
    v.b1 = n_bases;
    v.stream_bases = n_bases;
    v.d_keep = d_keep;
    v.d_hits = d_hits;
    v.d_total = d_total;
    v.d_report = ctx->d_report;
    DCN_TRY(enqueue_batch(ctx, v, params, /*pack_ahead=*/true));
    ctx->batch_pending = true;
    return DCN_OK;
}

extern "C" int dcn_ctx_set_profiling(dcn_ctx *ctx, int enable) {
    if (!ctx) return dcn_fail(DCN_ERR_ARG, "ctx is NULL");
    DCN_HIP(hipSetDevice(ctx->device));
    DCN_HIP(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < dcn_ctx::PROF_RING; ++i) ctx->prof_used[i] = false;
    for (int j = 0; j < DCN_N_STAGES; ++j) ctx->prof_ms[j] = 0.0;
    ctx->prof_batches = 0;
    ctx->profiling = enable == 2 ? 2 : (enable != 0 ? 1 : 0);
    return DCN_OK;
}

extern "C" int dcn_ctx_profile(dcn_ctx *ctx, double stage_ms[DCN_N_STAGES], uint64_t *n_batches) {
    if (!ctx || !stage_ms) return dcn_fail(DCN_ERR_ARG, "ctx/stage_ms is NULL");
    if (ctx->profiling) { // waits for the runs marked so far
        DCN_HIP(hipSetDevice(ctx->device));
        DCN_TRY(prof_harvest(ctx));
    }
    for (int j = 0; j < DCN_N_STAGES; ++j) stage_ms[j] = ctx->prof_ms[j];
    if (n_batches) *n_batches = ctx->prof_batches;
    return DCN_OK;
}

// counters = completed host batches (summed on the host when each batch is waited for) + everything the
// device-pointer API has enqueued (accumulated on the device)
extern "C" int dcn_ctx_stats(dcn_ctx *ctx, uint64_t counters[DCN_N_STATS]) {
    if (!ctx || !counters) return dcn_fail(DCN_ERR_ARG, "ctx/counters is NULL");
    DCN_HIP(hipSetDevice(ctx->device));
    DCN_HIP(hipStreamSynchronize(ctx->stream));
    DCN_HIP(hipMemcpy(ctx->h_report, ctx->d_report, sizeof(dcn_batch_report), hipMemcpyDeviceToHost));
    for (int i = 0; i < DCN_N_STATS; ++i) counters[i] = ctx->h_report->stats[i] + ctx->host_stats[i];
    return DCN_OK;
}

extern "C" int dcn_ctx_reset_stats(dcn_ctx *ctx) {
    if (!ctx) return dcn_fail(DCN_ERR_ARG, "ctx is NULL");
    DCN_HIP(hipSetDevice(ctx->device));
    DCN_HIP(hipStreamSynchronize(ctx->stream));
    DCN_HIP(hipMemsetAsync(ctx->d_report->stats, 0, sizeof(unsigned long long) * DCN_N_STATS, ctx->stream));
    DCN_HIP(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < DCN_N_STATS; ++i) ctx->host_stats[i] = 0;
    return DCN_OK;
}

// Sum of the six counters over several contexts: the merge the reference does when its worker threads finish
// (ProcessingStats, src/local_filter.rs:388-396).  All contexts live in this process, one per device or several per
// device, so the sum is taken on the host; ranks in separate processes reduce with RCCL instead.
extern "C" int dcn_stats_allreduce(dcn_ctx *const *ctxs, int n_ctx, uint64_t counters[DCN_N_STATS]) {
    if (!counters || (n_ctx > 0 && !ctxs) || n_ctx < 0) return dcn_fail(DCN_ERR_ARG, "ctxs/counters is NULL");
    for (int i = 0; i < DCN_N_STATS; ++i) counters[i] = 0;
    for (int j = 0; j < n_ctx; ++j) {
        uint64_t one[DCN_N_STATS];
        DCN_TRY(dcn_ctx_stats(ctxs[j], one));
        for (int i = 0; i < DCN_N_STATS; ++i) counters[i] += one[i];
    }
    return DCN_OK;
}

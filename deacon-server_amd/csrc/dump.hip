// dump.hip -- the entry points that run "pack -> plan -> scan in dump mode" or probe precomputed hashes on a context:
// the minimizer dump (parity / debugging seam), the server's hash seam and the GPU index build.
#include "dcn_ctx.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace dcn_impl;

// ----------------------------------------------------------------------------------------------------
// minimizer dump (parity / debugging seam)
// ----------------------------------------------------------------------------------------------------
extern "C" int dcn_minimizer_hashes_batch(dcn_ctx *ctx, const uint8_t *bases, const uint64_t *offsets,
                                          uint32_t n_reads, uint64_t prefix_length, uint64_t *out_offsets,
                                          uint64_t *out_hashes, uint32_t *out_positions, uint64_t capacity) {
    if (!ctx || !out_offsets) return dcn_fail(DCN_ERR_ARG, "ctx/out_offsets is NULL");
    out_offsets[0] = 0;
    if (n_reads == 0) return DCN_OK;
    if (!offsets) return dcn_fail(DCN_ERR_ARG, "offsets is NULL");
    DCN_TRY(validate_host_batch(ctx, offsets, n_reads));
    uint64_t n_bases = offsets[n_reads];
    if (n_bases > 0 && !bases) return dcn_fail(DCN_ERR_ARG, "bases is NULL");
    dcn_ctx *c = ctx;
    DCN_HIP(hipSetDevice(c->device));
    DCN_TRY(ensure_dump_buffers(c));
    if (!c->d_tile_read_pos) DCN_TRY(dev_alloc(&c->d_tile_read_pos, c->max_tiles, "tile_read_pos"));
    DCN_TRY(stage_batch(c, bases, n_bases, offsets, n_reads, nullptr));
    hipStream_t st = c->stream;
    DCN_HIP(hipMemsetAsync(c->d_status, 0, sizeof(dcn_status), st));
    DCN_TRY(dcn_launch_pack(c->d_ascii, 0, n_bases, c->d_packed + DCN_FRONT_PAD, c->d_invmask + DCN_FRONT_PAD, c->d_status, st));
    // (check_offsets stays 0: validate_host_batch has walked the offsets on the host)
    dcn_plan_args pa = plan_args(c, c->index, c->d_ascii, c->d_offsets, nullptr, n_reads, n_reads, prefix_length);
    pa.read_tiles = c->d_read_tiles;
    pa.read_tile_first = c->d_read_tile_first;
    pa.tile_read_pos = c->d_tile_read_pos;
    DCN_TRY(dcn_launch_plan(pa, st));
    dcn_scan_args sa = dump_scan_args(c, c->index, n_bases);
    sa.tile_read_pos = c->d_tile_read_pos; // positions in the read, not dump_abs
    DCN_TRY(dcn_launch_scan(sa, tile_bound(c, n_reads, n_bases), true, st));
    DCN_HIP(hipStreamSynchronize(st));
    // gather on the host: tiles are in read order, a tile's entries sit at [first own window's absolute
    // base index ...) in emit order; entries failing the ACGT test are dropped (src/filter_common.rs:275-286)
    std::vector<uint32_t> rtf(n_reads), rtn(n_reads);
    DCN_HIP(hipMemcpy(rtf.data(), c->d_read_tile_first, (uint64_t)n_reads * sizeof(uint32_t), hipMemcpyDeviceToHost));
    DCN_HIP(hipMemcpy(rtn.data(), c->d_read_tiles, (uint64_t)n_reads * sizeof(uint32_t), hipMemcpyDeviceToHost));
    uint32_t nt = 0;
    DCN_HIP(hipMemcpy(&nt, &c->d_status->n_tiles, sizeof(uint32_t), hipMemcpyDeviceToHost));
    std::vector<dcn_tile> tiles(nt);
    std::vector<uint32_t> tcount(nt);
    std::vector<uint64_t> h(n_bases + 2);
    std::vector<uint32_t> p(n_bases + 2);
    std::vector<uint8_t> v(n_bases + 2);
    if (nt) {
        DCN_HIP(hipMemcpy(tiles.data(), c->d_tiles, (uint64_t)nt * sizeof(dcn_tile), hipMemcpyDeviceToHost));
        DCN_HIP(hipMemcpy(tcount.data(), c->d_dump_count, (uint64_t)nt * sizeof(uint32_t), hipMemcpyDeviceToHost));
        DCN_HIP(hipMemcpy(h.data(), c->d_dump_hash, (n_bases + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
        DCN_HIP(hipMemcpy(p.data(), c->d_dump_pos, (n_bases + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
        DCN_HIP(hipMemcpy(v.data(), c->d_dump_valid, (n_bases + 1), hipMemcpyDeviceToHost));
    }
    uint64_t n_out = 0;
    for (uint32_t r = 0; r < n_reads; ++r) {
        for (uint32_t t = rtf[r]; t < rtf[r] + rtn[r]; ++t) {
            uint64_t base = tiles[t].scan_start + tiles[t].carry();
            for (uint32_t e = 0; e < tcount[t]; ++e) {
                if (!v[base + e]) continue;
                if (n_out < capacity) {
                    if (out_hashes) out_hashes[n_out] = h[base + e];
                    if (out_positions) out_positions[n_out] = p[base + e];
                }
                n_out++;
            }
        }
        out_offsets[r + 1] = n_out;
    }
    if (n_out > capacity) return dcn_fail(DCN_ERR_CAPACITY, "output capacity too small: need " + std::to_string(n_out));
    return DCN_OK;
}

// ----------------------------------------------------------------------------------------------------
// server batch seam: hashes precomputed (src/remote_filter.rs:230-301)
// ----------------------------------------------------------------------------------------------------
extern "C" int dcn_should_keep_hashes(dcn_ctx *ctx, const uint64_t *hashes, const uint64_t *hash_offsets,
                                      uint32_t n_units, const dcn_params *params, uint8_t *keep, uint32_t *hits,
                                      uint32_t *total) {
    if (!ctx) return dcn_fail(DCN_ERR_ARG, "ctx is NULL");
    DCN_TRY(check_params(params));
    if (n_units == 0) return DCN_OK;
    if (!hash_offsets || !keep) return dcn_fail(DCN_ERR_ARG, "hash_offsets/keep is NULL");
    if (n_units > ctx->max_reads) return dcn_fail(DCN_ERR_CAPACITY, "n_units exceeds the context's max_batch_reads");
    DCN_TRY(check_idle(ctx));
    DCN_TRY(check_offsets_walk(hash_offsets, n_units, "hash_offsets", "unit has more than 2^32 hashes"));
    uint64_t n_hashes = hash_offsets[n_units];
    if (n_hashes > 0 && !hashes) return dcn_fail(DCN_ERR_ARG, "hashes is NULL");
    dcn_ctx *c = ctx;
    DCN_HIP(hipSetDevice(c->device));
    // a unit with more hashes than the LDS set of the distinct pass holds takes a global set of <= 4 slots per hash
    if (n_hashes > c->rec_capacity) DCN_TRY(dcn_ctx_reserve_records(c, std::min<uint64_t>(n_hashes, 1ull << 29)));
    if (n_hashes > c->rec_capacity) return dcn_fail(DCN_ERR_CAPACITY, "too many hashes in one call");
    uint64_t *d_hashes = nullptr, *d_hoff = nullptr;
    DCN_TRY(dev_alloc(&d_hashes, n_hashes, "hashes"));
    int rc = dev_alloc(&d_hoff, (uint64_t)n_units + 1, "hash_offsets");
    if (rc != DCN_OK) {
        hipFree(d_hashes);
        return rc;
    }
    auto body = [&]() -> int {
        hipStream_t st = c->stream;
        DCN_HIP(hipMemcpyAsync(d_hashes, hashes, n_hashes * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        DCN_HIP(hipMemcpyAsync(d_hoff, hash_offsets, ((uint64_t)n_units + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        DCN_HIP(hipMemsetAsync(c->d_status, 0, sizeof(dcn_status), st));
        const UnitScratch us = unit_scratch(c);
        dcn_probe_hashes_args ha;
        ha.table = c->index->view();
        ha.hashes = d_hashes;
        ha.hash_offsets = d_hoff;
        ha.n_hashes = n_hashes;
        ha.n_units = n_units;
        ha.tiles = c->d_tiles;
        ha.n_tiles = &c->d_status->n_tiles;
        ha.tile_hits = c->d_tile_hits;
        ha.unit_tile_first = c->d_unit_tile_first;
        ha.unit_tile_count = c->d_unit_tile_count;
        ha.pending = c->d_pending;
        ha.unit_state = c->d_unit_state;
        ha.g_total = us.g_total;
        ha.g_hitcnt = us.g_hitcnt;
        ha.g_distinct = us.g_distinct;
        ha.g_zero = us.g_zero;
        ha.status = c->d_status;
        DCN_TRY(dcn_launch_probe_hashes(ha, st));
        // the hashes are their own runs, one slot each; every hit is counted (the server's answer carries the hit
        // count: src/server_common.rs:54-58)
        DCN_TRY(dcn_launch_distinct(distinct_args(c, n_units, params, d_hashes, 0, nullptr), st));
        // no unit_first_read (unit == entry) and no offsets (no read lengths here: the counters are untouched)
        DCN_TRY(dcn_launch_finish(finish_args(c, n_units, params, nullptr, nullptr, c->d_keep, c->d_hits, c->d_total, c->d_report), st));
        c->batch_pending = true;
        DCN_TRY(sync_and_check(c, nullptr));
        DCN_HIP(hipMemcpy(keep, c->d_keep, n_units, hipMemcpyDeviceToHost));
        if (hits) DCN_HIP(hipMemcpy(hits, c->d_hits, (uint64_t)n_units * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (total) DCN_HIP(hipMemcpy(total, c->d_total, (uint64_t)n_units * sizeof(uint32_t), hipMemcpyDeviceToHost));
        return DCN_OK;
    };
    rc = body();
    hipStreamSynchronize(c->stream);
    hipFree(d_hashes);
    hipFree(d_hoff);
    return rc;
}

// ----------------------------------------------------------------------------------------------------
// index build (f1): chunks of sequence pieces -> pack (index-side codes) -> plan -> scan in dump mode -> insert
// ----------------------------------------------------------------------------------------------------
uint64_t dcn_impl::build_chunk_bases() {
    uint64_t chunk_bases = 1ull << 27;
    if (const char *cb = getenv("DCN_BUILD_CHUNK_BASES")) {
        long long v = atoll(cb);
        if (v >= 4096) chunk_bases = (uint64_t)v;
    }
    return chunk_bases;
}

// DCN_INDEX_TIMING (dcn_ctx.h)
double dcn_impl::build_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int dcn_impl::build_timing_begin(dcn_ctx *c) { return dcn_ctx_set_profiling(c, 1); }

int dcn_impl::build_times_print(const char *which, dcn_ctx *c, const build_times &t) {
    double ms[DCN_N_STAGES] = {};
    uint64_t chunks = 0;
    DCN_TRY(dcn_ctx_profile(c, ms, &chunks));
    fprintf(stderr,
            "index build timing (%s): front end made %.3f s; %llu chunks: staging %.3f s, pack %.1f ms, plan %.1f ms, "
            "scan %.1f ms, sweep %.1f ms (of it growth %.3f s); finish %.3f s (of it its table made %.3f s)\n",
            which, t.front_end_s, (unsigned long long)chunks, t.staging_s, ms[DCN_STAGE_PACK], ms[DCN_STAGE_PLAN],
            ms[DCN_STAGE_SCAN], ms[DCN_STAGE_DISTINCT], t.growth_s, t.finish_s, t.finish_table_s);
    return DCN_OK;
}

// The front end of both index builds on a dump-mode context of chunk_bases bases and DCN_BUILD_MAX_PIECES reads: after
// each chunk's scan, sweep(nb, continues) sees the chunk's dump (nb bases; dump_abs = 1) on c->stream.  `continues`: the
// chunk's first piece continues the piece that ended the chunk before it (the same sequence, l-1 bases further back).
int dcn_impl::build_run_chunks(dcn_ctx *c, const dcn_index *idx, const uint8_t *bases, const uint64_t *offsets, uint32_t n_seqs,
                               uint64_t chunk_bases, const build_sweep_fn &sweep, build_times *times) {
    if (n_seqs == 0) return DCN_OK;
    if (offsets[0] != 0) return dcn_fail(DCN_ERR_ARG, "offsets[0] must be 0");
    const uint32_t k = idx->k, l = (uint32_t)idx->k + idx->w - 1;
    // a piece is a range of one sequence; a sequence longer than the chunk is cut into pieces overlapping by
    // l-1 bases, which yields every window exactly once (an extra duplicate at a seam merges in the set)
    const uint32_t max_pieces = DCN_BUILD_MAX_PIECES;
    DCN_TRY(ensure_dump_buffers(c));
    std::vector<uint64_t> p_off;   // offsets of the pieces inside the chunk buffer
    std::vector<const uint8_t *> p_src;
    std::vector<uint64_t> p_len;
    bool continues = false;
    auto run_chunk = [&]() -> int {
        if (p_len.empty()) return DCN_OK;
        uint32_t np = (uint32_t)p_len.size();
        p_off.assign(np + 1, 0);
        for (uint32_t i = 0; i < np; ++i) p_off[i + 1] = p_off[i] + p_len[i];
        uint64_t nb = p_off[np];
        const double t_stage = times ? build_now() : 0.0;
        // pieces that follow each other in the caller's memory (the reads of a batch) cross as one copy: one copy per
        // 150-base read was the whole build of a read set
        for (uint32_t i = 0; i < np;) {
            uint32_t j = i + 1;
            while (j < np && p_src[j] == p_src[j - 1] + p_len[j - 1]) ++j;
            DCN_TRY(staged_h2d(c, c->d_ascii + p_off[i], p_src[i], p_off[j] - p_off[i]));
            i = j;
        }
        DCN_TRY(staged_h2d(c, c->d_offsets, p_off.data(), (uint64_t)(np + 1) * sizeof(uint64_t)));
        DCN_TRY(stage_done(c));
        if (times) {
            DCN_HIP(hipEventSynchronize(c->copy_done));
            times->staging_s += build_now() - t_stage;
        }
        hipStream_t st = c->stream;
        int prof_slot = -1;
        DCN_TRY(prof_begin(c, &prof_slot));
        DCN_HIP(hipMemsetAsync(c->d_status, 0, sizeof(dcn_status), st));
        DCN_HIP(hipMemsetAsync(c->d_dump_valid, 0, nb + 2, st));
        // no status word for the pack (a newline is not looked for), the index side's code table
        DCN_TRY(dcn_launch_pack(c->d_ascii, 0, nb, c->d_packed + DCN_FRONT_PAD, c->d_invmask + DCN_FRONT_PAD, nullptr, st,
                                /*index_side=*/true));
        DCN_PROF_MARK(DCN_STAGE_PACK);
        // (check_offsets stays 0: the pieces' offsets were made right here)
        dcn_plan_args pa = plan_args(c, idx, c->d_ascii, c->d_offsets, nullptr, np, np, 0);
        pa.read_tiles = c->d_read_tiles;
        pa.read_tile_first = c->d_read_tile_first;
        DCN_TRY(dcn_launch_plan(pa, st));
        DCN_PROF_MARK(DCN_STAGE_PLAN);
        dcn_scan_args sa = dump_scan_args(c, idx, nb);
        sa.dump_abs = 1; // positions in the chunk: the sweeps read the bases around them
        DCN_TRY(dcn_launch_scan(sa, tile_bound(c, np, nb), true, st));
        DCN_PROF_MARK(DCN_STAGE_SCAN);
        DCN_TRY(sweep(nb, continues));
        DCN_PROF_MARK(DCN_STAGE_DISTINCT); // (the sweep's slot; nothing follows it)
        DCN_PROF_MARK(DCN_STAGE_FINISH);
        if (prof_slot >= 0) c->prof_used[prof_slot] = true;
        p_src.clear();
        p_len.clear();
        return DCN_OK;
    };
    uint64_t used = 0;
    for (uint32_t sidx = 0; sidx < n_seqs; ++sidx) {
        if (offsets[sidx + 1] < offsets[sidx]) return dcn_fail(DCN_ERR_ARG, "offsets must be non-decreasing");
        const uint8_t *seq = bases + offsets[sidx];
        uint64_t len = offsets[sidx + 1] - offsets[sidx];
        if (len < k || len < l) continue; // src/minimizers.rs:135; fewer than l bases have no window
        uint64_t a = 0;
        while (a + l <= len) {
            uint64_t room = chunk_bases - used;
            if (room < l || p_len.size() >= max_pieces) {
                DCN_TRY(run_chunk());
                continues = a > 0; // (a cut piece fills its chunk: the piece at a > 0 that opens a chunk continues it)
                used = 0;
                room = chunk_bases;
            }
            uint64_t take = std::min<uint64_t>(room, len - a);
            if (take > 0xFFFFFF00ull) take = 0xFFFFFF00ull;
            p_src.push_back(seq + a);
            p_len.push_back(take);
            used += take;
            if (a + take >= len) break;
            a += take - (l - 1); // next piece starts l-1 bases before the cut
        }
    }
    return run_chunk();
}

int dcn_build_index_impl(const uint8_t *bases, const uint64_t *offsets, uint32_t n_seqs, float entropy_threshold,
                         dcn_index *idx) {
    if (n_seqs == 0) return DCN_OK;
    const uint64_t chunk_bases = build_chunk_bases();
    const bool timing = getenv("DCN_INDEX_TIMING") != nullptr;
    build_times times;
    dcn_ctx *c = nullptr;
    double t0 = build_now();
    DCN_TRY(dcn_ctx_create(idx, chunk_bases, DCN_BUILD_MAX_PIECES, &c));
    times.front_end_s = build_now() - t0;
    int rc = timing ? build_timing_begin(c) : DCN_OK;
    if (rc == DCN_OK)
        rc = build_run_chunks(c, idx, bases, offsets, n_seqs, chunk_bases, [&](uint64_t nb, bool) -> int {
            uint64_t n_valid = 0;
            DCN_TRY(dcn_table_count_valid(c->d_dump_valid, nb, &n_valid, c->stream));
            const double t_grow = build_now();
            DCN_TRY(dcn_table_reserve(idx, idx->n_keys + n_valid));
            times.growth_s += build_now() - t_grow;
            return dcn_table_insert_dump(idx, c->d_dump_hash, c->d_dump_valid, c->d_dump_pos, nb, c->d_ascii, entropy_threshold,
                                         c->stream);
        }, timing ? &times : nullptr);
    // (the events are read before the context goes; what freeing it costs is printed by itself)
    if (timing && rc == DCN_OK) rc = build_times_print("plain", c, times);
    t0 = build_now();
    dcn_ctx_destroy(c);
    if (timing) fprintf(stderr, "index build timing (plain): front end freed %.3f s\n", build_now() - t0);
    return rc;
}

// host_batch.hip -- host batches of the C ABI: dcn_filter_batch[_packed][_submit] / dcn_filter_batch_wait.  A batch is cut
// into chunks whose payload crosses the link on the copy stream (as ASCII, packed by the host threads, or packed by the
// caller) while the kernels of the chunk before run on the compute stream (enqueue_batch, ctx.hip) and results return on
// a third; small batches take the same steps on one stream.
#include "dcn_ctx.h"
#include "dcn_host_pool.h"

#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>

using dcn_host::HostPool;
using namespace dcn_impl;

namespace {

enum class Transport {
    AsciiDirect, // page-locked ASCII: DMA as it is, pack on the device
    AsciiStaged, // pageable ASCII copied into the pinned ring, pack on the device
    HostPacked,  // pageable ASCII packed by the host threads INTO the pinned ring: 0.375 B/bp on the link
    Packed,      // the caller hands over the 2-bit stream + mask
};

struct HostInput {
    const uint8_t *bases = nullptr;    // ASCII, or null
    const uint32_t *packed = nullptr;  // caller-packed stream (Transport::Packed)
    const uint32_t *invmask = nullptr;
    const uint64_t *offsets = nullptr;
    const uint32_t *unit_id = nullptr;
    uint32_t n_reads = 0;
};

int alloc_slot_impl(dcn_ctx *c, int si);

// a slot is either complete or empty: a failure half-way (slot 1 duplicates every max_bases-sized buffer, so it is the
// allocation most likely to fail) releases what it got, and the next submit starts from null pointers again
int alloc_slot(dcn_ctx *c, int si) {
    if (c->slots[si].allocated) return DCN_OK;
    const int rc = alloc_slot_impl(c, si);
    if (rc != DCN_OK) free_slot_buffers(c->slots[si]);
    return rc;
}

int alloc_slot_impl(dcn_ctx *c, int si) {
    dcn_slot &sl = c->slots[si];
    const uint64_t MR = c->max_reads;
    if (si == 0) { // the context's own buffers
        sl.d_ascii = c->d_ascii;
        sl.d_packed = c->d_packed;
        sl.d_invmask = c->d_invmask;
        sl.d_offsets = c->d_offsets;
        sl.d_unit_id = c->d_unit_id;
        sl.d_keep = c->d_keep;
        sl.d_hits = c->d_hits;
        sl.d_total = c->d_total;
        sl.owns_buffers = false;
    } else {
        sl.owns_buffers = true;
        DCN_TRY(dev_alloc(&sl.d_ascii, c->max_bases + 64, "slot ascii"));
        DCN_TRY(dev_alloc(&sl.d_packed, packed_words(c->max_bases), "slot packed"));
        DCN_TRY(dev_alloc(&sl.d_invmask, mask_words(c->max_bases), "slot invmask"));
        DCN_TRY(dev_alloc(&sl.d_offsets, MR + 1, "slot offsets"));
        DCN_TRY(dev_alloc(&sl.d_unit_id, MR, "slot unit_id"));
        DCN_TRY(dev_alloc(&sl.d_keep, MR, "slot keep"));
        DCN_TRY(dev_alloc(&sl.d_hits, MR, "slot hits"));
        DCN_TRY(dev_alloc(&sl.d_total, MR, "slot total"));
        DCN_HIP(hipMemset(sl.d_packed, 0, packed_words(c->max_bases) * sizeof(uint32_t)));
        DCN_HIP(hipMemset(sl.d_invmask, 0, mask_words(c->max_bases) * sizeof(uint32_t)));
        DCN_HIP(hipDeviceSynchronize()); // the null-stream memsets must not overtake this slot's first copies
    }
    DCN_TRY(dev_alloc(&sl.d_report, 1, "slot report"));
    DCN_TRY(dev_alloc(&sl.d_off32, MR + 1, "slot offsets (u32)"));
    sl.mask_pairs_cap = std::max<uint64_t>(4096, mask_words(c->max_bases) / 16);
    if (const char *e = getenv("DCN_SPARSE_MASK_CAP")) sl.mask_pairs_cap = std::max<uint64_t>(1, strtoull(e, nullptr, 10)); // (tests: force the whole-mask path)
    DCN_TRY(dev_alloc(&sl.d_mask_pairs, sl.mask_pairs_cap, "slot mask pairs"));
    DCN_HIP(hipHostMalloc((void **)&sl.h_report, sizeof(dcn_batch_report), hipHostMallocDefault));
    DCN_HIP(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    sl.allocated = true;
    return DCN_OK;
}

template <typename T>
int ensure_pinned(T **p, uint64_t count) {
    if (*p) return DCN_OK;
    hipError_t e = hipHostMalloc((void **)p, std::max<uint64_t>(count, 1) * sizeof(T), hipHostMallocDefault);
    if (e != hipSuccess) {
        *p = nullptr;
        return dcn_fail(DCN_ERR_NOMEM, std::string("pinned result staging: ") + hipGetErrorString(e));
    }
    return DCN_OK;
}

// End of the chunk that starts at read r0: the first unit boundary at which the chunk holds its target number of
// bases (or the end of the batch).  (Tapering the chunks towards the end of the batch, so that less kernel time is
// left uncovered behind the last copy, was measured slower: 107 vs 114 Gbp/s packed -- every extra chunk costs more
// in copy commands and launches than the shorter tail gives back.)  Found by bisection on offsets that have NOT been
// validated yet (any answer in (r0, n_reads] is safe; validate_chunk runs while the
// chunk's payload is already on its way).
uint32_t find_cut(const dcn_ctx *c, const HostInput &in, uint32_t r0, uint64_t chunk_bases) {
    const uint64_t *off = in.offsets;
    const uint64_t b0 = off[r0];
    const uint64_t target = b0 + chunk_bases;
    uint32_t lo = r0 + 1, hi = in.n_reads; // smallest r in [lo, hi] with off[r] >= target, else n_reads
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (off[mid] >= target) hi = mid;
        else lo = mid + 1;
    }
    uint32_t r = lo;
    if (in.unit_id)
        while (r < in.n_reads && in.unit_id[r] == in.unit_id[r - 1]) ++r; // mates stay together
    return r;
}

// offsets / unit ids of reads [r0, r1): the checks of the ABI's contract, and the chunk's longest read
__global__ __launch_bounds__(256) void widen_offsets_kernel(const uint32_t *__restrict__ in32, uint64_t *__restrict__ out64, uint32_t n) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out64[i] = in32[i];
}

__global__ __launch_bounds__(256) void scatter_mask_kernel(const uint2 *__restrict__ pairs, uint32_t n, uint32_t *__restrict__ invmask) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) invmask[pairs[i].x] = pairs[i].y;
}

// The non-zero words of mask[0, m) (group g_base + i of the stream) appended to the slot's page-locked pair buffer, found by
// the pool.  false: sparse form off, or no room left -- the caller sends the words whole.
bool sparse_mask_pairs(dcn_slot &sl, const uint32_t *mask, uint64_t g_base, uint64_t m, dcn_mask_range *out) {
    if (sl.lean) return false; // (a small batch: the mask words themselves are one short copy, the pairs a memset and a kernel more)
    if (getenv("DCN_NO_SPARSE_MASK") || g_base + m > 0xFFFFFFFFull) return false; // (read per chunk: tests switch it)
    if (ensure_pinned(&sl.h_mask_pairs, sl.mask_pairs_cap) != DCN_OK) return false;
    std::vector<std::vector<uint2>> found((size_t)std::max(1, HostPool::get().width()));
    HostPool::get().run([&](int i, int nt) {
        const uint64_t per = (m + nt - 1) / nt, lo = std::min<uint64_t>(m, per * i), hi = std::min<uint64_t>(m, lo + per);
        std::vector<uint2> &v = found[(size_t)i];
        uint64_t j = lo;
        for (; j + 8 <= hi; j += 8) { // (the OR of eight words first: zero nearly always)
            const uint32_t *q = mask + j;
            if ((q[0] | q[1] | q[2] | q[3] | q[4] | q[5] | q[6] | q[7]) == 0) continue;
            for (int t = 0; t < 8; ++t)
                if (q[t]) v.push_back(make_uint2((uint32_t)(g_base + j + t), q[t]));
        }
        for (; j < hi; ++j)
            if (mask[j]) v.push_back(make_uint2((uint32_t)(g_base + j), mask[j]));
    }, m < (1u << 16));
    uint64_t total = 0;
    for (const auto &v : found) total += v.size();
    if (sl.mask_pairs_used + total > sl.mask_pairs_cap) return false;
    out->g0 = g_base;
    out->g1 = g_base + m;
    out->pairs_off = sl.mask_pairs_used;
    out->n = (uint32_t)total;
    for (const auto &v : found) {
        if (!v.empty()) memcpy(sl.h_mask_pairs + sl.mask_pairs_used, v.data(), v.size() * sizeof(uint2));
        sl.mask_pairs_used += v.size();
    }
    return true;
}

// off32_out (may be null): the chunk's offsets [r0, r1] narrowed to u32, written to off32_out[r0 .. r1]
int validate_chunk(const HostInput &in, uint32_t r0, uint32_t r1, uint64_t n_bases_total, uint64_t *max_len_out,
                   uint32_t *off32_out = nullptr) {
    // One pass over the chunk's offsets (and unit ids) on the host threads: at 10 M reads per batch the plain loop cost the
    // submitting thread 4-5 ms of a 12 ms call, next to the pack it also waits for when the bases are pageable.
    const uint64_t *off = in.offsets;
    const uint32_t *uid = in.unit_id;
    const uint32_t n = r1 - r0, n_reads = in.n_reads;
    std::atomic<uint32_t> bad{0};
    std::atomic<uint64_t> max_len{0};
    static const bool serial = getenv("DCN_SERIAL_VALIDATE") != nullptr; // (A/B: the submitting thread alone)
    HostPool::get().run([&](int i, int nt) {
        const uint32_t per = (n + (uint32_t)nt - 1) / (uint32_t)nt;
        const uint32_t a = r0 + std::min<uint64_t>(n, (uint64_t)per * (uint32_t)i), b = r0 + std::min<uint64_t>(n, (uint64_t)per * ((uint32_t)i + 1));
        uint64_t m = 0;
        uint32_t e = 0;
        for (uint32_t r = a; r < b; ++r) { // (no early exit: the loop vectorises)
            const uint64_t lo = off[r], hi = off[r + 1];
            e |= (uint32_t)(hi < lo) | (uint32_t)(hi > n_bases_total);
            m = std::max(m, hi - lo);
        }
        if (off32_out) {
            for (uint32_t r = a; r < b; ++r) off32_out[r] = (uint32_t)off[r];
            if (b == r1) off32_out[r1] = (uint32_t)off[r1]; // (every slice that ends at r1 writes the same value)
        }
        if (uid)
            for (uint32_t r = a + 1; r <= b && r < n_reads; ++r) e |= (uid[r] != uid[r - 1] && uid[r] != uid[r - 1] + 1) ? 2u : 0u;
        if (e) bad.fetch_or(e);
        uint64_t cur = max_len.load();
        while (m > cur && !max_len.compare_exchange_weak(cur, m)) {
        }
    }, n < (1u << 16) || serial);
    const uint32_t e = bad.load();
    if (e & 1u) return dcn_fail(DCN_ERR_ARG, "offsets must be non-decreasing");
    if (max_len.load() > 0xFFFFFFF0ull) return dcn_fail(DCN_ERR_ARG, "read longer than 2^32 bases");
    if (e & 2u) return dcn_fail(DCN_ERR_ARG, "unit_id must stay equal or grow by one");
    *max_len_out = max_len.load();
    return DCN_OK;
}

int chunk_events(dcn_slot &sl, size_t n) {
    while (sl.ev_h2d.size() < n) {
        hipEvent_t a = nullptr, b = nullptr;
        DCN_HIP(hipEventCreateWithFlags(&a, hipEventDisableTiming));
        sl.ev_h2d.push_back(a);
        DCN_HIP(hipEventCreateWithFlags(&b, hipEventDisableTiming));
        sl.ev_comp.push_back(b);
    }
    return DCN_OK;
}

// kernels + result copies of one chunk (its inputs are on the device, or on their way on the copy stream)
// n_known: the batch's chunks are all in sl.chunks (false while a host-bound submission is still cutting them: the
// decisions then go back in one copy behind the last chunk)
int enqueue_chunk(dcn_ctx *c, dcn_slot &sl, size_t ci, bool wait_h2d, bool n_known = true, bool is_last = false) {
    const dcn_chunk &ch = sl.chunks[ci];
    if (wait_h2d && !c->lean) DCN_HIP(hipStreamWaitEvent(c->stream, sl.ev_h2d[ci], 0)); // (lean: the copies are on this stream)
    if (sl.off32) {
        const uint32_t n = ch.r1 - ch.r0 + 1;
        hipLaunchKernelGGL(widen_offsets_kernel, dim3(std::min<uint32_t>((n + 255) / 256, 1024)), dim3(256), 0, c->stream,
                           sl.d_off32 + ch.r0, sl.d_offsets + ch.r0, n);
        DCN_HIP(hipGetLastError());
    }
    for (const dcn_mask_range &mr : ch.mask_ranges) { // mask words that crossed the link as their non-zero ones only
        DCN_HIP(hipMemsetAsync(sl.d_invmask + DCN_FRONT_PAD + mr.g0, 0, (mr.g1 - mr.g0) * sizeof(uint32_t), c->stream));
        if (mr.n) {
            hipLaunchKernelGGL(scatter_mask_kernel, dim3(std::min<uint32_t>((mr.n + 255) / 256, 1024)), dim3(256), 0, c->stream,
                               sl.d_mask_pairs + mr.pairs_off, mr.n, sl.d_invmask + DCN_FRONT_PAD);
            DCN_HIP(hipGetLastError());
        }
    }
    BatchView v;
    v.d_ascii = sl.device_pack ? sl.d_ascii : nullptr;
    v.d_packed = sl.d_packed;
    v.d_invmask = sl.d_invmask;
    v.d_offsets = sl.d_offsets + ch.r0;
    v.d_unit_id = sl.has_units ? sl.d_unit_id + ch.r0 : nullptr;
    v.unit_base = ch.u0;
    v.n_reads = ch.r1 - ch.r0;
    v.n_units = ch.u1 - ch.u0;
    // ASCII chunks are copied and packed in whole 32-base groups (see submit_impl)
    v.b0 = ch.b0 / 32 * 32;
    v.b1 = std::min<uint64_t>((ch.b1 + 31) / 32 * 32, sl.n_bases);
    v.stream_bases = sl.n_bases;
    v.d_keep = sl.d_keep + ch.u0;
    v.d_hits = sl.counts ? sl.d_hits + ch.u0 : nullptr;
    v.d_total = sl.counts ? sl.d_total + ch.u0 : nullptr;
    v.d_report = sl.d_report;
    DCN_TRY(enqueue_batch(c, v, &sl.params));
    // Results travel back per chunk when hit counts were asked for (8 bytes per unit: worth overlapping).  When only the
    // decisions are (1 byte per unit) a copy per chunk is three runtime calls per chunk for nothing: they go back in one
    // copy behind the last chunk -- or, for a batch of many chunks, in two: everything up to the last chunk but one while
    // the last chunk is still on the link, and the last chunk's own (a 10 M-read call otherwise ends with 10 MB crossing
    // the link back after everything else is done: 0.2 ms of its 12.4 ms).
    const size_t n_ch = sl.chunks.size();
    const bool last = n_known ? ci + 1 == n_ch : is_last;
    const bool split = n_known && !sl.counts && n_ch >= 4, early = split && ci + 2 == n_ch;
    if (!sl.counts && !last && !early) return DCN_OK;
    if (!c->lean) { // (lean: d2h_stream IS the compute stream for this submission)
        DCN_HIP(hipEventRecord(sl.ev_comp[ci], c->stream));
        DCN_HIP(hipStreamWaitEvent(c->d2h_stream, sl.ev_comp[ci], 0));
    }
    const uint32_t k0 = sl.counts ? ch.u0 : (split && last ? sl.chunks[n_ch - 2].u1 : 0u);
    const uint32_t nu = ch.u1 - k0;
    DCN_HIP(hipMemcpyAsync((sl.keep_direct ? sl.u_keep : sl.h_keep) + k0, sl.d_keep + k0, nu, hipMemcpyDeviceToHost,
                           c->d2h_stream));
    if (sl.u_hits)
        DCN_HIP(hipMemcpyAsync((sl.hits_direct ? sl.u_hits : sl.h_hits) + ch.u0, sl.d_hits + ch.u0,
                               (uint64_t)nu * sizeof(uint32_t), hipMemcpyDeviceToHost, c->d2h_stream));
    if (sl.u_total)
        DCN_HIP(hipMemcpyAsync((sl.total_direct ? sl.u_total : sl.h_total) + ch.u0, sl.d_total + ch.u0,
                               (uint64_t)nu * sizeof(uint32_t), hipMemcpyDeviceToHost, c->d2h_stream));
    return DCN_OK;
}

int finish_submission(dcn_ctx *c, dcn_slot &sl) {
    // the report is written on the compute stream (cleared at submission, filled by the finish kernels): the copy must
    // come behind all of it, also for a batch without any chunk
    if (!c->lean) {
        const int e = c->ev_next;
        c->ev_next = (e + 1) % dcn_ctx::N_EV;
        DCN_HIP(hipEventRecord(c->ev_comp[e], c->stream));
        DCN_HIP(hipStreamWaitEvent(c->d2h_stream, c->ev_comp[e], 0));
    }
    DCN_HIP(hipMemcpyAsync(sl.h_report, sl.d_report, sizeof(dcn_batch_report), hipMemcpyDeviceToHost, c->d2h_stream));
    DCN_HIP(hipEventRecord(sl.done, c->d2h_stream));
    return DCN_OK;
}

// after a failure in the middle of a submission: nothing of this context may still be running when the caller's
// buffers go away
void drain(dcn_ctx *c) {
    (void)hipStreamSynchronize(c->copy_stream);
    (void)hipStreamSynchronize(c->stream);
    (void)hipStreamSynchronize(c->d2h_stream);
}

int submit_impl(dcn_ctx *c, const HostInput &in, const dcn_params *params, uint8_t *keep, uint32_t *hits,
                uint32_t *total, uint64_t *ticket) {
    if (!c) return dcn_fail(DCN_ERR_ARG, "ctx is NULL");
    if (!ticket) return dcn_fail(DCN_ERR_ARG, "ticket is NULL");
    *ticket = 0;
    DCN_TRY(check_params(params));
    if (in.n_reads > 0 && (!in.offsets || !keep)) return dcn_fail(DCN_ERR_ARG, "offsets/keep is NULL");
    if (in.n_reads > c->max_reads) return dcn_fail(DCN_ERR_CAPACITY, "n_reads exceeds the context's max_batch_reads");
    if (c->batch_pending) return dcn_fail(DCN_ERR_ARG, "device-pointer batches are pending: dcn_ctx_synchronize first");
    int si = -1;
    for (int i = 0; i < dcn_ctx::N_SLOTS && si < 0; ++i)
        if (!c->slots[i].busy) si = i;
    if (si < 0) return dcn_fail(DCN_ERR_CAPACITY, "two batches are already in flight: dcn_filter_batch_wait first");
    DCN_HIP(hipSetDevice(c->device));
    DCN_TRY(alloc_slot(c, si));
    dcn_slot &sl = c->slots[si];
    const uint32_t n_reads = in.n_reads;
    uint64_t n_bases = 0;
    uint32_t n_units = 0;
    if (n_reads) {
        if (in.offsets[0] != 0) return dcn_fail(DCN_ERR_ARG, "offsets[0] must be 0");
        n_bases = in.offsets[n_reads];
        if (n_bases > c->max_bases) return dcn_fail(DCN_ERR_CAPACITY, "batch exceeds the context's max_batch_bases");
        if (in.unit_id && in.unit_id[0] != 0) return dcn_fail(DCN_ERR_ARG, "unit_id[0] must be 0");
        const bool packed_in = in.packed != nullptr;
        if (n_bases > 0 && !packed_in && !in.bases) return dcn_fail(DCN_ERR_ARG, "bases is NULL");
        if (n_bases > 0 && packed_in && !in.invmask) return dcn_fail(DCN_ERR_ARG, "invmask is NULL");
    }
    const bool host_pack_ok = !getenv("DCN_NO_HOST_PACK"); // read per call: tests switch it
    // Page-locked ASCII can cross the link as it is (1 byte per base, no host work: 52-53 Gbp/s) or be packed by the host
    // threads like pageable ASCII (0.375 bytes per base: 90-110 Gbp/s where they pack with AVX-512, csrc/host_pack.cpp).
    // The faster one is taken; DCN_PINNED_ASCII_DMA=1 keeps the host out of it.
    const bool bases_pinned = is_pinned_host(in.bases);
    const bool pinned_dma = bases_pinned && (!host_pack_ok || !dcn_host_pack_is_wide() || getenv("DCN_PINNED_ASCII_DMA"));
    Transport tr;
    if (in.packed) tr = Transport::Packed;
    else if (pinned_dma) tr = Transport::AsciiDirect;
    else tr = host_pack_ok ? Transport::HostPacked : Transport::AsciiStaged;

    // A SMALL batch is some twenty GPU commands -- copies, memsets, a handful of kernels, event records and waits between three
    // streams -- whatever it carries, and those, not its kernels, are what it costs (130 us for 1,024 reads as for 16,384), and
    // what several contexts calling at once queue up behind (eight threads: 1.2 Gbp/s at 1,024 reads per call, 17 at 16,384;
    // profiles/r04_small_calls.txt).  Up to DCN_LEAN_MAX_BASES (16 Mbp; 0: never) a batch is submitted in its plain form on ONE
    // stream: copies, kernels and result copies in order on `stream` (no events between streams; what a batch of this size
    // could overlap inside itself is tens of microseconds), 64-bit offsets as they are (no narrowing and widening kernel), the
    // mask words themselves (no pairs, memset and scatter kernel).  Same box: 1,024 reads per call 1.2 -> 1.5 Gbp/s from one
    // thread and 1.2 -> 4.0 from eight, 16,384: 15 -> 18 and 17 -> 45, 65,536: 37 -> 40 and 52 -> 79; at 262,144 (39 Mbp) the
    // three-stream form wins again (98 against 67 from two threads), hence the limit.
    const char *lean_env = getenv("DCN_LEAN_MAX_BASES"); // (read per call: tests run both forms in one process)
    const uint64_t lean_max_bases = lean_env ? strtoull(lean_env, nullptr, 10) : (16ull << 20);
    struct LeanScope {
        dcn_ctx *c;
        hipStream_t copy, d2h;
        bool on;
        ~LeanScope() {
            if (!on) return;
            c->copy_stream = copy;
            c->d2h_stream = d2h;
            c->lean = false;
        }
    } lean_scope{c, c->copy_stream, c->d2h_stream, n_reads > 0 && n_bases <= lean_max_bases && n_bases <= c->chunk_bases};
    if (lean_scope.on) {
        c->copy_stream = c->stream;
        c->d2h_stream = c->stream;
        c->lean = true;
    }
    sl.lean = lean_scope.on;
    sl.params = *params;
    sl.counts = hits || total;
    sl.has_units = in.unit_id != nullptr;
    sl.n_reads = n_reads;
    sl.n_bases = n_bases;
    sl.u_keep = keep;
    sl.u_hits = hits;
    sl.u_total = total;
    sl.keep_direct = is_pinned_host(keep);
    sl.hits_direct = hits && is_pinned_host(hits);
    sl.total_direct = total && is_pinned_host(total);
    if (!sl.keep_direct) DCN_TRY(ensure_pinned(&sl.h_keep, c->max_reads));
    if (hits && !sl.hits_direct) DCN_TRY(ensure_pinned(&sl.h_hits, c->max_reads));
    if (total && !sl.total_direct) DCN_TRY(ensure_pinned(&sl.h_total, c->max_reads));
    const int off_pinned = is_pinned_host(in.offsets) ? 1 : 0, uid_pinned = is_pinned_host(in.unit_id) ? 1 : 0;
    static const bool no_off32 = getenv("DCN_NO_OFF32") != nullptr; // (A/B)
    sl.off32 = n_reads > 0 && n_bases < (1ull << 32) && !no_off32 && !sl.lean;
    if (sl.off32) DCN_TRY(ensure_pinned(&sl.h_off32, c->max_reads + 1));
    const int pk_pinned = in.packed ? ((is_pinned_host(in.packed) && is_pinned_host(in.invmask)) ? 1 : 0) : 0;

    // With another batch already in flight the kernels of this batch's last chunk are covered by the next batch's
    // copies, so nothing argues for small chunks any more, and every chunk costs the host ~0.2 ms of runtime calls:
    // twice the chunk size then (packed input, two in flight: 105 -> 120 Gbp/s when the host was the limit).
    static const uint64_t inflight_factor = getenv("DCN_INFLIGHT_CHUNK_FACTOR") ? strtoull(getenv("DCN_INFLIGHT_CHUNK_FACTOR"), nullptr, 10) : 2;
    const uint64_t chunk_bases = c->chunk_bases * (slots_busy(c) ? std::max<uint64_t>(inflight_factor, 1) : 1);
    // DCN_SUBMIT_TIMING=1: where the submitting thread's time goes, one line per call on stderr
    static const bool submit_timing = getenv("DCN_SUBMIT_TIMING") != nullptr;
    double tm[6] = {0, 0, 0, 0, 0, 0}; // stage wait, pack, copy calls, offsets / unit ids, validate, kernels
    const auto t_submit0 = std::chrono::steady_clock::now();
    auto lap = [&](int which, std::chrono::steady_clock::time_point &t) {
        if (!submit_timing) return;
        const auto now = std::chrono::steady_clock::now();
        tm[which] += std::chrono::duration<double, std::milli>(now - t).count();
        t = now;
    };
    for (int attempt = 0;; ++attempt) {
        sl.device_pack = tr == Transport::AsciiDirect || tr == Transport::AsciiStaged;
        sl.chunks.clear();
        sl.mask_pairs_used = 0;
        DCN_HIP(hipMemsetAsync(sl.d_report, 0, sizeof(dcn_batch_report), c->stream));
        bool saw_newline = false;
        int rc = DCN_OK;
        if (n_reads && off_pinned && !sl.off32) rc = staged_h2d(c, sl.d_offsets, in.offsets, (uint64_t)(n_reads + 1) * sizeof(uint64_t), 1);
        if (rc == DCN_OK && n_reads && in.unit_id && uid_pinned)
            rc = staged_h2d(c, sl.d_unit_id, in.unit_id, (uint64_t)n_reads * sizeof(uint32_t), 1);
        uint32_t r0 = 0, u0 = 0;
        uint64_t groups_done = 0; // 32-base groups of the stream already sent (HostPacked / Packed)
        static const bool no_interleave = getenv("DCN_NO_INTERLEAVE") != nullptr, no_ride = getenv("DCN_NO_RIDE") != nullptr; // (A/B)
        const bool interleave = !no_interleave;
        while (r0 < n_reads && rc == DCN_OK) {
            dcn_chunk ch;
            ch.r0 = r0;
            ch.u0 = u0;
            ch.r1 = find_cut(c, in, r0, chunk_bases);
            ch.u1 = in.unit_id ? (ch.r1 == n_reads ? in.unit_id[n_reads - 1] + 1 : in.unit_id[ch.r1]) : ch.r1;
            ch.b0 = in.offsets[ch.r0];
            ch.b1 = in.offsets[ch.r1];
            if (ch.b1 < ch.b0 || ch.b1 > n_bases) {
                rc = dcn_fail(DCN_ERR_ARG, "offsets must be non-decreasing");
                break;
            }
            bool rode = false; // this chunk's pageable offsets / unit ids went with its packed piece
            auto copies = [&]() -> int {
                if (ch.b1 > ch.b0) {
                    if (sl.device_pack) {
                        // whole 32-base groups, so that the device pack of the groups two chunks share is right
                        // whichever of them runs last
                        const uint64_t a0 = ch.b0 / 32 * 32, a1 = std::min<uint64_t>((ch.b1 + 31) / 32 * 32, n_bases);
                        DCN_TRY(staged_h2d(c, sl.d_ascii + a0, in.bases + a0, a1 - a0, tr == Transport::AsciiDirect ? 1 : 0));
                    } else {
                        // groups not sent yet, up to the one holding this chunk's last base
                        const uint64_t g0 = groups_done, g1 = (ch.b1 + 31) / 32;
                        if (g1 > g0) {
                            uint32_t *dp = sl.d_packed + DCN_FRONT_PAD + 2 * g0, *dm = sl.d_invmask + DCN_FRONT_PAD + g0;
                            if (tr == Transport::Packed) {
                                DCN_TRY(staged_h2d(c, dp, in.packed + 2 * g0, (g1 - g0) * 8, pk_pinned));
                                dcn_mask_range mr;
                                if (sparse_mask_pairs(sl, in.invmask + g0, g0, g1 - g0, &mr)) {
                                    if (mr.n)
                                        DCN_HIP(hipMemcpyAsync(sl.d_mask_pairs + mr.pairs_off, sl.h_mask_pairs + mr.pairs_off, (uint64_t)mr.n * sizeof(uint2),
                                                               hipMemcpyHostToDevice, c->copy_stream));
                                    ch.mask_ranges.push_back(mr);
                                } else {
                                    DCN_TRY(staged_h2d(c, dm, in.invmask + g0, (g1 - g0) * 4, pk_pinned));
                                }
                            } else {
                                // pieces of whole groups: 8 bytes of stream + 4 of mask per group, side by side in a
                                // staging buffer, packed there by the host threads
                                const uint64_t per_piece = c->stage_bytes / 12 / 64 * 64;
                                // pageable offsets (and unit ids) of the chunk ride in the same staging buffer when they fit
                                // behind its one piece, copied by the threads that pack it: no ring slot, no job and no
                                // copy by the submitting thread of their own (3.5 MB per 64 Mbp chunk of 150 bp reads:
                                // 3.7 ms of a 10 M-read call)
                                const uint64_t n_off = sl.off32 ? 0 : (uint64_t)(ch.r1 - ch.r0 + 1) * sizeof(uint64_t); // (u32 offsets go by themselves, below)
                                const uint64_t n_uid = (in.unit_id && !uid_pinned) ? (uint64_t)(ch.r1 - ch.r0) * sizeof(uint32_t) : 0;
                                const bool ride = (!off_pinned || sl.off32) && (n_off || n_uid) && !no_ride && g1 - g0 <= per_piece &&
                                                  12 * (g1 - g0) + 16 + n_off + n_uid <= c->stage_bytes;
                                for (uint64_t g = g0; g < g1; g += per_piece) {
                                    const uint64_t m = std::min<uint64_t>(per_piece, g1 - g);
                                    const int which = c->stage_next;
                                    c->stage_next = (which + 1) % dcn_ctx::N_STAGE;
                                    auto tl = std::chrono::steady_clock::now();
                                    DCN_HIP(hipEventSynchronize(c->stage_free[which]));
                                    lap(0, tl);
                                    uint32_t *hp = (uint32_t *)c->h_stage[which], *hm = hp + 2 * m;
                                    uint8_t *ho = (uint8_t *)(((uintptr_t)(hm + m) + 7) & ~(uintptr_t)7), *hu = ho + n_off;
                                    std::atomic<bool> nl(false);
                                    HostPool::get().run([&](int i, int nt) {
                                        if (ride) {
                                            const uint64_t o0 = n_off * i / nt, o1 = n_off * (i + 1) / nt, q0 = n_uid * i / nt, q1 = n_uid * (i + 1) / nt;
                                            if (n_off) memcpy(ho + o0, (const uint8_t *)(in.offsets + ch.r0) + o0, o1 - o0);
                                            if (n_uid) memcpy(hu + q0, (const uint8_t *)(in.unit_id + ch.r0) + q0, q1 - q0);
                                        }
                                        const uint64_t per = (m + nt - 1) / nt, lo = std::min<uint64_t>(m, per * i),
                                                       hi = std::min<uint64_t>(m, lo + per);
                                        if (hi <= lo) return;
                                        // a '\n' anywhere means some read may end in one (src/filter_common.rs:229 strips
                                        // it): only the device path probes read ends, so the batch is sent again as ASCII
                                        if (dcn_host_pack_groups(in.bases, n_bases, g + lo, g + hi, hp + 2 * lo, hm + lo))
                                            nl.store(true);
                                    }, m < 4096);
                                    lap(1, tl);
                                    saw_newline = saw_newline || nl.load();
                                    DCN_HIP(hipMemcpyAsync(dp + 2 * (g - g0), hp, m * 8, hipMemcpyHostToDevice, c->copy_stream));
                                    dcn_mask_range mr;
                                    if (sparse_mask_pairs(sl, hm, g, m, &mr)) {
                                        if (mr.n)
                                            DCN_HIP(hipMemcpyAsync(sl.d_mask_pairs + mr.pairs_off, sl.h_mask_pairs + mr.pairs_off, (uint64_t)mr.n * sizeof(uint2),
                                                                   hipMemcpyHostToDevice, c->copy_stream));
                                        ch.mask_ranges.push_back(mr);
                                    } else {
                                        DCN_HIP(hipMemcpyAsync(dm + (g - g0), hm, m * 4, hipMemcpyHostToDevice, c->copy_stream));
                                    }
                                    if (ride) {
                                        if (n_off) DCN_HIP(hipMemcpyAsync(sl.d_offsets + ch.r0, ho, n_off, hipMemcpyHostToDevice, c->copy_stream));
                                        if (n_uid) DCN_HIP(hipMemcpyAsync(sl.d_unit_id + ch.r0, hu, n_uid, hipMemcpyHostToDevice, c->copy_stream));
                                        rode = true;
                                    }
                                    DCN_HIP(hipEventRecord(c->stage_free[which], c->copy_stream));
                                    lap(2, tl);
                                }
                            }
                            groups_done = g1;
                        }
                    }
                }
                // page-locked offsets / unit ids went over in one copy each before the first chunk (two runtime calls
                // less per chunk); pageable ones are staged chunk by chunk
                auto to = std::chrono::steady_clock::now();
                if (!off_pinned && !rode && !sl.off32)
                    DCN_TRY(staged_h2d(c, sl.d_offsets + ch.r0, in.offsets + ch.r0, (uint64_t)(ch.r1 - ch.r0 + 1) * sizeof(uint64_t), 0));
                if (in.unit_id && !uid_pinned && !rode)
                    DCN_TRY(staged_h2d(c, sl.d_unit_id + ch.r0, in.unit_id + ch.r0, (uint64_t)(ch.r1 - ch.r0) * sizeof(uint32_t), 0));
                lap(3, to);
                return DCN_OK;
            };
            if ((rc = copies()) != DCN_OK) break;
            if (saw_newline) break; // this attempt is abandoned
            // validated while the copies above are in flight; the kernels are only queued in the second pass
            auto tv = std::chrono::steady_clock::now();
            rc = validate_chunk(in, ch.r0, ch.r1, n_bases, &ch.max_len, sl.off32 ? sl.h_off32 : nullptr);
            lap(4, tv);
            if (rc != DCN_OK) break;
            if (sl.off32) { // narrowed by the check's own pass over them, into the slot's page-locked copy
                hipError_t he2 = hipMemcpyAsync(sl.d_off32 + ch.r0, sl.h_off32 + ch.r0, (uint64_t)(ch.r1 - ch.r0 + 1) * sizeof(uint32_t),
                                                hipMemcpyHostToDevice, c->copy_stream);
                if (he2 != hipSuccess) {
                    rc = dcn_fail(DCN_ERR_HIP, std::string("hipMemcpyAsync (offsets): ") + hipGetErrorString(he2));
                    break;
                }
            }
            if (ch.u1 < ch.u0 || (uint64_t)ch.u1 - ch.u0 > (uint64_t)ch.r1 - ch.r0) {
                rc = dcn_fail(DCN_ERR_ARG, "unit_id must stay equal or grow by one");
                break;
            }
            sl.chunks.push_back(ch);
            if ((rc = chunk_events(sl, sl.chunks.size())) != DCN_OK) break;
            hipError_t he = c->lean ? hipSuccess : hipEventRecord(sl.ev_h2d[sl.chunks.size() - 1], c->copy_stream);
            if (he != hipSuccess) {
                rc = dcn_fail(DCN_ERR_HIP, std::string("hipEventRecord: ") + hipGetErrorString(he));
                break;
            }
            r0 = ch.r1;
            u0 = ch.u1;
            if (interleave && sl.chunks.size() >= 2) { // the chunk before this one: its copies are queued, it is not the last
                auto tk = std::chrono::steady_clock::now();
                rc = enqueue_chunk(c, sl, sl.chunks.size() - 2, true, false, false);
                lap(5, tk);
            }
        }
        // The kernels of a chunk are queued as soon as the next chunk's copies are, one chunk behind: they then run under
        // the host's work on the chunks that follow (packing pageable bases: a blocking 10 M-read call 19.3 -> 15 ms; scanning a
        // caller's mask for its non-zero words: 10.5 -> 8.8 ms), not after it.  (Until late in round 3 all copies were queued
        // first and all kernels after them -- right while a chunk's runtime calls cost the host as much as its copy took on
        // the link; a chunk's copy is three times that now.  DCN_NO_INTERLEAVE=1 brings the two passes back.)
        auto tk = std::chrono::steady_clock::now();
        if (interleave) {
            if (rc == DCN_OK && !saw_newline && !sl.chunks.empty()) {
                const size_t n_ch = sl.chunks.size();
                if (!sl.counts && n_ch >= 4) { // the decisions of every chunk but the last go back while the last one's kernels run
                    hipError_t he = hipEventRecord(sl.ev_comp[n_ch - 2], c->stream);
                    if (he == hipSuccess) he = hipStreamWaitEvent(c->d2h_stream, sl.ev_comp[n_ch - 2], 0);
                    if (he == hipSuccess)
                        he = hipMemcpyAsync(sl.keep_direct ? sl.u_keep : sl.h_keep, sl.d_keep, sl.chunks[n_ch - 2].u1, hipMemcpyDeviceToHost, c->d2h_stream);
                    if (he != hipSuccess) rc = dcn_fail(DCN_ERR_HIP, std::string("early result copy: ") + hipGetErrorString(he));
                }
                if (rc == DCN_OK) rc = enqueue_chunk(c, sl, n_ch - 1, true); // (all chunks known now: it copies its own decisions only)
            }
        } else {
            for (size_t ci = 0; rc == DCN_OK && !saw_newline && ci < sl.chunks.size(); ++ci) rc = enqueue_chunk(c, sl, ci, true);
        }
        lap(5, tk);

        n_units = u0;
        if (rc == DCN_OK && saw_newline && attempt == 0) {
            drain(c);
            tr = bases_pinned ? Transport::AsciiDirect : Transport::AsciiStaged;
            continue;
        }
        if (rc != DCN_OK) {
            drain(c);
            return rc;
        }
        break;
    }
    sl.n_units = n_units;
    int rc = finish_submission(c, sl);
    if (rc != DCN_OK) {
        drain(c);
        return rc;
    }
    if (submit_timing)
        fprintf(stderr, "submit timing: %.2f ms, %zu chunks: stage wait %.2f, pack %.2f, copy calls %.2f, offsets / unit ids %.2f, validate %.2f, "
                        "kernels %.2f\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_submit0).count(),
                sl.chunks.size(), tm[0], tm[1], tm[2], tm[3], tm[4], tm[5]);
    sl.busy = true;
    sl.ticket = c->next_ticket++;
    *ticket = sl.ticket;
    return DCN_OK;
}

int wait_impl(dcn_ctx *c, uint64_t ticket) {
    if (!c) return dcn_fail(DCN_ERR_ARG, "ctx is NULL");
    dcn_slot *slp = nullptr;
    for (auto &s : c->slots)
        if (s.busy && s.ticket == ticket) slp = &s;
    if (!slp) return dcn_fail(DCN_ERR_ARG, "no batch with this ticket is in flight");
    dcn_slot &sl = *slp;
    DCN_HIP(hipSetDevice(c->device));
    auto fail = [&](int rc) {
        drain(c);
        sl.busy = false;
        return rc;
    };
    for (int attempt = 0;; ++attempt) {
        hipError_t e = hipEventSynchronize(sl.done);
        if (e != hipSuccess) return fail(dcn_fail(DCN_ERR_HIP, std::string("hipEventSynchronize: ") + hipGetErrorString(e)));
        if (sl.h_report->bounds) return fail(dcn_fail(DCN_ERR_INTERNAL, "scan kernel: index out of range in phase B (DCN_DEBUG_BOUNDS build)"));
        if (sl.h_report->bad_offsets) return fail(dcn_fail(DCN_ERR_INTERNAL, "the device met offsets the host had validated as decreasing or beyond the batch"));
        if (!sl.h_report->overflow) break;
        // Some chunk dropped hit records.  Grow the scratch and run the batch's kernels again: its inputs are still
        // resident in the slot.  Everything else in flight is drained first, since the scratch is shared.
        const uint64_t need = sl.h_report->need;
        if (attempt >= 4) return fail(overflow_error(c, need));
        drain(c);
        int rc = DCN_OK;
        if (sl.h_report->overflow & 2u) rc = grow_run_slots(c); // one slot per window from now on
        if (rc == DCN_OK && (sl.h_report->overflow & 1u)) {
            uint64_t want = std::max<uint64_t>(need + need / 8 + 1024, c->rec_capacity * 2);
            rc = alloc_records(c, std::min<uint64_t>(want, 1ull << 29));
        }
        if (rc != DCN_OK) return fail(rc);
        if (hipMemsetAsync(sl.d_report, 0, sizeof(dcn_batch_report), c->stream) != hipSuccess)
            return fail(dcn_fail(DCN_ERR_HIP, "hipMemsetAsync failed"));
        for (size_t ci = 0; ci < sl.chunks.size(); ++ci)
            if ((rc = enqueue_chunk(c, sl, ci, false)) != DCN_OK) return fail(rc);
        if ((rc = finish_submission(c, sl)) != DCN_OK) return fail(rc);
    }
    if (!sl.keep_direct && sl.n_units) memcpy(sl.u_keep, sl.h_keep, sl.n_units);
    if (sl.u_hits && !sl.hits_direct && sl.n_units) memcpy(sl.u_hits, sl.h_hits, (uint64_t)sl.n_units * sizeof(uint32_t));
    if (sl.u_total && !sl.total_direct && sl.n_units) memcpy(sl.u_total, sl.h_total, (uint64_t)sl.n_units * sizeof(uint32_t));
    for (int i = 0; i < DCN_N_STATS; ++i) c->host_stats[i] += sl.h_report->stats[i];
    sl.busy = false;
    return DCN_OK;
}

} // namespace

extern "C" int dcn_filter_batch_submit(dcn_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, const uint32_t *unit_id,
                                       uint32_t n_reads, const dcn_params *params, uint8_t *keep, uint32_t *hits,
                                       uint32_t *total, uint64_t *ticket) {
    HostInput in;
    in.bases = bases;
    in.offsets = offsets;
    in.unit_id = unit_id;
    in.n_reads = n_reads;
    return submit_impl(ctx, in, params, keep, hits, total, ticket);
}

extern "C" int dcn_filter_batch_packed_submit(dcn_ctx *ctx, const uint32_t *packed, const uint32_t *invmask,
                                              const uint64_t *offsets, const uint32_t *unit_id, uint32_t n_reads,
                                              const dcn_params *params, uint8_t *keep, uint32_t *hits, uint32_t *total,
                                              uint64_t *ticket) {
    if (n_reads > 0 && !packed) return dcn_fail(DCN_ERR_ARG, "packed is NULL");
    HostInput in;
    in.packed = packed;
    in.invmask = invmask;
    in.offsets = offsets;
    in.unit_id = unit_id;
    in.n_reads = n_reads;
    return submit_impl(ctx, in, params, keep, hits, total, ticket);
}

extern "C" int dcn_filter_batch_wait(dcn_ctx *ctx, uint64_t ticket) { return wait_impl(ctx, ticket); }

extern "C" int dcn_filter_batch(dcn_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, const uint32_t *unit_id,
                                uint32_t n_reads, const dcn_params *params, uint8_t *keep, uint32_t *hits,
                                uint32_t *total) {
    uint64_t ticket = 0;
    DCN_TRY(dcn_filter_batch_submit(ctx, bases, offsets, unit_id, n_reads, params, keep, hits, total, &ticket));
    return wait_impl(ctx, ticket);
}

extern "C" int dcn_filter_batch_packed(dcn_ctx *ctx, const uint32_t *packed, const uint32_t *invmask,
                                       const uint64_t *offsets, const uint32_t *unit_id, uint32_t n_reads,
                                       const dcn_params *params, uint8_t *keep, uint32_t *hits, uint32_t *total) {
    uint64_t ticket = 0;
    DCN_TRY(dcn_filter_batch_packed_submit(ctx, packed, invmask, offsets, unit_id, n_reads, params, keep, hits, total,
                                           &ticket));
    return wait_impl(ctx, ticket);
}

// dcn_dump_sweep.h -- what the consumers of a batch's minimizer dump share (internal, not part of the public ABI): the
// view of the dump that the front end (dump_front_end, ctx.hip) hands to their kernels, the flat sweep over its entries
// (locate.hip, track.hip, depth.hip, place.hip), and the helpers of the position bitmap those sweeps fill and the
// per-read kernels behind them cut up.
#pragma once

#include "dcn_internal.h"

// DCN_SWEEP_TILE_LANES lanes walk one tile's dump entries (a short read's tile has ~14, a full tile of 256 windows
// ~32), so a wave sweeps four tiles with coalesced loads and 64 probes in flight.
constexpr uint32_t DCN_SWEEP_THREADS = 256;
constexpr uint32_t DCN_SWEEP_TILE_LANES = 16;

// plan + minimizer dump of a batch (scan_kernel<..., DUMP = true> with dump_abs = 1)
struct dcn_dump_view {
    const dcn_tile *tiles;
    const uint32_t *n_tiles;
    const uint64_t *hash;
    const uint8_t *valid;
    const uint32_t *pos;   // low 32 bits of the minimizer's base index in the batch stream
    const uint32_t *count; // per tile: entries at [scan_start + carry, + count)
    uint32_t max_tiles;    // launch bound of the sweep
    uint64_t n_bases;
};

// body(s) once per valid entry s of this lane's tile.  Grid: dcn_launch_dump_sweep's.
template <typename F>
__device__ __forceinline__ void dcn_for_dump_entries(const dcn_dump_view &d, F body) {
    const uint64_t gid = (uint64_t)blockIdx.x * DCN_SWEEP_THREADS + threadIdx.x;
    const uint64_t tile = gid / DCN_SWEEP_TILE_LANES;
    const uint32_t sub = (uint32_t)(gid % DCN_SWEEP_TILE_LANES);
    if (tile >= *d.n_tiles) return;
    const dcn_tile t = d.tiles[tile];
    const uint64_t base = t.scan_start + t.carry();
    if (base >= d.n_bases) return;
    // (an entry's slot is at or before its window's first base: never past the stream)
    const uint32_t cnt = (uint32_t)min((uint64_t)d.count[tile], d.n_bases - base);
    for (uint32_t e = sub; e < cnt; e += DCN_SWEEP_TILE_LANES) {
        const uint64_t s = base + e;
        if (d.valid[s]) body(s);
    }
}

// the position of entry s.  The minimizer of a window lies at or after the window's start, which is at or after its
// slot: the low 32 bits of the position and the slot give the position
__device__ __forceinline__ uint64_t dcn_dump_position(const dcn_dump_view &d, uint64_t s) {
    return s + (uint32_t)(d.pos[s] - (uint32_t)s);
}

// set bit p of a bitmap that other lanes set bits of too: test, then atomicOr
__device__ __forceinline__ void dcn_bit_mark(uint32_t *bits, uint64_t p) {
    uint32_t *word = bits + (p >> 5);
    const uint32_t bit = 1u << (p & 31);
    if (!(*word & bit)) atomicOr(word, bit);
}

// ... and whether this lane was the one that set it: the lane that finds the bit clear owns the position
__device__ __forceinline__ bool dcn_bit_claim(uint32_t *bits, uint64_t p) {
    uint32_t *word = bits + (p >> 5);
    const uint32_t bit = 1u << (p & 31);
    if (*word & bit) return false;         // (bits are only ever set during a sweep: a set bit seen is set)
    return !(atomicOr(word, bit) & bit);   // set already: another entry of this position was first
}

// word wi of a bitmap, cut to the bits of [b0, b1)
__device__ __forceinline__ uint32_t dcn_bits_cut(const uint32_t *bits, uint64_t wi, uint64_t b0, uint64_t b1) {
    uint32_t word = bits[wi];
    if (wi == (b0 >> 5)) word &= ~0u << (b0 & 31);
    if (wi == (b1 >> 5)) word &= ~(~0u << (b1 & 31)); // (b1 a multiple of 32: its word is past the range and not loaded)
    return word;
}

// the read that owns item i of a prefix array off[0 .. n]: the last r with off[r] <= i (i < off[n])
__device__ __forceinline__ uint32_t dcn_owner_of(const uint64_t *off, uint32_t n, uint64_t i) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// per-read counts -> CSR offsets (offsets_scan.hip): offsets[0 .. n] = the exclusive scan of counts[0 .. n), offsets[n] the
// total; 64-bit offsets from 32-bit counts.  A workgroup scans DCN_SCAN_BLOCK counts (DCN_SCAN_ITEMS per thread), one
// workgroup the block sums: `block_sums` is scratch of n / DCN_SCAN_BLOCK + 1 words.
constexpr uint32_t DCN_SCAN_THREADS = 256;
constexpr uint32_t DCN_SCAN_ITEMS = 8;
constexpr uint32_t DCN_SCAN_BLOCK = DCN_SCAN_THREADS * DCN_SCAN_ITEMS;
int dcn_launch_offsets_scan(const uint32_t *counts, uint32_t n, unsigned long long *block_sums, uint64_t *offsets,
                            hipStream_t stream);

// launches a kernel that sweeps a.dump with dcn_for_dump_entries; `too_many` is the message of a grid past 2^31 blocks
template <typename Args>
int dcn_launch_dump_sweep(void (*kernel)(Args), const Args &a, const char *too_many, hipStream_t stream) {
    if (a.dump.max_tiles == 0) return DCN_OK;
    const uint64_t threads = (uint64_t)a.dump.max_tiles * DCN_SWEEP_TILE_LANES;
    const uint64_t blocks = (threads + DCN_SWEEP_THREADS - 1) / DCN_SWEEP_THREADS;
    if (blocks > 0x7FFFFFFFull) return dcn_fail(DCN_ERR_INTERNAL, too_many);
    hipLaunchKernelGGL(kernel, dim3((uint32_t)blocks), dim3(DCN_SWEEP_THREADS), 0, stream, a);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

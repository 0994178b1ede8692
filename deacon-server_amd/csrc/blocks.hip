// blocks.hip -- the reference blocks of a range (THE DEFINITION OF A REFERENCE BLOCK, include/deacon_hip_blocks.h; the
// rule, shared with the host, is dcn_blocks_classify of dcn_blocks.h).  No pass over reads: a segmented reduction over the
// positions of the range.
//   blocks_classify_kernel  genotype_kernel's load shape with the N and DEL planes beside it: 40 B read per position and the
//                           packed reference base; one class byte and one GQ byte written.  A lane takes four consecutive
//                           store bases, the first divisible by 4 (the alignment is on the store's base index, not on the
//                           range's start); the bytes of a lane's word that lie outside the range are DCN_BLK_VARIANT, so
//                           that the passes behind need not know the range's ends.
//   blocks_breaks_kernel    a thread per break stores DCN_BLK_VARIANT into its class byte: order and duplicates cannot matter.
//   blocks_heads_kernel     a position is a head when its class is not VARIANT and differs from its predecessor's, which a
//                           lane's first position reads from the class buffer (nothing in front of slot 0).
//                           <false> counts the heads of a workgroup; <true>, behind the scan of those numbers, knows every
//                           position's block (the heads at or before it, minus one) and reduces: inside the lane over its
//                           four positions, then inside the wave by block index, and the last lane of each wave segment
//                           combines into the block's record with returnless atomic min / max / add.  The head alone writes
//                           pos and cls.  A block of any length costs one set of atomics per wave it crosses; no thread
//                           walks a block.  Min, max and add commute: the result does not depend on the order (rule B8).
//   blocks_fill_kernel      the records before the reduction: minima all ones, everything else 0.
// Under -DDCN_PILEUP_POSITION_MAJOR a lane takes one position through dcn_pile_index / dcn_pile_sum_index, as genotype.hip does.
// Integers only; a lane indexes nothing by a runtime value.  The grids are sized by the range and are not capped.
#include "dcn_blocks.h"
#include "dcn_pileup.h"
#include "dcn_verify.h"

static_assert(sizeof(dcn_blk_block) == 40, "a reference block is ABI");

namespace {

constexpr uint32_t BLK_THREADS = 256;
#if defined(DCN_PILEUP_POSITION_MAJOR)
constexpr bool WIDE = false;
#else
constexpr bool WIDE = true;
#endif
constexpr uint32_t PER = WIDE ? 4u : 1u; // store bases of a lane
constexpr uint32_t NO_KEY = 0xFFFFFFFFu;

__device__ inline uint64_t first_of(const dcn_blocks_args &a) { return WIDE ? a.base0 & ~3ull : a.base0; } // the store base of slot 0

__global__ __launch_bounds__(BLK_THREADS) void blocks_classify_kernel(dcn_blocks_args a) {
    const uint64_t slot = (uint64_t)blockIdx.x * BLK_THREADS + threadIdx.x;
    const uint64_t b0 = first_of(a) + slot * PER, end = a.base0 + a.n;
    if (b0 >= end) return;
    const dcn_geno_params prm = {a.ploidy, a.min_depth, a.min_gq, a.min_qual, a.err_centi, a.het_centi};
    const dcn_blk_edges edges = {a.edges_lo, a.edges_hi};

    uint32_t n[PER][4], Q[PER][4], nn[PER], nd[PER], ref_code, ref_inv;
    if constexpr (WIDE) {
        // (in bounds as genotype_kernel's loads are: b0 + 3 < the store's used bases rounded up to 4 <= a.bases)
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c) {
            const uint4 vn = *reinterpret_cast<const uint4 *>(a.counters + (uint64_t)c * a.bases + b0);
            const uint4 vq = *reinterpret_cast<const uint4 *>(a.sums + (uint64_t)c * a.bases + b0);
            n[0][c] = vn.x, n[1][c] = vn.y, n[2][c] = vn.z, n[3][c] = vn.w;
            Q[0][c] = vq.x, Q[1][c] = vq.y, Q[2][c] = vq.z, Q[3][c] = vq.w;
        }
        const uint4 vN = *reinterpret_cast<const uint4 *>(a.counters + (uint64_t)DCN_PILE_N * a.bases + b0);
        const uint4 vD = *reinterpret_cast<const uint4 *>(a.counters + (uint64_t)DCN_PILE_DEL * a.bases + b0);
        nn[0] = vN.x, nn[1] = vN.y, nn[2] = vN.z, nn[3] = vN.w;
        nd[0] = vD.x, nd[1] = vD.y, nd[2] = vD.z, nd[3] = vD.w;
        ref_code = (a.t_packed[b0 >> 4] >> (2 * (b0 & 15))) & 0xFFu; // four bases never straddle a word: b0 % 4 == 0
        ref_inv = (a.t_invmask[b0 >> 5] >> (b0 & 31)) & 0xFu;
    } else {
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c) {
            n[0][c] = a.counters[dcn_pile_index(c, b0, a.bases)];
            Q[0][c] = a.sums[dcn_pile_sum_index(c, b0, a.bases)];
        }
        nn[0] = a.counters[dcn_pile_index(DCN_PILE_N, b0, a.bases)];
        nd[0] = a.counters[dcn_pile_index(DCN_PILE_DEL, b0, a.bases)];
        ref_code = (a.t_packed[b0 >> 4] >> (2 * (b0 & 15))) & 3u;
        ref_inv = (a.t_invmask[b0 >> 5] >> (b0 & 31)) & 1u;
    }

    // One position after the other in a loop that is not unrolled, the components rotated, as genotype_kernel does and for
    // its reason: unrolled, four cost computations are interleaved over too many registers for a streaming kernel.
    uint32_t cls_word = 0, gq_word = 0;
#pragma unroll 1
    for (uint32_t k = 0; k < PER; ++k) {
        const uint64_t b = b0 + k;
        const bool inside = b >= a.base0 && b < end;
        const uint32_t ref_column = dcn_pile_column((ref_code >> (2 * k)) & 3u, (ref_inv >> k) & 1u);
        const dcn_blk_position p = dcn_blocks_classify(n[0], Q[0], nn[0], nd[0], ref_column, prm, edges);
        cls_word |= (inside ? p.cls : DCN_BLK_VARIANT) << (8 * k);
        gq_word |= (inside ? p.gq : 0u) << (8 * k);
        if constexpr (WIDE) {
#pragma unroll
            for (uint32_t c = 0; c < 4; ++c) {
                const uint32_t tn = n[0][c], tq = Q[0][c];
                n[0][c] = n[1][c], n[1][c] = n[2][c], n[2][c] = n[3][c], n[3][c] = tn;
                Q[0][c] = Q[1][c], Q[1][c] = Q[2][c], Q[2][c] = Q[3][c], Q[3][c] = tq;
            }
            const uint32_t tN = nn[0], tD = nd[0];
            nn[0] = nn[1], nn[1] = nn[2], nn[2] = nn[3], nn[3] = tN;
            nd[0] = nd[1], nd[1] = nd[2], nd[2] = nd[3], nd[3] = tD;
        }
    }
    if constexpr (WIDE) { // byte (b - first) of the padded buffers: a word per lane
        reinterpret_cast<uint32_t *>(a.cls)[slot] = cls_word;
        reinterpret_cast<uint32_t *>(a.gq)[slot] = gq_word;
    } else {
        a.cls[slot] = (uint8_t)cls_word;
        a.gq[slot] = (uint8_t)gq_word;
    }
}

__global__ __launch_bounds__(BLK_THREADS) void blocks_breaks_kernel(dcn_blocks_args a) {
    const uint64_t i = (uint64_t)blockIdx.x * BLK_THREADS + threadIdx.x;
    if (i >= a.n_breaks) return;
    const uint64_t q = a.breaks[i];
    if (q < a.n) a.cls[(a.base0 - first_of(a)) + q] = (uint8_t)DCN_BLK_VARIANT; // (the API has checked q; the guard costs nothing)
}

__global__ __launch_bounds__(BLK_THREADS) void blocks_fill_kernel(dcn_blocks_args a) {
    const uint64_t i = (uint64_t)blockIdx.x * BLK_THREADS + threadIdx.x;
    if (i >= a.n_blocks) return;
    dcn_blk_block b;
    b.pos = 0, b.sum_depth = 0, b.len = 0, b.min_depth = 0xFFFFFFFFu, b.max_depth = 0, b.min_gq = 0xFFFFFFFFu, b.cls = 0, b.reserved = 0;
    static_cast<dcn_blk_block *>(a.blocks)[i] = b;
}

// what a lane, and then a wave segment, knows of one block
struct partial {
    unsigned long long sum;
    uint32_t len, min_depth, max_depth, min_gq;
};

__device__ inline partial nothing() { return {0ull, 0u, 0xFFFFFFFFu, 0u, 0xFFFFFFFFu}; }

__device__ inline void combine(partial &into, const partial &o) {
    into.sum += o.sum;
    into.len += o.len;
    into.min_depth = min(into.min_depth, o.min_depth);
    into.max_depth = max(into.max_depth, o.max_depth);
    into.min_gq = min(into.min_gq, o.min_gq);
}

__device__ inline partial shuffled_up(const partial &p, uint32_t d) {
    partial o;
    o.sum = __shfl_up(p.sum, d);
    o.len = __shfl_up(p.len, d);
    o.min_depth = __shfl_up(p.min_depth, d);
    o.max_depth = __shfl_up(p.max_depth, d);
    o.min_gq = __shfl_up(p.min_gq, d);
    return o;
}

// a finished partial into its block's record (results not looked at: the atomics are returnless)
__device__ inline void flush(const dcn_blocks_args &a, uint64_t index, const partial &p) {
    if (index >= a.n_blocks) return; // (cannot be: the index counts heads)
    dcn_blk_block *blk = static_cast<dcn_blk_block *>(a.blocks) + index;
    atomicAdd(&blk->len, p.len);
    atomicMin(&blk->min_depth, p.min_depth);
    atomicMax(&blk->max_depth, p.max_depth);
    atomicMin(&blk->min_gq, p.min_gq);
    atomicAdd(reinterpret_cast<unsigned long long *>(&blk->sum_depth), p.sum);
}

template <bool REDUCE>
__global__ __launch_bounds__(BLK_THREADS) void blocks_heads_kernel(dcn_blocks_args a) {
    __shared__ uint32_t s_wave[BLK_THREADS / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x / 64;
    const uint64_t slot = (uint64_t)blockIdx.x * BLK_THREADS + threadIdx.x;
    const uint64_t first = first_of(a), b0 = first + slot * PER, end = a.base0 + a.n;

    // the lane's classes, VARIANT where it has none, and the class in front of them (VARIANT: no predecessor)
    uint32_t cls_word = 0xFFFFFFFFu, prev = DCN_BLK_VARIANT;
    if (b0 < end) {
        if constexpr (WIDE) cls_word = reinterpret_cast<const uint32_t *>(a.cls)[slot];
        else cls_word = a.cls[slot] | 0xFFFFFF00u;
        if (slot > 0) prev = a.cls[slot * PER - 1];
    }
    uint32_t head_mask = 0;
    {
        uint32_t before_k = prev;
#pragma unroll
        for (uint32_t k = 0; k < PER; ++k) {
            const uint32_t c = (cls_word >> (8 * k)) & 0xFFu;
            if (c != DCN_BLK_VARIANT && c != before_k) head_mask |= 1u << k;
            before_k = c;
        }
    }

    // the heads of the lanes in front of this one in its wave, and of the waves in front of that
    const uint32_t mine = __popc(head_mask);
    uint32_t incl = mine;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    if constexpr (!REDUCE) {
        if (threadIdx.x == 0) a.block_counts[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    } else {
        // `local` counts the workgroup's heads at or before a position: block (block_offsets + local - 1); local 0 is the
        // block that the workgroup in front left open
        uint32_t local = incl - mine;
        for (uint32_t v = 0; v < wave; ++v) local += s_wave[v];
        const uint64_t group_first = a.block_offsets[blockIdx.x];

        uint32_t gq_word = 0, d0 = 0, d1 = 0, d2 = 0, d3 = 0;
        if (b0 < end) {
            if constexpr (WIDE) {
                gq_word = reinterpret_cast<const uint32_t *>(a.gq)[slot];
#pragma unroll
                for (uint32_t c = 0; c < 4; ++c) {
                    const uint4 vn = *reinterpret_cast<const uint4 *>(a.counters + (uint64_t)c * a.bases + b0);
                    d0 += vn.x, d1 += vn.y, d2 += vn.z, d3 += vn.w;
                }
            } else {
                gq_word = a.gq[slot];
#pragma unroll
                for (uint32_t c = 0; c < 4; ++c) d0 += a.counters[dcn_pile_index(c, b0, a.bases)];
            }
        }

        // Inside the lane.  `cur` is the run that is open; it is `front` when it came in from the lane before.  A run that
        // closes here goes to its block at once unless it is the front one, which first takes what the lanes before hold.
        partial cur = nothing(), front = nothing();
        bool open = false, cur_is_front = false, has_front = false;
        uint32_t cur_local = 0;
        const uint32_t local_in = local; // the block of a run that comes in from the lane before
        const auto close = [&] {
            if (!open) return;
            if (cur_is_front) front = cur, has_front = true;
            else flush(a, group_first + cur_local - 1, cur);
            open = false;
        };
        const auto step = [&](uint32_t k, uint32_t depth) {
            const uint32_t c = (cls_word >> (8 * k)) & 0xFFu;
            if (c == DCN_BLK_VARIANT) {
                close();
                return;
            }
            if (head_mask & (1u << k)) {
                close();
                cur = nothing(), open = true, cur_is_front = false, cur_local = ++local;
                const uint64_t index = group_first + cur_local - 1;
                if (index < a.n_blocks) { // (always: the index counts heads)
                    dcn_blk_block *blk = static_cast<dcn_blk_block *>(a.blocks) + index;
                    blk->pos = a.pos0 + (b0 + k - a.base0);
                    blk->cls = c;
                }
            } else if (!open) { // the lane's first position, inside the run of the lane before
                cur = nothing(), open = true, cur_is_front = true, cur_local = local;
            }
            cur.sum += depth;
            cur.len += 1;
            cur.min_depth = min(cur.min_depth, depth);
            cur.max_depth = max(cur.max_depth, depth);
            cur.min_gq = min(cur.min_gq, (gq_word >> (8 * k)) & 0xFFu);
        };
        step(0, d0);
        if constexpr (WIDE) {
            step(1, d1);
            step(2, d2);
            step(3, d3);
        }
        const uint32_t first_cls = cls_word & 0xFFu;
        const bool comes_in = first_cls != DCN_BLK_VARIANT && !(head_mask & 1u); // the run of the lane before goes on here

        // Inside the wave: an inclusive scan of the open runs, segmented by block.  The keys ascend over the lanes and a
        // lane without an open run lies between no two lanes of one key, so one compare per step is the segment test.
        const uint32_t key = open ? cur_local : NO_KEY;
        partial run = open ? cur : nothing();
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const partial o = shuffled_up(run, d);
            const uint32_t okey = __shfl_up(key, d);
            if (lane >= d && okey == key && key != NO_KEY) combine(run, o);
        }
        const partial before_me = shuffled_up(run, 1);            // the open run of the lane before, with all it gathered
        const uint32_t next_comes_in = __shfl_down(comes_in ? 1u : 0u, 1);
        if (has_front) { // the run ends in this lane: its last lane of the wave
            if (lane > 0) combine(front, before_me);
            flush(a, group_first + local_in - 1, front);
        }
        if (open && (lane == 63 || !next_comes_in)) flush(a, group_first + cur_local - 1, run);
    }
}

uint64_t slots_of(uint64_t base0, uint64_t n) { // lanes with a position of the range
    if (n == 0) return 0;
    return WIDE ? ((base0 + n + 3) >> 2) - (base0 >> 2) : n;
}

uint32_t groups_of(uint64_t items) { return (uint32_t)((items + BLK_THREADS - 1) / BLK_THREADS); }
} // namespace

uint32_t dcn_blocks_groups(uint64_t base0, uint64_t n) { return groups_of(slots_of(base0, n)); }

uint64_t dcn_blocks_pad(uint64_t base0) { return WIDE ? base0 & 3u : 0u; }

uint64_t dcn_blocks_out_bytes(uint64_t base0, uint64_t n) { return slots_of(base0, n) * PER; }

int dcn_launch_blocks_classify(const dcn_blocks_args &args, hipStream_t stream) {
    if (args.n == 0) return DCN_OK;
    hipLaunchKernelGGL(blocks_classify_kernel, dim3(dcn_blocks_groups(args.base0, args.n)), dim3(BLK_THREADS), 0, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_launch_blocks_breaks(const dcn_blocks_args &args, hipStream_t stream) {
    if (args.n_breaks == 0) return DCN_OK;
    hipLaunchKernelGGL(blocks_breaks_kernel, dim3(groups_of(args.n_breaks)), dim3(BLK_THREADS), 0, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_launch_blocks_heads(const dcn_blocks_args &args, bool reduce, hipStream_t stream) {
    if (args.n == 0) return DCN_OK;
    const dim3 grid(dcn_blocks_groups(args.base0, args.n)), block(BLK_THREADS);
    if (reduce) hipLaunchKernelGGL(blocks_heads_kernel<true>, grid, block, 0, stream, args);
    else hipLaunchKernelGGL(blocks_heads_kernel<false>, grid, block, 0, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_launch_blocks_fill(const dcn_blocks_args &args, hipStream_t stream) {
    if (args.n_blocks == 0) return DCN_OK;
    hipLaunchKernelGGL(blocks_fill_kernel, dim3(groups_of(args.n_blocks)), dim3(BLK_THREADS), 0, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

// genotype.hip -- the genotype of every position of a range (THE DEFINITION OF A GENOTYPE, include/deacon_hip.h; the
// arithmetic, shared with the host, is dcn_genotype_decide of dcn_genotype.h).
//   genotype_kernel   the shape of pileup_call_kernel.  <false> writes the gt and gq bytes and the workgroup's number of
//                     sites; <true>, behind the scan of those numbers, writes the 48-byte sites compactly in ascending
//                     position.  Both passes decide in the same code: the writing pass recomputes the costs from the
//                     counters and the sums (it does not reread gt, which the caller may not even have asked for).
//                     The kernel streams: 32 B read per position (four counter planes, four sum planes) and the packed
//                     reference base, 2 B written.  The N and DEL counters, which only a site's depth needs, are loaded
//                     for sites alone.
//                     A lane takes four consecutive store bases, the first divisible by 4: one 16-byte load per plane, one
//                     byte of packed reference, a nibble of the invalid mask, and one word each of gt and gq.  The
//                     alignment is on the store's base index, not on the range's start: a record may begin anywhere in a
//                     word of the store.  Bases in front of the range or behind it are computed on what was loaded (or on
//                     nothing) and masked.  (A form with one position and a dword per plane per lane was measured beside
//                     it and deleted: DESIGN.md section 17.  Under -DDCN_PILEUP_POSITION_MAJOR, where a position's words
//                     lie together, a lane takes one position through dcn_pile_index / dcn_pile_sum_index.)
// Integers only; a lane indexes nothing by a runtime value.  The grid is sized by the range and is not capped.
#include "dcn_genotype.h"
#include "dcn_pileup.h"
#include "dcn_verify.h"

static_assert(sizeof(dcn_genotype_site) == 48, "a genotype site is ABI");
static_assert(DCN_GENOTYPE_NONE == DCN_GENO_NONE, "the header's and dcn_genotype.h's");
static_assert(DCN_GENO_REF_INVALID == DCN_PILE_N, "dcn_pile_column's invalid base");

namespace {

constexpr uint32_t GENO_THREADS = 256;
#if defined(DCN_PILEUP_POSITION_MAJOR)
constexpr bool WIDE = false;
#else
constexpr bool WIDE = true;
#endif

__device__ inline dcn_geno_params params_of(const dcn_genotype_args &a) {
    return {a.ploidy, a.min_depth, a.min_gq, a.min_qual, a.err_centi, a.het_centi};
}

// the site of store base b (rule G7 holds there)
__device__ inline void write_site(const dcn_genotype_args &a, uint64_t at, uint64_t b, const uint32_t *n, uint32_t ref_column,
                                  const dcn_geno_result &r, const uint8_t *pl) {
    dcn_genotype_site s;
    s.pos = a.pos0 + (b - a.base0);
    s.qual = r.qual;
    s.depth = n[0] + n[1] + n[2] + n[3] + a.counters[dcn_pile_index(DCN_PILE_N, b, a.bases)] +
              a.counters[dcn_pile_index(DCN_PILE_DEL, b, a.bases)];
    s.ad[0] = n[0], s.ad[1] = n[1], s.ad[2] = n[2], s.ad[3] = n[3];
    s.gt = (uint8_t)r.gt;
    s.gq = (uint8_t)r.gq;
    s.ref_code = (uint8_t)ref_column;
    s.reserved0 = 0;
#pragma unroll
    for (uint32_t g = 0; g < DCN_GENO_GENOTYPES; ++g) s.pl[g] = pl[g];
    s.reserved1[0] = s.reserved1[1] = 0;
    static_cast<dcn_genotype_site *>(a.sites)[at] = s;
}

template <bool WRITE>
__global__ __launch_bounds__(GENO_THREADS) void genotype_kernel(dcn_genotype_args a) {
    constexpr uint32_t PER = WIDE ? 4u : 1u; // store bases of a lane
    __shared__ uint32_t s_wave[GENO_THREADS / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x / 64;
    const uint64_t slot = (uint64_t)blockIdx.x * GENO_THREADS + threadIdx.x;
    const uint64_t first = WIDE ? a.base0 & ~3ull : a.base0; // the store base of slot 0
    const uint64_t b0 = first + slot * PER, end = a.base0 + a.n;
    const dcn_geno_params prm = params_of(a);

    uint32_t n[PER][4], Q[PER][4], ref_code = 0, ref_inv = 0;
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k)
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c) n[k][c] = Q[k][c] = 0;
    if (b0 < end) {
        if constexpr (WIDE) {
            // (in bounds: b0 + 3 < the store's used bases rounded up to 4 <= a.bases, a multiple of 32, so every plane
            // begins on 16 bytes as well)
#pragma unroll
            for (uint32_t c = 0; c < 4; ++c) {
                const uint4 vn = *reinterpret_cast<const uint4 *>(a.counters + (uint64_t)c * a.bases + b0);
                const uint4 vq = *reinterpret_cast<const uint4 *>(a.sums + (uint64_t)c * a.bases + b0);
                n[0][c] = vn.x, n[1][c] = vn.y, n[2][c] = vn.z, n[3][c] = vn.w;
                Q[0][c] = vq.x, Q[1][c] = vq.y, Q[2][c] = vq.z, Q[3][c] = vq.w;
            }
            ref_code = (a.t_packed[b0 >> 4] >> (2 * (b0 & 15))) & 0xFFu; // four bases never straddle a word: b0 % 4 == 0
            ref_inv = (a.t_invmask[b0 >> 5] >> (b0 & 31)) & 0xFu;
        } else {
#pragma unroll
            for (uint32_t c = 0; c < 4; ++c) {
                n[0][c] = a.counters[dcn_pile_index(c, b0, a.bases)];
                Q[0][c] = a.sums[dcn_pile_sum_index(c, b0, a.bases)];
            }
            ref_code = (a.t_packed[b0 >> 4] >> (2 * (b0 & 15))) & 3u;
            ref_inv = (a.t_invmask[b0 >> 5] >> (b0 & 31)) & 1u;
        }
    }

    // One position after the other, in a loop that is not unrolled: unrolled, the four cost computations of a wide lane are
    // interleaved over more than 190 registers, which leaves two waves per SIMD to hide the loads of a streaming kernel.
    // The loop always looks at component 0 and then rotates the components (register moves, no runtime index); after four
    // turns they are where they were, for the writing pass.
    const auto rotate = [&] {
        if constexpr (WIDE) {
#pragma unroll
            for (uint32_t c = 0; c < 4; ++c) {
                const uint32_t tn = n[0][c], tq = Q[0][c];
                n[0][c] = n[1][c], n[1][c] = n[2][c], n[2][c] = n[3][c], n[3][c] = tn;
                Q[0][c] = Q[1][c], Q[1][c] = Q[2][c], Q[2][c] = Q[3][c], Q[3][c] = tq;
            }
        }
    };
    const auto ref_column_of = [&](uint32_t k) { return dcn_pile_column((ref_code >> (2 * k)) & 3u, (ref_inv >> k) & 1u); };
    uint32_t site_mask = 0, gt_word = 0, gq_word = 0;
#pragma unroll 1
    for (uint32_t k = 0; k < PER; ++k) {
        const uint64_t b = b0 + k;
        const bool inside = b >= a.base0 && b < end;
        uint8_t pl[DCN_GENO_GENOTYPES]; // (not looked at here: the compiler drops the ten quotients)
        const dcn_geno_result r = dcn_genotype_decide(n[0], Q[0], ref_column_of(k), prm, pl);
        if (inside && r.site) site_mask |= 1u << k;
        gt_word |= (inside ? r.gt : DCN_GENO_NONE) << (8 * k);
        gq_word |= (inside ? r.gq : 0u) << (8 * k);
        rotate();
    }
    if (!WRITE && b0 < end) {
        if constexpr (WIDE) { // byte (b - first) of the padded buffers: a word per lane
            reinterpret_cast<uint32_t *>(a.gt)[slot] = gt_word;
            reinterpret_cast<uint32_t *>(a.gq)[slot] = gq_word;
        } else {
            const uint64_t at = (a.base0 & 3u) + slot;
            a.gt[at] = (uint8_t)gt_word;
            a.gq[at] = (uint8_t)gq_word;
        }
    }

    // the sites of the lanes in front of this one in its wave, and of the waves in front of that
    const uint32_t mine = __popc(site_mask);
    uint32_t before;
    if constexpr (WIDE) {
        uint32_t incl = mine;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        before = incl - mine;
        if (lane == 63) s_wave[wave] = incl;
    } else {
        const unsigned long long sites = __ballot(site_mask != 0);
        before = (uint32_t)__popcll(sites & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave[wave] = (uint32_t)__popcll(sites);
    }
    __syncthreads();
    if (!WRITE) {
        if (threadIdx.x == 0) a.block_counts[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    } else if (site_mask) {
        uint64_t at = a.block_offsets[blockIdx.x] + before;
        for (uint32_t v = 0; v < wave; ++v) at += s_wave[v];
#pragma unroll 1
        for (uint32_t k = 0; k < PER; ++k) {
            if (site_mask & (1u << k)) { // (decided a second time, for the few lanes with a site: only the mask lives across the barrier)
                uint8_t pl[DCN_GENO_GENOTYPES];
                const dcn_geno_result r = dcn_genotype_decide(n[0], Q[0], ref_column_of(k), prm, pl);
                write_site(a, at++, b0 + k, n[0], ref_column_of(k), r, pl);
            }
            rotate();
        }
    }
}

uint64_t slots_of(uint64_t base0, uint64_t n) { // lanes with a position of the range
    if (n == 0) return 0;
    return WIDE ? ((base0 + n + 3) >> 2) - (base0 >> 2) : n;
}
} // namespace

uint32_t dcn_genotype_blocks(uint64_t base0, uint64_t n) { return (uint32_t)((slots_of(base0, n) + GENO_THREADS - 1) / GENO_THREADS); }

uint64_t dcn_genotype_out_bytes(uint64_t base0, uint64_t n) { return (((base0 + n + 3) >> 2) - (base0 >> 2)) * 4; }

int dcn_launch_genotype(const dcn_genotype_args &args, bool write, hipStream_t stream) {
    if (args.n == 0) return DCN_OK;
    const dim3 grid(dcn_genotype_blocks(args.base0, args.n)), block(GENO_THREADS);
    if (write) hipLaunchKernelGGL(genotype_kernel<true>, grid, block, 0, stream, args);
    else hipLaunchKernelGGL(genotype_kernel<false>, grid, block, 0, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

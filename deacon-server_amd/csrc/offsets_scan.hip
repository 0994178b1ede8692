// offsets_scan.hip -- per-read counts to CSR offsets (dcn_launch_offsets_scan, declared in dcn_dump_sweep.h): the
// exclusive scan behind dcn_locate_batch's segment offsets and dcn_place_split_batch's placement offsets.
//   offsets_scan_sums_kernel    a workgroup per DCN_SCAN_BLOCK counts: their sum -> block_sums[block]
//   offsets_scan_blocks_kernel  one workgroup: block_sums[] -> their exclusive prefix (64 bits)
//   offsets_scan_write_kernel   the block's prefix + the scan inside the block -> offsets[i + 1]; offsets[0] = 0
// Sums inside a block are 32 bits like the counts; what crosses blocks is 64 bits.
#include "dcn_dump_sweep.h"

namespace {

__device__ inline uint32_t scan_thread_sum(const uint32_t *counts, uint32_t n, uint32_t i0) {
    uint32_t s = 0;
#pragma unroll
    for (uint32_t i = 0; i < DCN_SCAN_ITEMS; ++i)
        if (i0 + i < n) s += counts[i0 + i];
    return s;
}

// inclusive scan of one value per thread over the workgroup
__device__ inline uint32_t scan_block(uint32_t v, uint32_t *s_wave) {
    const uint32_t lane = threadIdx.x & (DCN_WAVE - 1), wave = threadIdx.x / DCN_WAVE;
    for (uint32_t d = 1; d < DCN_WAVE; d <<= 1) {
        const uint32_t o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    if (lane == DCN_WAVE - 1) s_wave[wave] = v;
    __syncthreads();
    for (uint32_t q = 0; q < wave; ++q) v += s_wave[q];
    return v;
}

__global__ __launch_bounds__(DCN_SCAN_THREADS) void offsets_scan_sums_kernel(const uint32_t *counts, uint32_t n,
                                                                             unsigned long long *block_sums) {
    __shared__ uint32_t s_wave[DCN_SCAN_THREADS / DCN_WAVE];
    const uint32_t i0 = blockIdx.x * DCN_SCAN_BLOCK + threadIdx.x * DCN_SCAN_ITEMS;
    const uint32_t incl = scan_block(scan_thread_sum(counts, n, i0), s_wave);
    if (threadIdx.x == DCN_SCAN_THREADS - 1) block_sums[blockIdx.x] = incl;
}

__global__ __launch_bounds__(DCN_SCAN_THREADS) void offsets_scan_blocks_kernel(unsigned long long *block_sums, uint32_t n_blocks) {
    __shared__ unsigned long long s_part[DCN_SCAN_THREADS];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (n_blocks + DCN_SCAN_THREADS - 1) / DCN_SCAN_THREADS;
    const uint32_t b0 = min(tid * per, n_blocks), b1 = min(b0 + per, n_blocks);
    unsigned long long mine = 0;
    for (uint32_t b = b0; b < b1; ++b) mine += block_sums[b];
    s_part[tid] = mine;
    __syncthreads();
    unsigned long long before = 0;
    for (uint32_t q = 0; q < tid; ++q) before += s_part[q];
    for (uint32_t b = b0; b < b1; ++b) {
        const unsigned long long v = block_sums[b];
        block_sums[b] = before;
        before += v;
    }
}

__global__ __launch_bounds__(DCN_SCAN_THREADS) void offsets_scan_write_kernel(const uint32_t *counts, uint32_t n,
                                                                              const unsigned long long *block_sums,
                                                                              uint64_t *offsets) {
    __shared__ uint32_t s_wave[DCN_SCAN_THREADS / DCN_WAVE];
    const uint32_t i0 = blockIdx.x * DCN_SCAN_BLOCK + threadIdx.x * DCN_SCAN_ITEMS;
    const uint32_t mine = scan_thread_sum(counts, n, i0);
    uint64_t at = block_sums[blockIdx.x] + (scan_block(mine, s_wave) - mine);
    if (i0 == 0) offsets[0] = 0;
    for (uint32_t i = 0; i < DCN_SCAN_ITEMS && i0 + i < n; ++i) {
        at += counts[i0 + i];
        offsets[i0 + i + 1] = at;
    }
}

} // namespace

int dcn_launch_offsets_scan(const uint32_t *counts, uint32_t n, unsigned long long *block_sums, uint64_t *offsets,
                            hipStream_t stream) {
    if (n == 0) return DCN_OK;
    const uint32_t blocks = (n + DCN_SCAN_BLOCK - 1) / DCN_SCAN_BLOCK;
    hipLaunchKernelGGL(offsets_scan_sums_kernel, dim3(blocks), dim3(DCN_SCAN_THREADS), 0, stream, counts, n, block_sums);
    hipLaunchKernelGGL(offsets_scan_blocks_kernel, dim3(1), dim3(DCN_SCAN_THREADS), 0, stream, block_sums, blocks);
    hipLaunchKernelGGL(offsets_scan_write_kernel, dim3(blocks), dim3(DCN_SCAN_THREADS), 0, stream, counts, n,
                       (const unsigned long long *)block_sums, offsets);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

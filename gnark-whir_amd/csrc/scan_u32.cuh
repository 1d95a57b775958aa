// The library's one global exclusive scan of u32: the single-wave kernels, the wave scans they are made of and the host driver.  Shared
// by msm.hip (whose fused kernels add up the block sums themselves: sums_ready) and setup.hip.
// The kernels are static: every translation unit that includes this header carries its own copy of the ones it launches.
#pragma once
#include "ctx.h"
#include "field.cuh"

// ---------------------------------------------------------------- exclusive scan of u32 (out has m+1 entries, out[m] = total)
// Every kernel of this family is a grid of SINGLE-WAVE workgroups (64 threads, scans by wave shuffles, no LDS, no barrier).  These launches
// sit between the heavy kernels of an MSM's chain, and beside them run the level-1 accumulations of the other MSMs, whose one-wave
// workgroups keep every SIMD's register file full: a four-wave workgroup needs a free slot on all four SIMDs of one CU at the same
// moment (rocprofv3: k_scan_block_sums 3.7 ms inside a proof, 12 us alone), one wave takes any slot.  Measured on the job and on the
// single proof: no difference either way (the freed slots go to the accumulations' next workgroups first); kept for the simpler kernels.
static constexpr u32 SCAN_PER_THREAD = 16, SCAN_THREADS = 64, SCAN_BLOCK = SCAN_PER_THREAD * SCAN_THREADS;
static constexpr u32 SCAN_MAX_INLINE_BLOCKS = 8 * SCAN_THREADS;   // mode 2 of k_scan_final: every workgroup scans the block sums itself, eight per lane
__device__ __forceinline__ u32 wave_inclusive_scan(u32 v) {
    for (int off = 1; off < 64; off <<= 1) { const u32 o = (u32)__shfl_up((int)v, off); if ((int)(threadIdx.x & 63) >= off) v += o; }
    return v;
}
__device__ __forceinline__ u32 wave_exclusive_scan(u32 v, u32 *total) {
    const u32 incl = wave_inclusive_scan(v);
    *total = (u32)__shfl((int)incl, 63);
    return incl - v;
}
static __global__ void __launch_bounds__(64) k_scan_block_sums(const u32 *in, size_t m, u32 *block_sums) {
    size_t base = (size_t)blockIdx.x * SCAN_BLOCK + (size_t)threadIdx.x * SCAN_PER_THREAD;
    u32 s = 0;
    for (u32 k = 0; k < SCAN_PER_THREAD; k++) if (base + k < m) s += in[base + k];
    u32 total;
    wave_exclusive_scan(s, &total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}
static __global__ void __launch_bounds__(64) k_scan_of_sums(u32 *block_sums, u32 nblocks) {  // single workgroup, in place; eight sums per lane per trip
    u32 carry = 0;
    for (u32 base = 0; base < nblocks; base += 8 * 64) {
        const u32 i0 = base + threadIdx.x * 8;
        u32 v[8], mine = 0;
        for (u32 k = 0; k < 8; k++) { v[k] = i0 + k < nblocks ? block_sums[i0 + k] : 0; mine += v[k]; }
        u32 total;
        u32 ex = carry + wave_exclusive_scan(mine, &total);
        for (u32 k = 0; k < 8; k++) { if (i0 + k < nblocks) block_sums[i0 + k] = ex; ex += v[k]; }
        carry += total;
    }
    if (threadIdx.x == 0) block_sums[nblocks] = carry;
}
// mode 0: block_sums holds the exclusive scan of the block sums (+ the total at [gridDim.x]) -- after k_scan_of_sums
// mode 1: a single block: no block sums at all
// mode 2: block_sums holds the raw sums of <= SCAN_MAX_INLINE_BLOCKS blocks: every workgroup scans them itself (saves the k_scan_of_sums launch)
// The block that writes out[m] can also leave words in PINNED HOST memory (device-visible: hipHostMalloc) for the enqueueing thread: the
// total (total_host) and one more word (copy_src -> copy_host: the sort's fullest bucket).  A hipMemcpyAsync of four bytes is a blit KERNEL
// (__amd_rocclr_copyBuffer: 22 per proof, ~60 us each inside the job, every one on an MSM's chain); a store from a kernel that runs anyway is not.
static __global__ void __launch_bounds__(64) k_scan_final(const u32 *in, size_t m, const u32 *block_sums, u32 *out, int mode,
                                                   u32 *total_host = nullptr, const u32 *copy_src = nullptr, u32 *copy_host = nullptr) {
    u32 offset = 0, grand = 0;
    if (mode == 0) { offset = block_sums[blockIdx.x]; grand = block_sums[gridDim.x]; }
    if (mode == 2) {   // lane t holds the sums of blocks 8 t .. 8 t + 7; this block's offset = sums of the blocks before it
        const u32 i0 = threadIdx.x * 8;
        u32 mine = 0, before_in_lane = 0;
        for (u32 k = 0; k < 8; k++) {
            const u32 v = i0 + k < gridDim.x ? block_sums[i0 + k] : 0;
            if (i0 + k < blockIdx.x) before_in_lane += v;
            mine += v;
        }
        const u32 ex = wave_exclusive_scan(mine, &grand);
        const u32 owner = blockIdx.x >> 3;   // the lane that holds this block's sum
        offset = (u32)__shfl((int)(ex + before_in_lane), (int)owner);
    }
    size_t base = (size_t)blockIdx.x * SCAN_BLOCK + (size_t)threadIdx.x * SCAN_PER_THREAD;
    u32 v[SCAN_PER_THREAD], s = 0;
    for (u32 k = 0; k < SCAN_PER_THREAD; k++) { v[k] = base + k < m ? in[base + k] : 0; s += v[k]; }
    u32 total;
    u32 ex = wave_exclusive_scan(s, &total) + offset;
    for (u32 k = 0; k < SCAN_PER_THREAD; k++) {
        if (base + k < m) out[base + k] = ex;
        ex += v[k];
    }
    if (mode == 1) grand = total;
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        out[m] = grand;
        if (total_host) *total_host = grand;
        if (copy_host) *copy_host = *copy_src;
    }
}
// total_host / copy_src -> copy_host: words the last kernel also leaves in pinned host memory (k_scan_final), or null
// sums_ready: a kernel of the caller's has left the raw sums of the (<= SCAN_MAX_INLINE_BLOCKS) blocks in tmp: only the last kernel is launched
static int32_t exclusive_scan(mi_ctx *ctx, hipStream_t st, const u32 *in, size_t m, u32 *out, DevBuf &tmp,
                              u32 *total_host = nullptr, const u32 *copy_src = nullptr, u32 *copy_host = nullptr, bool sums_ready = false) {
    u32 nblocks = (u32)((m + SCAN_BLOCK - 1) / SCAN_BLOCK);
    if (nblocks == 0) nblocks = 1;
    MI_TRY(mi_reserve(ctx, tmp, (size_t)(nblocks + 1) * 4));
    u32 *bs = (u32 *)tmp.p;
    const int mode = nblocks == 1 && !sums_ready ? 1 : nblocks <= SCAN_MAX_INLINE_BLOCKS ? 2 : 0;   // (k_scan_final's modes)
    if (mode != 1 && !sums_ready) hipLaunchKernelGGL(k_scan_block_sums, dim3(nblocks), dim3(SCAN_THREADS), 0, st, in, m, bs);
    if (mode == 0) hipLaunchKernelGGL(k_scan_of_sums, dim3(1), dim3(SCAN_THREADS), 0, st, bs, nblocks);
    hipLaunchKernelGGL(k_scan_final, dim3(nblocks), dim3(SCAN_THREADS), 0, st, in, m, bs, out, mode, total_host, copy_src, copy_host);
    MI_CHECK_HIP(ctx, hipGetLastError());
    return MI_OK;
}

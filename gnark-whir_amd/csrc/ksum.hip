// kSum of a whole batch over a window table of the key's K[1..] (include/mi355x_groth16_verify_ksum.h).  The per-lane text is
// ksum_ops.cuh, which the host build of the tests runs too; this file holds the kernels around it, the build of a key's table and the
// four entry points.  Every launch goes to ctx->stream.
//
// The table (mi_vk::ksum), built once per key:
//   k_ksum_rows        one lane per base: 2^(c w) K_j for every window, by doublings down the lane -> XYZZ rows
//   k_ksum_multiples   one lane per (j, w) of a chunk: d row for 1 <= d < 2^c by repeated addition -> XYZZ entries
//   k_xyzz_batch_to_affine   the chunk's entries to affine, one inversion per 16 (batch_affine.cuh's mi_xyzz_to_affine_enqueue)
// in chunks of MI_KSUM_BUILD_CHUNK entries, so the scratch of a build is bounded whatever the table's size.  Rows, entries and running
// products are allocations of the build alone, freed when it ends; when they or the table are not to be had the key stays without a
// table (MI_KSUM_NO_MEMORY), which is no error.
// The sums of a batch of n rows, three launches whatever n is (mi_ksum_enqueue):
//   k_ksum_partial     one lane per (row, slice of the row's (j, w) terms): ksum_lane -> one XYZZ partial sum
//   k_ksum_reduce      ksum_reduce_lanes(slices) lanes per row: each adds a stride of the row's partials, then a tree over LDS -> one XYZZ sum
//   k_xyzz_batch_to_affine   the sums to affine
// Rows whose skip byte is set are neither read nor summed: their sum is written as infinity by the second launch.  Grids are capped at
// MI_KSUM_GRID_CAP workgroups of 64 lanes, which walk their items with the grid's stride.  The scratch (partials | sums | running
// products) is the caller's: a region of WS_VERIFY, cut by the stage of a batch (verify.hip) or by the entry points here.
#include "verify_internal.h"
#include "ksum_ops.cuh"
#include "batch_affine.cuh"
#include <chrono>
#include <cstring>

namespace {

__global__ void __launch_bounds__(64) k_ksum_rows(const G1Aff *k, u32 ns, u32 c, u32 windows, G1X *rows) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ns) return;
    ksum_rows_lane(k[j], c, windows, rows + (size_t)j * windows);
}
__global__ void __launch_bounds__(64) k_ksum_multiples(const G1X *rows, size_t n_rows, u32 entries, G1X *out) {
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    ksum_multiples_lane(rows[r], entries, out + r * entries);
}
__global__ void __launch_bounds__(64) k_ksum_partial(const G1Aff *table, const Fr *scal, const uint8_t *skip, u32 ns, u32 c, u32 slices, uint64_t slice_terms,
                                                     size_t n, G1X *part) {
    const uint64_t terms = (uint64_t)ns * ksum_windows(c), lanes = (uint64_t)n * slices, stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < lanes; t += stride) {
        const uint64_t i = t / slices, s = t - i * slices;
        if (skip && skip[i]) continue;
        const uint64_t t0 = s * slice_terms, t1 = t0 + slice_terms < terms ? t0 + slice_terms : terms;
        part[t] = t0 < terms ? ksum_lane(table, scal + i * ns, c, t0, t1) : G1X::inf();
    }
}
// lanes_per_row: a power of two, at most 64; a workgroup takes 64 / lanes_per_row rows at a time
__global__ void __launch_bounds__(64) k_ksum_reduce(const G1X *part, const uint8_t *skip, u32 slices, u32 lanes_per_row, size_t n, G1X *sums) {
    __shared__ G1X sh[64];
    const u32 rows_per_wg = 64 / lanes_per_row, g = threadIdx.x / lanes_per_row, sub = threadIdx.x % lanes_per_row;
    const uint64_t items = ((uint64_t)n + rows_per_wg - 1) / rows_per_wg;
    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint64_t i = item * rows_per_wg + g;
        const bool live = i < n && !(skip && skip[i]);
        G1X acc = live ? ksum_strided_sum(part + i * slices, slices, sub, lanes_per_row) : G1X::inf();
        for (u32 h = lanes_per_row >> 1; h; h >>= 1) {   // the same trip count in every lane of the workgroup
            sh[threadIdx.x] = acc;
            __syncthreads();
            if (sub < h) {
                const G1X other = sh[threadIdx.x + h];
                xyzz_add(acc, other);
            }
            __syncthreads();
        }
        if (sub == 0 && i < n) sums[i] = acc;
    }
}

unsigned capped_blocks(uint64_t lanes) {
    const uint64_t b = (lanes + 63) / 64;
    return (unsigned)(b < MI_KSUM_GRID_CAP ? b : MI_KSUM_GRID_CAP);
}

struct KsumScratch { size_t part, sums, prefix, total; };
KsumScratch scratch_of(u32 ns, u32 c, size_t n) {
    WsCut cut;
    KsumScratch s;
    s.part = cut.take(n * ksum_slices(ns, c, n) * sizeof(G1X));
    s.sums = cut.take(n * sizeof(G1X));
    s.prefix = cut.take(n * sizeof(Fp));
    s.total = cut.total;
    return s;
}

void drop_table(mi_vk::Ksum &k) {
    if (k.table) (void)hipFree(k.table);
    k.table = nullptr; k.c = 0; k.bytes = 0;
}
bool try_alloc(void **p, size_t bytes) {
    if (hipMalloc(p, bytes) == hipSuccess) return true;
    (void)hipGetLastError();
    *p = nullptr;
    return false;
}

// the key's table under `budget`, replacing the one it has
int32_t build_table(mi_ctx *ctx, const mi_vk *vk, uint64_t budget) {
    mi_vk::Ksum &k = vk->ksum;
    const auto t0 = std::chrono::steady_clock::now();
    MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // nothing in flight reads the table that goes
    drop_table(k);
    k.budget = budget; k.build_ms = 0;
    const u32 ns = vk->ksum_bases(), c = ksum_window_bits(ns, budget);
    if (!ns) { k.state = MI_KSUM_NO_BASES; return MI_OK; }
    if (!c) { k.state = MI_KSUM_OVER_BUDGET; return MI_OK; }
    const u32 windows = ksum_windows(c), entries = (u32)ksum_row_entries(c);
    const size_t n_rows = (size_t)ns * windows, bytes = ksum_table_bytes(ns, c);
    const size_t chunk_rows = MI_KSUM_BUILD_CHUNK / entries < n_rows ? MI_KSUM_BUILD_CHUNK / entries : n_rows;
    void *table = nullptr, *rows = nullptr, *xyzz = nullptr, *prefix = nullptr;
    auto body = [&]() -> int32_t {
        if (!try_alloc(&table, bytes) || !try_alloc(&rows, n_rows * sizeof(G1X)) || !try_alloc(&xyzz, chunk_rows * entries * sizeof(G1X)) ||
            !try_alloc(&prefix, chunk_rows * entries * sizeof(Fp))) {
            k.state = MI_KSUM_NO_MEMORY;
            return MI_OK;
        }
        MI_TRY(mi_launch64(ctx, k_ksum_rows, ns, (const G1Aff *)vk->k_dev, ns, c, windows, (G1X *)rows));
        for (size_t r0 = 0; r0 < n_rows; r0 += chunk_rows) {
            const size_t m = n_rows - r0 < chunk_rows ? n_rows - r0 : chunk_rows, cnt = m * entries;
            MI_TRY(mi_launch64(ctx, k_ksum_multiples, m, (const G1X *)rows + r0, m, entries, (G1X *)xyzz));
            MI_TRY(mi_xyzz_to_affine_enqueue<Fp>(ctx, (const G1X *)xyzz, (G1Aff *)table + r0 * entries, (Fp *)prefix, cnt));
        }
        MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        k.table = (G1Aff *)table; table = nullptr;
        k.c = c; k.bytes = bytes; k.state = MI_KSUM_READY;
        return MI_OK;
    };
    const int32_t rc = body();
    if (rc != MI_OK) (void)hipStreamSynchronize(ctx->stream);
    for (void *p : {table, rows, xyzz, prefix})
        if (p) (void)hipFree(p);
    k.build_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

// the checks the two batch calls share, under their prefix
int32_t batch_args(mi_ctx *ctx, const mi_vk *vk, const void *scalars, size_t n, const void *out) {
    if (!ctx) return MI_EINVAL;
    if (!vk) MI_FAIL(ctx, MI_EINVAL, "ksum: vk is null");
    if (n > ((size_t)1 << 24)) MI_FAIL(ctx, MI_EINVAL, "ksum: n is above 2^24");
    if (n && !scalars) MI_FAIL(ctx, MI_EINVAL, "ksum: scalars is null");
    if (n && !out) MI_FAIL(ctx, MI_EINVAL, "ksum: out is null");
    if (n && !vk->ksum_bases()) MI_FAIL(ctx, MI_EINVAL, "ksum: the key has no bases (nb_public + n_commitments is 1)");
    if (n && !vk->ksum.table) MI_FAIL(ctx, MI_EINVAL, "ksum: the key has no table (mi_vk_ksum_prepare builds one; mi_vk_ksum_get_info says why it has none)");
    return MI_OK;
}

}   // namespace

int32_t mi_ksum_ready(mi_ctx *ctx, const mi_vk *vk, bool *ready) {
    if (vk->ksum.state == MI_KSUM_NOT_BUILT) MI_TRY(build_table(ctx, vk, vk->ksum.budget));
    *ready = vk->ksum.table != nullptr;
    return MI_OK;
}
size_t mi_ksum_scratch_bytes(const mi_vk *vk, size_t n) { return scratch_of(vk->ksum_bases(), vk->ksum.c, n).total; }
int32_t mi_ksum_enqueue(mi_ctx *ctx, const mi_vk *vk, const Fr *scal_dev, const uint8_t *skip_dev, size_t n, G1Aff *out_dev, char *scratch, uint64_t *launches) {
    if (!n) return MI_OK;
    const u32 ns = vk->ksum_bases(), c = vk->ksum.c, slices = ksum_slices(ns, c, n), lanes_per_row = ksum_reduce_lanes(slices);
    const KsumScratch at = scratch_of(ns, c, n);
    G1X *part = (G1X *)(scratch + at.part), *sums = (G1X *)(scratch + at.sums);
    hipLaunchKernelGGL(k_ksum_partial, dim3(capped_blocks((uint64_t)n * slices)), dim3(64), 0, ctx->stream, (const G1Aff *)vk->ksum.table, scal_dev, skip_dev, ns, c,
                       slices, ksum_slice_terms(ns, c, slices), n, part);
    MI_CHECK_HIP(ctx, hipGetLastError());
    const uint64_t items = ((uint64_t)n + 64 / lanes_per_row - 1) / (64 / lanes_per_row);
    hipLaunchKernelGGL(k_ksum_reduce, dim3((unsigned)(items < MI_KSUM_GRID_CAP ? items : MI_KSUM_GRID_CAP)), dim3(64), 0, ctx->stream, (const G1X *)part, skip_dev,
                       slices, lanes_per_row, n, sums);
    MI_CHECK_HIP(ctx, hipGetLastError());
    MI_TRY(mi_xyzz_to_affine_enqueue<Fp>(ctx, (const G1X *)sums, out_dev, (Fp *)(scratch + at.prefix), n));
    if (launches) *launches += 3;
    return MI_OK;
}

extern "C" {

int32_t mi_vk_ksum_prepare(mi_ctx *ctx, mi_vk *vk, uint64_t max_table_bytes) {
    if (!ctx) return MI_EINVAL;
    if (!vk) MI_FAIL(ctx, MI_EINVAL, "ksum: vk is null");
    const uint64_t budget = max_table_bytes ? max_table_bytes : MI_KSUM_DEFAULT_TABLE_BYTES;
    if (vk->ksum.state != MI_KSUM_NOT_BUILT && vk->ksum.state != MI_KSUM_NO_MEMORY && vk->ksum.budget == budget) return MI_OK;
    return build_table(ctx, vk, budget);
}
int32_t mi_vk_ksum_get_info(mi_ctx *ctx, const mi_vk *vk, mi_vk_ksum_info *out) {
    if (!ctx) return MI_EINVAL;
    if (!vk) MI_FAIL(ctx, MI_EINVAL, "ksum: vk is null");
    if (!out) MI_FAIL(ctx, MI_EINVAL, "ksum: the info pointer is null");
    std::memset(out, 0, sizeof(*out));
    const mi_vk::Ksum &k = vk->ksum;
    out->window_bits = k.c; out->windows = k.c ? ksum_windows(k.c) : 0; out->table_bytes = k.bytes; out->bases = vk->ksum_bases();
    out->budget_bytes = k.budget; out->state = k.state; out->build_ms = k.build_ms;
    return MI_OK;
}
int32_t mi_vk_ksum_batch_dev(mi_ctx *ctx, const mi_vk *vk, const mi_fr *scalars_dev, const uint8_t *skip_dev, size_t n, mi_g1_affine *out_dev) {
    MI_TRY(batch_args(ctx, vk, scalars_dev, n, out_dev));
    if (!n) return MI_OK;
    MI_TRY(mi_reserve(ctx, ctx->ws[WS_VERIFY], mi_ksum_scratch_bytes(vk, n)));
    return mi_ksum_enqueue(ctx, vk, (const Fr *)scalars_dev, skip_dev, n, (G1Aff *)out_dev, (char *)ctx->ws[WS_VERIFY].p, nullptr);
}
int32_t mi_vk_ksum_batch(mi_ctx *ctx, const mi_vk *vk, const mi_fr *scalars, const uint8_t *skip, size_t n, mi_g1_affine *out) {
    MI_TRY(batch_args(ctx, vk, scalars, n, out));
    if (!n) return MI_OK;
    const u32 ns = vk->ksum_bases();
    WsCut cut;
    const size_t off_scal = cut.take(n * ns * sizeof(Fr)), off_skip = cut.take(n), off_out = cut.take(n * sizeof(G1Aff)), off_scratch = cut.take(mi_ksum_scratch_bytes(vk, n));
    MI_TRY(mi_reserve(ctx, ctx->ws[WS_VERIFY], cut.total));
    char *ws = (char *)ctx->ws[WS_VERIFY].p;
    MI_TRY(mi_verify_upload(ctx, ws + off_scal, scalars, n * ns * sizeof(Fr)));
    if (skip) MI_TRY(mi_verify_upload(ctx, ws + off_skip, skip, n));
    MI_TRY(mi_ksum_enqueue(ctx, vk, (const Fr *)(ws + off_scal), skip ? (const uint8_t *)(ws + off_skip) : nullptr, n, (G1Aff *)(ws + off_out), ws + off_scratch, nullptr));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(out, ws + off_out, n * sizeof(G1Aff), hipMemcpyDeviceToHost, ctx->stream));
    MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MI_OK;
}

}   // extern "C"

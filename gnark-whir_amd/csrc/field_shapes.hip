// mi_debug_field_shape_dev: one record of shape_ops.cuh per lane, one kernel per shape (test infrastructure; nothing in the product
// includes shape_ops.cuh or launches these kernels).
#include <utility>
#include "ctx.h"
#include "shape_ops.cuh"

static_assert(SH_IN_WORDS == MI_SHAPE_IN_WORDS && SH_OUT_WORDS == MI_SHAPE_OUT_WORDS, "the debug header mirrors shape_ops.cuh");

// the record goes through registers: every input word is read before the first result is written, every store is by lane index
template <int SHAPE>
__global__ void __launch_bounds__(64) k_field_shape(u32 *out, const u32 *in, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 r[SH_IN_WORDS], o[SH_OUT_WORDS];
#pragma unroll
    for (int w = 0; w < SH_IN_WORDS; w++) r[w] = in[i * SH_IN_WORDS + w];
#pragma unroll
    for (int w = 0; w < SH_OUT_WORDS; w++) o[w] = 0;
    shape_op<SHAPE>(r, o);
#pragma unroll
    for (int w = 0; w < SH_OUT_WORDS; w++) out[i * SH_OUT_WORDS + w] = o[w];
}

typedef void (*shape_launch_fn)(hipStream_t, unsigned, u32 *, const u32 *, size_t);
template <int SHAPE>
static void shape_launch(hipStream_t st, unsigned grid, u32 *out, const u32 *in, size_t n) {
    hipLaunchKernelGGL(k_field_shape<SHAPE>, dim3(grid), dim3(64), 0, st, out, in, n);
}
template <int... S>
static shape_launch_fn shape_launcher(int shape, std::integer_sequence<int, S...>) {
    static const shape_launch_fn table[] = {shape_launch<S>...};
    return table[shape];
}

extern "C" int32_t mi_debug_field_shape_dev(mi_ctx *ctx, int shape, void *out_dev, const void *in_dev, size_t n) {
    if (!ctx || shape < 0 || shape >= SH_OP_END || ((!out_dev || !in_dev) && n) || n > ((size_t)1 << 24)) return MI_EINVAL;
    if (!n) return MI_OK;
    shape_launcher(shape, std::make_integer_sequence<int, SH_OP_END>())(ctx->stream, (unsigned)((n + 63) / 64), (u32 *)out_dev, (const u32 *)in_dev, n);
    MI_CHECK_HIP(ctx, hipGetLastError());
    return MI_OK;
}

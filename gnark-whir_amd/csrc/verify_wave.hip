// groth16.Verify with one WAVE per pairing (include/mi355x_groth16_verify_wave.h): the second body of the verifier, beside mi_verify_run
// (verify.hip) -- same inputs, same verdict bytes, built for the latency of one proof.  The arithmetic is the phase text of
// fp12_wave.cuh / pairing_wave.cuh; the image of a wave is MI_WAVE_IMAGE_BYTES of LDS, and every workgroup is ONE wave of 64 lanes.
//
// One batch, every launch on ctx->stream.  The host half is mi_verify_run's, the same function: mi_verify_open (argument checks, the
// VerifyStage) under this body's prefix, then mi_verify_stage_pairs (verify.hip: the scalars up, the sums of every row over the key's
// window table and verify_assemble one lane per proof -- or, without a table, one mi_verify_msm per well-formed proof and verify_assemble
// on the host) -- so a malformed proof is decided exactly as there and its words stay out of the arithmetic.  Then
//   k_pairing_miller_wave   one workgroup per (proof, pair): a Miller loop, 384 B out.  The SAME launch carries the Bs checks, 64 proofs
//                           per workgroup and one lane each (wave_bs_in_subgroup: the 63-bit endomorphism test), in front of the pairs:
//                           the longest one-lane chain of the call starts first and runs beside the Miller waves, not before them
//   k_verify_judge_wave     one workgroup per (proof, equation): the product of the equation's Miller values, the final
//                           exponentiation, the comparison with e(alpha, beta)^s or 1 -> one byte; a flagged proof is skipped
//   k_verify_verdict_wave   one lane per proof: the verdict byte with verify_judge's precedence
// Everything lives in WS_VERIFY, laid out by one WsCut: nothing is allocated in steady state, and the old body may use the same context
// before and after.  A grid is capped at MI_WAVE_GRID_CAP workgroups, each walking its items with the grid's stride: the largest batch
// (2^24 proofs of 20 pairs) is more workgroups than a grid may have threads for, and a few thousand fill the device.
#include "verify_internal.h"
#include "../../include/mi355x_groth16_verify_wave.h"
#include "pairing_wave.cuh"
#include <chrono>
#include <cstring>
#include <vector>

namespace {

#define MI_WAVE_GRID_CAP ((size_t)4096)   // 16 workgroups per CU, four times what the registers admit at once; tests/test_gpu_verify_wave.py crosses it

// items 0 .. check_blocks): the Bs checks of proofs 64 item + lane; then one pair per item
__global__ void __launch_bounds__(64) k_pairing_miller_wave(const G1Aff *p, const G2Aff *q, Fp12 *out, size_t n_pairs, u32 pairs_per_proof,
                                                             uint8_t *flags, size_t n_checks) {
    __shared__ Fp2 im[MI_WAVE_IMAGE_RECORDS];
    const size_t check_blocks = (n_checks + 63) / 64, items = check_blocks + n_pairs;
    for (size_t item = blockIdx.x; item < items; item += gridDim.x) {
        if (item < check_blocks) {
            const size_t i = item * 64 + threadIdx.x;
            if (i < n_checks && !wave_bs_in_subgroup(q[i * pairs_per_proof])) flags[i] = 1;
            continue;
        }
        const size_t pair = item - check_blocks;
        wave_miller_loop(im, p + pair, q + pair);
        MI_WAVE_PHASE(w12_ph_store(lane, im, out + pair, MI_WAVE_S(0)));
    }
}
__global__ void __launch_bounds__(64) k_final_exp_wave(Fp12 *io, size_t n) {
    __shared__ Fp2 im[MI_WAVE_IMAGE_RECORDS];
    for (size_t item = blockIdx.x; item < n; item += gridDim.x) {
        MI_WAVE_PHASE(w12_ph_load(lane, im, MI_WAVE_S(0), io + item));
        wave_final_exp(im);
        MI_WAVE_PHASE(w12_ph_store(lane, im, io + item, MI_WAVE_S(0)));
    }
}
__global__ void __launch_bounds__(64) k_fp12_op_wave(int op, Fp12 *z, const Fp12 *x, const Fp12 *y, size_t n) {
    __shared__ Fp2 im[MI_WAVE_IMAGE_RECORDS];
    for (size_t item = blockIdx.x; item < n; item += gridDim.x) {
        MI_WAVE_PHASE(w12_ph_load(lane, im, MI_WAVE_S(1), x + item));
        MI_WAVE_PHASE(w12_ph_load(lane, im, MI_WAVE_S(2), (y ? y : x) + item));
        MI_WAVE_PHASE(if (lane < 6) im[MI_WAVE_S(0) + lane] = Fp2::zero());
        (void)wave_fp12_op(im, op);
        MI_WAVE_PHASE(w12_ph_store(lane, im, z + item, MI_WAVE_S(0)));
    }
}
// pass[n_eq i + eq] = equation eq of proof i holds; the byte of a flagged proof is not written (its verdict does not read it)
__global__ void __launch_bounds__(64) k_verify_judge_wave(const Fp12 *ml, u32 pairs_per_proof, const Fp12 *e_alpha_beta, const uint8_t *flags,
                                                           uint8_t *pass, size_t n) {
    __shared__ Fp2 im[MI_WAVE_IMAGE_RECORDS];
    __shared__ Fp12 one;
    const u32 n_eq = wave_equations(pairs_per_proof);
    if (threadIdx.x == 0) one = Fp12::one();
    __syncthreads();
    for (size_t item = blockIdx.x; item < n * n_eq; item += gridDim.x) {
        const size_t i = item / n_eq;
        const u32 eq = (u32)(item - i * n_eq);
        if (flags[i]) continue;   // one byte, read by every lane
        wave_judge_equation(im, ml + i * pairs_per_proof + wave_equation_first(eq), wave_equation_count(eq, pairs_per_proof),
                            eq ? &one : e_alpha_beta, pass + item);
    }
}
__global__ void __launch_bounds__(64) k_verify_verdict_wave(const uint8_t *flags, const uint8_t *pass, u32 n_eq, uint8_t *verdicts, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    verdicts[i] = wave_verdict(flags[i] != 0, pass + i * n_eq, n_eq);
}

// k over `items` single-wave workgroups (at most MI_WAVE_GRID_CAP of them: the kernels walk their items with the grid's stride) on
// ctx->stream, and the one checked hipGetLastError of a launch: mi_launch64's sibling by workgroup count.  No item, no launch
template <class K, class... A> int32_t mi_launch_waves(mi_ctx *ctx, K k, size_t items, A... args) {
    if (!items) return MI_OK;
    hipLaunchKernelGGL(k, dim3((unsigned)(items < MI_WAVE_GRID_CAP ? items : MI_WAVE_GRID_CAP)), dim3(MI_WAVE_LANES), 0, ctx->stream, args...);
    MI_CHECK_HIP(ctx, hipGetLastError());
    return MI_OK;
}

// Miller values of n_pairs pairs on the device and, in the same launch, the Bs checks of n_checks proofs (flags[i] = 1 where
// q[i * pairs_per_proof] is not a point of the r-torsion of the twist, else flags[i] stays)
int32_t miller_wave_enqueue(mi_ctx *ctx, const G1Aff *p_dev, const G2Aff *q_dev, size_t n_pairs, Fp12 *ml_dev, u32 pairs_per_proof, uint8_t *flags_dev,
                            size_t n_checks) {
    return mi_launch_waves(ctx, k_pairing_miller_wave, (n_checks + 63) / 64 + n_pairs, p_dev, q_dev, ml_dev, n_pairs, pairs_per_proof, flags_dev, n_checks);
}

struct SplitClock {   // the phase split of mi_debug_verify_wave_split: events on ctx->stream, read after the call's last wait
    hipEvent_t ev[5] = {};
    bool on = false;
    int32_t open(mi_ctx *ctx, bool want) {
        on = want;
        for (int i = 0; on && i < 5; i++) MI_CHECK_HIP(ctx, hipEventCreate(&ev[i]));
        return MI_OK;
    }
    int32_t mark(mi_ctx *ctx, int i) {
        if (on) MI_CHECK_HIP(ctx, hipEventRecord(ev[i], ctx->stream));
        return MI_OK;
    }
    ~SplitClock() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

}   // namespace

int32_t mi_verify_run_wave(mi_ctx *ctx, const mi_vk *vk, const mi_verify_input *in, size_t n, uint8_t *verdicts, const uint8_t *decode_malformed,
                           const Fr *pub_dev, float *split_ms) {
    const auto t0 = std::chrono::steady_clock::now();
    VerifyStage st;   // host: flags (range and curve checks), scalars
    MI_TRY(mi_verify_open(ctx, "verify wave: ", vk, in, n, verdicts || !n, decode_malformed, &st, pub_dev));
    if (split_ms) std::memset(split_ms, 0, MI_VERIFY_WAVE_SPLIT_PHASES * sizeof(float));
    if (!n) return MI_OK;
    const u32 np = verify_pairs_per_proof(st.nc), n_eq = wave_equations(np);
    SplitClock clk;
    MI_TRY(clk.open(ctx, split_ms != nullptr));
    VerifyPairs d;   // the host half, mi_verify_run's: a malformed proof is decided exactly as there; extra: the pass bytes
    MI_TRY(mi_verify_stage_pairs(ctx, vk, st, n * n_eq, &d));
    const auto t1 = std::chrono::steady_clock::now();
    // ---- device: Bs checks and Miller loops in one launch, one judgement per equation, the verdict bytes
    MI_TRY(clk.mark(ctx, 0));
    if (split_ms) {   // the split times the two halves of the first launch apart: two launches, the checks first
        MI_TRY(miller_wave_enqueue(ctx, d.p, d.q, 0, d.ml, np, d.flags, n));
        MI_TRY(clk.mark(ctx, 1));
        MI_TRY(miller_wave_enqueue(ctx, d.p, d.q, n * np, d.ml, np, d.flags, 0));
    } else {
        MI_TRY(miller_wave_enqueue(ctx, d.p, d.q, n * np, d.ml, np, d.flags, n));
    }
    MI_TRY(clk.mark(ctx, 2));
    MI_TRY(mi_launch_waves(ctx, k_verify_judge_wave, n * n_eq, (const Fp12 *)d.ml, np, (const Fp12 *)vk->e_alpha_beta_dev, (const uint8_t *)d.flags, d.extra, n));
    MI_TRY(mi_launch64(ctx, k_verify_verdict_wave, n, (const uint8_t *)d.flags, (const uint8_t *)d.extra, n_eq, d.verdicts, n));
    MI_TRY(clk.mark(ctx, 3));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(verdicts, d.verdicts, n, hipMemcpyDeviceToHost, ctx->stream));
    MI_TRY(clk.mark(ctx, 4));
    MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (split_ms) {
        split_ms[0] = std::chrono::duration<float, std::milli>(t1 - t0).count();
        for (int i = 0; i < 4; i++) MI_CHECK_HIP(ctx, hipEventElapsedTime(&split_ms[1 + i], clk.ev[i], clk.ev[i + 1]));
    }
    return MI_OK;
}

extern "C" {

int32_t mi_groth16_verify_wave(mi_ctx *ctx, const mi_vk *vk, const mi_verify_input *in, size_t n, uint8_t *verdicts) {
    return mi_verify_run_wave(ctx, vk, in, n, verdicts, nullptr);
}

// ---------------------------------------------------------------- debug surface (include/mi355x_groth16_debug.h)
int32_t mi_debug_pairing_wave_dev(mi_ctx *ctx, const mi_g1_affine *p_dev, const mi_g2_affine *q_dev, size_t n, mi_fp *gt_dev, uint32_t flags) {
    if (!ctx || (flags & ~MI_PAIRING_FINAL_EXP) || ((!p_dev || !q_dev || !gt_dev) && n) || n > ((size_t)1 << 24)) return MI_EINVAL;
    MI_TRY(miller_wave_enqueue(ctx, (const G1Aff *)p_dev, (const G2Aff *)q_dev, n, (Fp12 *)gt_dev, 1, nullptr, 0));
    return (flags & MI_PAIRING_FINAL_EXP) ? mi_launch_waves(ctx, k_final_exp_wave, n, (Fp12 *)gt_dev, n) : MI_OK;
}
int32_t mi_debug_fp12_op_wave_dev(mi_ctx *ctx, int op, mi_fp *z_dev, const mi_fp *x_dev, const mi_fp *y_dev, size_t n) {
    if (!ctx || op < 0 || op >= F12_OP_END || ((!z_dev || !x_dev) && n) || n > ((size_t)1 << 24)) return MI_EINVAL;
    return mi_launch_waves(ctx, k_fp12_op_wave, n, op, (Fp12 *)z_dev, (const Fp12 *)x_dev, (const Fp12 *)y_dev, n);
}
int32_t mi_debug_verify_wave_split(mi_ctx *ctx, const mi_vk *vk, const mi_verify_input *in, size_t n, uint8_t *verdicts, float *split_ms) {
    if (ctx && !split_ms) MI_FAIL(ctx, MI_EINVAL, "verify wave: null split pointer");
    return mi_verify_run_wave(ctx, vk, in, n, verdicts, nullptr, nullptr, split_ms);
}
}

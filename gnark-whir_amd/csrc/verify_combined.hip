// One verdict for a batch of proofs under one key (include/mi355x_groth16_verify_combined.h): the random linear combination of the
// per-proof equations.  The equations, the order of the pairs and the host half are in pairing_ops.cuh, the coefficients in
// combine_coeff.cuh; the host build of the tests (tests/emu/emu_verify_combined.cpp) runs the same text.
//
// One batch, every launch on ctx->stream:
//   host      mi_verify_open (verify.hip): the argument checks, then the VerifyStage of pairing_ops.cuh -- the range and curve checks of
//             every proof (verify_well_formed) and the scalar matrix
//   k_verify_g2_check (verify.hip)   Bs of every proof that passed them -> with the host's flags, the lowest malformed index.  If there
//             is one the batch ends here with verdict 3: nothing below runs.
//   host      the coefficients r_i (one SHA-256 each)
//   k_verify_combine_scalars / k_verify_combine_reduce   sum_i r_i s_ij for every column j of the scalar matrix, S = sum_i r_i, and
//             r_i c_i^k for the Pedersen equation: blocks over the proofs, one partial per (block, column), then one sum per column
//   MSMs      2 without commitments (1 for a key without a scalar column), 4 + n_commitments with: over the resident K[1..] with the
//             column sums, over Krs_i, over all C_ik, over pok_i with r_i, and per k over C_.k with r_i c_i^k (msm.hip; a base at infinity, (0, 0), contributes nothing there:
//             both of its level-1 additions skip it).  Their results come back to the host, which forms the tail pairs
//             (verify_combined_assemble: S K[0], S alpha, two additions, the negations)
//   k_g1_scale128   one lane per proof: r_i Ar_i, affine, in place
//   k_pairing_miller (verify.hip)   one lane per pair: the n pairs (r_i Ar_i, Bs_i) and the tail, ONE launch
//   k_fp12_product  the n + 3 Groth16 values down to one by a tree of fan-in 8, relaunched per level; then the Pedersen values
//   k_pairing_final_exp (verify.hip)   two lanes (one without commitments)
//   k_verify_combined_judge   one lane: both results against one -> the verdict byte
// The scaling is a kernel of its own in front of the Miller loops rather than fused into them: the tail pairs and the proofs' pairs
// then share one Miller launch (the tail would otherwise be a second, nearly empty one), the debug entry point measures the kernel
// the verifier runs, and the 64 bytes per proof that cross memory between the two are nothing beside a Miller loop.
// Everything of a batch lives in ONE grow-only workspace (WS_VERIFY, which mi_groth16_verify_batch uses too: the calls of a context
// are serial on its stream), laid out by a WsCut: nothing is allocated in steady state.  Launches go through mi_launch64, the MSMs
// through mi_verify_msm (verify_internal.h).
#include "verify_internal.h"
#include "combine_coeff.cuh"
#include <sys/random.h>
#include <cstring>
#include <string>
#include <vector>

namespace {

#define MI_COMBINE_MAX_BLOCKS 256   // blocks over the proofs in k_verify_combine_scalars: 2^24 proofs are 1024 per lane

// scal: n x ns Montgomery scalars, row-major.  r: n coefficients as canonical Fr records (below 2^128).  fold: n challenges, or null when
// the key has at most one commitment (c_i = 1).  nb * (ns + 1) blocks: block j * nb + b adds up column j over the proofs b * 64 + lane,
// + nb * 64, ...; column ns is S, and its blocks also write r_i c_i^k (Montgomery) and r_i again (canonical) at [k * n + i] for the
// MSMs over the commitments.  partial[j * nb + b].  Exact field arithmetic: the order of the additions does not reach the result.
__global__ void __launch_bounds__(64, 1) k_verify_combine_scalars(const Fr *scal, u32 ns, const Fr *r, const Fr *fold, u32 nc, size_t n, u32 nb,
                                                                  Fr *partial, Fr *rc, Fr *rrep) {
    __shared__ Fr sh[64];
    const u32 j = blockIdx.x / nb, b = blockIdx.x % nb, lane = threadIdx.x;
    Fr acc = Fr::zero();
    for (size_t i = (size_t)b * 64 + lane; i < n; i += (size_t)nb * 64) {
        const Fr plain = r[i];
        const Fr ri = fe_to_mont(plain);
        if (j < ns) {
            acc = acc + ri * scal[i * ns + j];
        } else {
            acc = acc + ri;
            const Fr c = fold ? fold[i] : Fr::one();
            Fr pw = ri;
            for (u32 k = 0; k < nc; k++) {
                rc[(size_t)k * n + i] = pw;
                rrep[(size_t)k * n + i] = plain;
                pw = pw * c;
            }
        }
    }
    sh[lane] = acc;
    __syncthreads();
    for (u32 s = 32; s > 0; s >>= 1) {
        if (lane < s) sh[lane] = sh[lane] + sh[lane + s];
        __syncthreads();
    }
    if (lane == 0) partial[(size_t)j * nb + b] = sh[0];
}
// sums[j] = the sum of column j's nb partials
__global__ void __launch_bounds__(64, 1) k_verify_combine_reduce(const Fr *partial, u32 nb, Fr *sums, u32 n_cols) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_cols) return;
    Fr acc = Fr::zero();
    for (u32 b = 0; b < nb; b++) acc = acc + partial[(size_t)j * nb + b];
    sums[j] = acc;
}
// out[i] = k_i p[i]; k_i = the four words at k + i * stride (stride 8: canonical Fr records below 2^128).  out may be p.
__global__ void __launch_bounds__(64, 1) k_g1_scale128(const G1Aff *p, const u32 *k, u32 stride, G1Aff *out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const G1Aff pp = p[i];
    u32 kk[4];
    for (int w = 0; w < 4; w++) kk[w] = k[i * stride + w];
    out[i] = g1_scale128(pp, kk);
}
// out[j] = x[8 j] x[8 j + 1] ... (the last run may be shorter), j < n_out = ceil(n / 8)
__global__ void __launch_bounds__(64, 1) k_fp12_product(const Fp12 *x, size_t n, Fp12 *out, size_t n_out) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_out) return;
    const size_t at = j * MI_FP12_PRODUCT_FAN_IN, left = n - at;
    Fp12 f;
    fp12_product_run(&f, x + at, left < MI_FP12_PRODUCT_FAN_IN ? left : MI_FP12_PRODUCT_FAN_IN);
    out[j] = f;
}
// res[0] = the Groth16 product after its final exponentiation, res[1] = the Pedersen one (read with has_ped only)
__global__ void __launch_bounds__(64, 1) k_verify_combined_judge(const Fp12 *res, u32 has_ped, uint8_t *verdict) {
    if (blockIdx.x || threadIdx.x) return;
    *verdict = verify_combined_judge(&res[0], has_ped ? &res[1] : nullptr);
}

size_t product_level(size_t m) { return (m + MI_FP12_PRODUCT_FAN_IN - 1) / MI_FP12_PRODUCT_FAN_IN; }
// *out = x[0] ... x[m - 1], m >= 1: levels of k_fp12_product that alternate between t0 (product_level(m) records) and t1
// (product_level(product_level(m))); the last level writes out
int32_t fp12_product_enqueue(mi_ctx *ctx, const Fp12 *x, size_t m, Fp12 *t0, Fp12 *t1, Fp12 *out) {
    for (int level = 0;; level++) {
        const size_t m_out = product_level(m);
        Fp12 *dst = m_out == 1 ? out : (level & 1) ? t1 : t0;
        MI_TRY(mi_launch64(ctx, k_fp12_product, m_out, x, m, dst, m_out));
        if (m_out == 1) return MI_OK;
        x = dst;
        m = m_out;
    }
}

}   // namespace

// the two kernels for verify_locate.hip, which keeps every level of the product and scales into trees of its own
int32_t mi_fp12_product_level_enqueue(mi_ctx *ctx, const Fp12 *x_dev, size_t m, Fp12 *out_dev, size_t m_out) {
    return mi_launch64(ctx, k_fp12_product, m_out, x_dev, m, out_dev, m_out);
}
int32_t mi_g1_scale128_enqueue(mi_ctx *ctx, const G1Aff *p_dev, const u32 *k_dev, u32 stride, G1Aff *out_dev, size_t n) {
    return mi_launch64(ctx, k_g1_scale128, n, p_dev, k_dev, stride, out_dev, n);
}

int32_t mi_verify_combined_run(mi_ctx *ctx, const mi_vk *vk, const mi_verify_input *in, size_t n, const uint8_t *seed, uint8_t *verdict,
                               uint64_t *first_malformed, const uint8_t *decode_malformed, const Fr *pub_dev) {
    // refused where it always was, between mi_verify_open's checks of ctx, vk, in, verdict and n and those of the proofs' pointers
    if (ctx && vk && in && verdict && n <= ((size_t)1 << 24) && (uint64_t)n * vk->n_commitments > MI_MSM_MAX_PAIRS)
        MI_FAIL(ctx, MI_EINVAL, "verify combined: n * n_commitments above MI_MSM_MAX_PAIRS (one MSM runs over every commitment of the batch)");
    VerifyStage st;   // host: the range and curve checks of every proof, the scalar matrix
    MI_TRY(mi_verify_open(ctx, "verify combined: ", vk, in, n, verdict != nullptr, decode_malformed, &st, pub_dev));
    const u32 nc = st.nc, ns = st.ns, np = verify_combined_tail_pairs(nc);
    uint8_t own_seed[32];
    if (!seed && n) {
        for (size_t got = 0; got < sizeof(own_seed);) {
            const ssize_t k = getrandom(own_seed + got, sizeof(own_seed) - got, 0);
            if (k <= 0) MI_FAIL(ctx, MI_ENODEV, "verify combined: the operating system gave no randomness for the seed (getrandom)");
            got += (size_t)k;
        }
        seed = own_seed;
    }
    if (first_malformed) *first_malformed = n;
    if (!n) { *verdict = MI_VERIFY_OK; return MI_OK; }

    // ---- workspace
    const u32 nb = mi_blocks_of(n, 64) < MI_COMBINE_MAX_BLOCKS ? mi_blocks_of(n, 64) : MI_COMBINE_MAX_BLOCKS;
    const size_t lvl0 = product_level(n + np), lvl1 = product_level(lvl0);
    WsCut cut;
    const size_t off_scal = cut.take(n * ns * sizeof(Fr)), off_r = cut.take(n * sizeof(Fr)), off_fold = cut.take(n * sizeof(Fr));
    const size_t off_part = cut.take((size_t)(ns + 1) * nb * sizeof(Fr)), off_sum = cut.take((size_t)(ns + 1) * sizeof(Fr));
    const size_t off_rc = cut.take(n * nc * sizeof(Fr)), off_rrep = cut.take(n * nc * sizeof(Fr));
    const size_t off_krs = cut.take(n * sizeof(G1Aff)), off_pok = cut.take(n * sizeof(G1Aff)), off_cm = cut.take(n * nc * sizeof(G1Aff));
    const size_t off_p = cut.take((n + np) * sizeof(G1Aff)), off_q = cut.take((n + np) * sizeof(G2Aff)), off_ml = cut.take((n + np) * sizeof(Fp12));
    const size_t off_t0 = cut.take(lvl0 * sizeof(Fp12)), off_t1 = cut.take(lvl1 * sizeof(Fp12)), off_res = cut.take(2 * sizeof(Fp12));
    const size_t off_fl = cut.take(n), off_vd = cut.take(1);
    MI_TRY(mi_reserve(ctx, ctx->ws[WS_VERIFY], cut.total));
    char *ws = (char *)ctx->ws[WS_VERIFY].p;

    // ---- malformed first: Bs of the proofs that passed the host's checks (infinity stands in for the others)
    std::vector<G2Aff> Q(n + np, G2Aff{Fp2::zero(), Fp2::zero()});
    for (size_t i = 0; i < n; i++)
        if (!st.flags[i]) Q[i] = *st.proofs[i].bs;
    MI_CHECK_HIP(ctx, hipMemcpyAsync(ws + off_q, Q.data(), n * sizeof(G2Aff), hipMemcpyHostToDevice, ctx->stream));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(ws + off_fl, st.flags.data(), n, hipMemcpyHostToDevice, ctx->stream));
    MI_TRY(mi_verify_g2_check_enqueue(ctx, (const G2Aff *)(ws + off_q), 1, (uint8_t *)(ws + off_fl), n));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(st.flags.data(), ws + off_fl, n, hipMemcpyDeviceToHost, ctx->stream));
    MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    st.merge(st.flags.data());
    if (st.first_flagged < n) {
        *verdict = MI_VERIFY_MALFORMED;
        if (first_malformed) *first_malformed = st.first_flagged;
        return MI_OK;
    }

    // ---- host: the coefficients and the inputs of the combination, the points in the MSMs' order (commitments by column: [k][i])
    std::vector<Fr> r(n, Fr::zero()), fold(nc > 1 ? n : 0);
    std::vector<G1Aff> krs(n), pok(nc ? n : 0), cm((size_t)n * nc), P(n + np);
    for (size_t i = 0; i < n; i++) {
        combine_coefficient(seed, n, i, r[i].l);
        if (nc > 1) std::memcpy(&fold[i], in[i].fold_challenge, sizeof(Fr));
        std::memcpy(&P[i], &in[i].proof.ar, sizeof(G1Aff));
        std::memcpy(&krs[i], &in[i].proof.krs, sizeof(G1Aff));
        if (nc) std::memcpy(&pok[i], in[i].pok, sizeof(G1Aff));
        for (u32 k = 0; k < nc; k++) std::memcpy(&cm[(size_t)k * n + i], &in[i].commitments[k], sizeof(G1Aff));
    }
    auto up = [&](size_t off, const void *src, size_t bytes) -> int32_t {
        if (bytes) MI_CHECK_HIP(ctx, hipMemcpyAsync(ws + off, src, bytes, hipMemcpyHostToDevice, ctx->stream));
        return MI_OK;
    };
    MI_TRY(mi_verify_put_scalars(ctx, st, (Fr *)(ws + off_scal)));
    MI_TRY(up(off_r, r.data(), n * sizeof(Fr)));
    MI_TRY(up(off_fold, fold.data(), fold.size() * sizeof(Fr)));
    MI_TRY(up(off_krs, krs.data(), n * sizeof(G1Aff)));
    MI_TRY(up(off_pok, pok.data(), pok.size() * sizeof(G1Aff)));
    MI_TRY(up(off_cm, cm.data(), cm.size() * sizeof(G1Aff)));
    MI_TRY(up(off_p, P.data(), n * sizeof(G1Aff)));

    // ---- device: the scalar combination; S comes back for S K[0] and S alpha
    MI_TRY(mi_launch64(ctx, k_verify_combine_scalars, (size_t)nb * (ns + 1) * 64, (const Fr *)(ws + off_scal), ns, (const Fr *)(ws + off_r),
                       nc > 1 ? (const Fr *)(ws + off_fold) : nullptr, nc, n, nb, (Fr *)(ws + off_part), (Fr *)(ws + off_rc), (Fr *)(ws + off_rrep)));
    MI_TRY(mi_launch64(ctx, k_verify_combine_reduce, ns + 1, (const Fr *)(ws + off_part), nb, (Fr *)(ws + off_sum), ns + 1));
    VerifyCombinedSums sums{};
    MI_CHECK_HIP(ctx, hipMemcpyAsync(&sums.s, ws + off_sum + (size_t)ns * sizeof(Fr), sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));

    // ---- the MSMs: their number does not depend on n
    const G1Aff inf{Fp::zero(), Fp::zero()};
    std::vector<G1Aff> ck(nc, inf);
    sums.k = sums.c = sums.pok = inf;
    sums.ck = ck.data();
    if (ns) MI_TRY(mi_verify_msm(ctx, vk->k_dev, ws + off_sum, ns, 0, &sums.k));
    MI_TRY(mi_verify_msm(ctx, ws + off_krs, ws + off_r, n, MI_MSM_SCALARS_CANONICAL, &sums.krs));
    if (nc) {
        MI_TRY(mi_verify_msm(ctx, ws + off_cm, ws + off_rrep, n * nc, MI_MSM_SCALARS_CANONICAL, &sums.c));
        MI_TRY(mi_verify_msm(ctx, ws + off_pok, ws + off_r, n, MI_MSM_SCALARS_CANONICAL, &sums.pok));
        for (u32 k = 0; k < nc; k++) MI_TRY(mi_verify_msm(ctx, (G1Aff *)(ws + off_cm) + (size_t)k * n, (Fr *)(ws + off_rc) + (size_t)k * n, n, 0, &ck[k]));
    }

    // ---- the tail pairs, r_i Ar_i, the Miller loops, the two products, their final exponentiations, the verdict
    verify_combined_assemble(st.key, vk->alpha1, vk->beta2, sums, &P[n], &Q[n]);
    MI_TRY(up(off_p + n * sizeof(G1Aff), &P[n], np * sizeof(G1Aff)));
    MI_TRY(up(off_q + n * sizeof(G2Aff), &Q[n], np * sizeof(G2Aff)));
    MI_TRY(mi_launch64(ctx, k_g1_scale128, n, (const G1Aff *)(ws + off_p), (const u32 *)(ws + off_r), 8u, (G1Aff *)(ws + off_p), n));
    Fp12 *ml = (Fp12 *)(ws + off_ml), *res = (Fp12 *)(ws + off_res);
    MI_TRY(mi_pairing_enqueue(ctx, (const G1Aff *)(ws + off_p), (const G2Aff *)(ws + off_q), n + np, ml, false));
    MI_TRY(fp12_product_enqueue(ctx, ml, n + MI_VERIFY_GROTH_PAIRS, (Fp12 *)(ws + off_t0), (Fp12 *)(ws + off_t1), &res[0]));
    if (nc) MI_TRY(fp12_product_enqueue(ctx, ml + n + MI_VERIFY_GROTH_PAIRS, nc + 1, (Fp12 *)(ws + off_t0), (Fp12 *)(ws + off_t1), &res[1]));
    MI_TRY(mi_final_exp_enqueue(ctx, res, nc ? 2 : 1));
    MI_TRY(mi_launch64(ctx, k_verify_combined_judge, 64, (const Fp12 *)res, nc ? 1u : 0u, (uint8_t *)(ws + off_vd)));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(verdict, ws + off_vd, 1, hipMemcpyDeviceToHost, ctx->stream));
    MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MI_OK;
}

extern "C" {

int32_t mi_groth16_verify_combined(mi_ctx *ctx, const mi_vk *vk, const mi_verify_input *in, size_t n, const uint8_t *seed, uint8_t *verdict,
                                   uint64_t *first_malformed) {
    return mi_verify_combined_run(ctx, vk, in, n, seed, verdict, first_malformed, nullptr);
}

// ---------------------------------------------------------------- debug surface (include/mi355x_groth16_debug.h)
int32_t mi_debug_fp12_product_dev(mi_ctx *ctx, const mi_fp *x_dev, size_t n, mi_fp *out_dev) {
    if (!ctx || !x_dev || !out_dev || n == 0 || n > ((size_t)1 << 24) + MI_VERIFY_GROTH_PAIRS) return MI_EINVAL;
    WsCut cut;
    const size_t lvl0 = product_level(n), off_t0 = cut.take(lvl0 * sizeof(Fp12)), off_t1 = cut.take(product_level(lvl0) * sizeof(Fp12));
    MI_TRY(mi_reserve(ctx, ctx->ws[WS_VERIFY], cut.total));
    char *ws = (char *)ctx->ws[WS_VERIFY].p;
    return fp12_product_enqueue(ctx, (const Fp12 *)x_dev, n, (Fp12 *)(ws + off_t0), (Fp12 *)(ws + off_t1), (Fp12 *)out_dev);
}
int32_t mi_debug_g1_scale128_dev(mi_ctx *ctx, const mi_g1_affine *p_dev, const uint64_t *k_dev, size_t n, mi_g1_affine *out_dev) {
    if (!ctx || ((!p_dev || !k_dev || !out_dev) && n) || n > ((size_t)1 << 24)) return MI_EINVAL;
    return mi_launch64(ctx, k_g1_scale128, n, (const G1Aff *)p_dev, (const u32 *)k_dev, 4u, (G1Aff *)out_dev, n);
}
}

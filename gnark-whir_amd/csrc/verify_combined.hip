// One verdict for a batch of proofs under one key (include/mi355x_groth16_verify_combined.h): the random linear combination of the
// per-proof equations.  The equations, the order of the pairs and the host half are in pairing_ops.cuh, the coefficients in
// combine_coeff.cuh; the host build of the tests (tests/emu/emu_verify_combined.cpp) runs the same text.
//
// One batch, every launch on ctx->stream:
//   host      mi_verify_open (verify.hip): the argument checks, then the VerifyStage of pairing_ops.cuh -- the range and curve checks of
//             every proof (verify_well_formed) and the scalar matrix
//   k_verify_g2_check (verify.hip)   Bs of every proof that passed them -> with the host's flags, the lowest malformed index
//             (mi_verify_flag_bs).  If there is one the batch ends here with verdict 3: nothing below runs.
//   host      the coefficients r_i (one SHA-256 each) and the inputs of the combination, up (mi_verify_put_coeffs)
//   k_verify_locate_colsums / _reduce (verify_locate.hip)   the batch as the root of that file's tree: sum_i r_i s_ij for every column j
//             of the scalar matrix, S = sum_i r_i, and r_i c_i^k for the Pedersen equation: blocks over the proofs, one partial per
//             (block, column), then one sum per column
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
// through mi_verify_msm (verify_internal.h).  The front of this body is the locating body's too and is defined here, once.
#include "verify_internal.h"
#include "combine_coeff.cuh"
#include <cstring>
#include <string>
#include <vector>

namespace {

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

// ---------------------------------------------------------------- the front of the two coefficient bodies (verify_internal.h)
int32_t mi_verify_refuse_msm_pairs(mi_ctx *ctx, const mi_vk *vk, bool args_ok, size_t n, const char *msg) {
    if (ctx && vk && args_ok && n <= ((size_t)1 << 24) && (uint64_t)n * vk->n_commitments > MI_MSM_MAX_PAIRS) MI_FAIL(ctx, MI_EINVAL, msg);
    return MI_OK;
}
int32_t mi_verify_seed(mi_ctx *ctx, const char *who, const uint8_t *&seed, uint8_t own[32]) {
    if (seed) return MI_OK;
    MI_TRY(mi_os_random(ctx, std::string(who) + "the operating system gave no randomness for the seed (getrandom)", own, 32));
    seed = own;
    return MI_OK;
}
int32_t mi_verify_flag_bs(mi_ctx *ctx, VerifyStage &st, G2Aff *Q, G2Aff *q_dev, uint8_t *flags_dev) {
    const size_t n = st.n();
    for (size_t i = 0; i < n; i++) Q[i] = st.flags[i] ? G2Aff{Fp2::zero(), Fp2::zero()} : *st.proofs[i].bs;
    MI_TRY(mi_verify_upload(ctx, q_dev, Q, n * sizeof(G2Aff)));
    MI_TRY(mi_verify_upload(ctx, flags_dev, st.flags.data(), n));
    MI_TRY(mi_verify_g2_check_enqueue(ctx, q_dev, 1, flags_dev, n));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(st.flags.data(), flags_dev, n, hipMemcpyDeviceToHost, ctx->stream));
    MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    st.merge(st.flags.data());
    return MI_OK;
}
int32_t mi_verify_put_coeffs(mi_ctx *ctx, const VerifyStage &st, const mi_verify_input *in, const uint8_t *seed, bool cm_by_column, VerifyCoeffs *h,
                             char *ws, const VerifyCoeffsAt &at) {
    const size_t n = st.n();
    const u32 nc = st.nc;
    const G1Aff inf{Fp::zero(), Fp::zero()};
    h->r.assign(n, Fr::zero()), h->fold.assign(nc > 1 ? n : 0, Fr::zero());
    h->p.assign(n, inf), h->krs.assign(n, inf), h->pok.assign(nc ? n : 0, inf), h->cm.assign(n * nc, inf);
    for (size_t i = 0; i < n; i++) {
        if (st.flags[i]) continue;
        combine_coefficient(seed, n, i, h->r[i].l);
        if (nc > 1) std::memcpy(&h->fold[i], in[i].fold_challenge, sizeof(Fr));
        std::memcpy(&h->p[i], &in[i].proof.ar, sizeof(G1Aff));
        std::memcpy(&h->krs[i], &in[i].proof.krs, sizeof(G1Aff));
        if (nc) std::memcpy(&h->pok[i], in[i].pok, sizeof(G1Aff));
        for (u32 k = 0; k < nc; k++) std::memcpy(&h->cm[cm_by_column ? k * n + i : i * nc + k], &in[i].commitments[k], sizeof(G1Aff));
    }
    MI_TRY(mi_verify_put_scalars(ctx, st, (Fr *)(ws + at.scal)));
    MI_TRY(mi_verify_upload(ctx, ws + at.r, h->r.data(), n * sizeof(Fr)));
    MI_TRY(mi_verify_upload(ctx, ws + at.fold, h->fold.data(), h->fold.size() * sizeof(Fr)));
    MI_TRY(mi_verify_upload(ctx, ws + at.krs, h->krs.data(), n * sizeof(G1Aff)));
    MI_TRY(mi_verify_upload(ctx, ws + at.pok, h->pok.data(), h->pok.size() * sizeof(G1Aff)));
    MI_TRY(mi_verify_upload(ctx, ws + at.cm, h->cm.data(), h->cm.size() * sizeof(G1Aff)));
    return mi_verify_upload(ctx, ws + at.p, h->p.data(), n * sizeof(G1Aff));
}

int32_t mi_verify_combined_run(mi_ctx *ctx, const mi_vk *vk, const mi_verify_input *in, size_t n, const uint8_t *seed, uint8_t *verdict,
                               uint64_t *first_malformed, const uint8_t *decode_malformed, const Fr *pub_dev) {
    MI_TRY(mi_verify_refuse_msm_pairs(ctx, vk, in && verdict, n,
                                      "verify combined: n * n_commitments above MI_MSM_MAX_PAIRS (one MSM runs over every commitment of the batch)"));
    VerifyStage st;   // host: the range and curve checks of every proof, the scalar matrix
    MI_TRY(mi_verify_open(ctx, "verify combined: ", vk, in, n, verdict != nullptr, decode_malformed, &st, pub_dev));
    const u32 nc = st.nc, ns = st.ns, np = verify_combined_tail_pairs(nc);
    uint8_t own_seed[32];
    if (n) MI_TRY(mi_verify_seed(ctx, "verify combined: ", seed, own_seed));
    if (first_malformed) *first_malformed = n;
    if (!n) { *verdict = MI_VERIFY_OK; return MI_OK; }

    // ---- workspace.  The batch is the root of the locating verifier's tree: its column sums are that node's
    const u32 root = LocateTree(n).L, nb = mi_verify_node_blocks(root, n);
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
    std::vector<G2Aff> Q(n);
    MI_TRY(mi_verify_flag_bs(ctx, st, Q.data(), (G2Aff *)(ws + off_q), (uint8_t *)(ws + off_fl)));
    if (st.first_flagged < n) {
        *verdict = MI_VERIFY_MALFORMED;
        if (first_malformed) *first_malformed = st.first_flagged;
        return MI_OK;
    }

    // ---- host: the coefficients and the inputs of the combination, the points in the MSMs' order (commitments by column: [k][i])
    VerifyCoeffs h;
    MI_TRY(mi_verify_put_coeffs(ctx, st, in, seed, true, &h, ws, VerifyCoeffsAt{off_scal, off_r, off_fold, off_krs, off_pok, off_cm, off_p}));

    // ---- device: the scalar combination (the root's column sums, with r_i c_i^k written beside S); S comes back for S K[0] and S alpha
    MI_TRY(mi_verify_colsums_enqueue(ctx, (const Fr *)(ws + off_scal), ns, (const Fr *)(ws + off_r), n, root, nullptr, 1, (Fr *)(ws + off_part), (Fr *)(ws + off_sum),
                                     nc > 1 ? (const Fr *)(ws + off_fold) : nullptr, nc, (Fr *)(ws + off_rc), (Fr *)(ws + off_rrep)));
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
    std::vector<G1Aff> tp(np);
    std::vector<G2Aff> tq(np);
    verify_combined_assemble(st.key, vk->alpha1, vk->beta2, sums, tp.data(), tq.data());
    MI_TRY(mi_verify_upload(ctx, ws + off_p + n * sizeof(G1Aff), tp.data(), np * sizeof(G1Aff)));
    MI_TRY(mi_verify_upload(ctx, ws + off_q + n * sizeof(G2Aff), tq.data(), np * sizeof(G2Aff)));
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

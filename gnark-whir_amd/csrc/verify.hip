// groth16.Verify on the device (include/mi355x_groth16_verify.h; mt.go:497 of the reference): the BN254 pairing check behind a
// device-resident verifying key, and the two debug entry points over the same arithmetic (fp12.cuh, pairing.cuh, pairing_ops.cuh).
//
// One batch, every launch on ctx->stream:
//   host      mi_verify_open, the start of every body: the argument checks, then the VerifyStage (the range checks of every word and the
//             curve checks of the G1 points, verify_well_formed: a proof that fails them is malformed and goes no further; the scalars
//             of kSum); then mi_verify_stage_pairs, the stage this body shares with the wave body.  With a window table on the key
//             (ksum.hip) the host gathers the proofs' points with copies and uploads them once, the sums of every row over K[1..]
//             take three launches whatever the batch's size, and k_verify_assemble, one lane per proof, forms kSum = K[0] + that +
//             sum C_k, the folded commitments c^k C_k and the layout of the pairs (verify_assemble).  Without one (the knob
//             "verify_ksum" at 0, or a key whose table does not fit) the older loop: per proof one G1 MSM over the resident K[1..]
//             (mi_verify_msm over msm.hip) and verify_assemble on the host, then the pairs up.  Stage and functions live in
//             pairing_ops.cuh, where the host build of the tests runs them too
//   k_verify_assemble   one lane per proof: its pairs into the stage's regions
//   k_verify_g2_check   one lane per proof: Bs on the twist and in its r-torsion -> the malformed flag
//   k_pairing_miller    one lane per (proof, pair): a Miller loop, 384 B out
//   k_verify_judge      one lane per proof: the products of its Miller values, the final exponentiations, the comparisons -> a verdict byte
// Everything of a batch lives in ONE grow-only workspace (WS_VERIFY), laid out by a WsCut: nothing is allocated in steady state.
// mi_verify_run is that batch; verify_bytes.hip calls it too, with the proofs it decoded, and verify_locate.hip with its suspects.  The
// other three bodies (verify_internal.h names all four) reuse k_verify_g2_check, k_pairing_miller and k_pairing_final_exp through the
// three *_enqueue functions.  Every launch of one lane per item goes through mi_launch64 (verify_internal.h, which holds mi_vk too).
#include "verify_internal.h"
#include <cstring>
#include <string>
#include <vector>

namespace {

// Fp12 values live in scratch memory here by design (fp12.cuh): one wave per SIMD is all these kernels ask for
__global__ void __launch_bounds__(64, 1) k_pairing_miller(const G1Aff *p, const G2Aff *q, Fp12 *out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const G1Aff pp = p[i];
    const G2Aff qq = q[i];
    Fp12 f;
    pairing_miller_loop(&f, &pp, &qq);
    out[i] = f;
}
__global__ void __launch_bounds__(64, 1) k_pairing_final_exp(Fp12 *io, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fp12 f = io[i];
    pairing_final_exp(&f, &f);
    io[i] = f;
}
__global__ void __launch_bounds__(64, 1) k_fp12_op(int op, Fp12 *z, const Fp12 *x, const Fp12 *y, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Fp12 xx = x[i], yy = y ? y[i] : x[i];
    Fp12 r = Fp12{Fp6::zero(), Fp6::zero()};
    (void)fp12_op(op, &r, &xx, &yy);
    z[i] = r;
}
// flags[i] |= Bs of proof i (the Q of its first pair) is not a point of the r-torsion of the twist
__global__ void __launch_bounds__(64, 1) k_verify_g2_check(const G2Aff *q, u32 pairs_per_proof, uint8_t *flags, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const G2Aff bs = q[i * pairs_per_proof];
    if (!g2_in_subgroup(&bs)) flags[i] = 1;
}
__global__ void __launch_bounds__(64, 1) k_verify_judge(const Fp12 *ml, u32 pairs_per_proof, const Fp12 *e_alpha_beta, const uint8_t *flags,
                                                        uint8_t *verdicts, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Fp12 eab = *e_alpha_beta;
    verdicts[i] = verify_judge(ml + i * pairs_per_proof, pairs_per_proof - MI_VERIFY_GROTH_PAIRS, &eab, flags[i] != 0);
}

// one lane per proof: its pairs from the gathered arrays of the stage and its row's sum (verify_assemble, the text the host ran before)
__global__ void __launch_bounds__(64, 1) k_verify_assemble(const VerifyAssembleArrays a, G1Aff *p, G2Aff *q, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    verify_assemble_lane(a, i, p, q);
}

static_assert(sizeof(mi_pedersen_vk) == 2 * sizeof(G2Aff) && sizeof(mi_g1_affine) == sizeof(G1Aff) && sizeof(mi_fr) == sizeof(Fr),
              "pairing_ops.cuh reads the header's records as G1Aff / G2Aff / Fr");

}   // namespace

int32_t mi_final_exp_enqueue(mi_ctx *ctx, Fp12 *io_dev, size_t n) { return mi_launch64(ctx, k_pairing_final_exp, n, io_dev, n); }
// Miller values of n pairs already on the device, then (final) f^d' in place
int32_t mi_pairing_enqueue(mi_ctx *ctx, const G1Aff *p_dev, const G2Aff *q_dev, size_t n, Fp12 *gt_dev, bool final_exp) {
    MI_TRY(mi_launch64(ctx, k_pairing_miller, n, p_dev, q_dev, gt_dev, n));
    return final_exp ? mi_final_exp_enqueue(ctx, gt_dev, n) : MI_OK;
}
int32_t mi_verify_g2_check_enqueue(mi_ctx *ctx, const G2Aff *q_dev, u32 stride, uint8_t *flags_dev, size_t n) {
    return mi_launch64(ctx, k_verify_g2_check, n, q_dev, stride, flags_dev, n);
}
int32_t mi_verify_msm(mi_ctx *ctx, const void *bases_dev, const void *scalars_dev, size_t count, uint32_t msm_flags, G1Aff *out) {
    mi_g1_jac j;   // the MSM's result is normalised: Z = 1, or Z = 0 for infinity
    MI_TRY(mi_msm_g1_dev(ctx, (const mi_g1_affine *)bases_dev, (const mi_fr *)scalars_dev, count, msm_flags, &j));
    Fp z;
    std::memcpy(&z, &j.z, sizeof(z));
    *out = G1Aff{Fp::zero(), Fp::zero()};
    if (!z.is_zero()) std::memcpy(out, &j, sizeof(*out));
    return MI_OK;
}

int32_t mi_verify_open(mi_ctx *ctx, const char *who, const mi_vk *vk, const mi_verify_input *in, size_t n, bool has_verdict,
                       const uint8_t *decode_malformed, VerifyStage *st, const Fr *pub_dev) {
    if (!ctx) return MI_EINVAL;
    const std::string w = who;
    if (!vk || (!in && n) || !has_verdict) MI_FAIL(ctx, MI_EINVAL, w + "null vk, input or verdict pointer");
    if (n > ((size_t)1 << 24)) MI_FAIL(ctx, MI_EINVAL, w + "more than 2^24 proofs in one batch");
    const u32 nc = vk->n_commitments, n_pub = vk->nb_public - 1;
    std::vector<VerifyProofRef> refs(n);
    for (size_t i = 0; i < n; i++) {
        if (n_pub && !pub_dev && !in[i].public_inputs) MI_FAIL(ctx, MI_EINVAL, w + "public_inputs is null");
        if (nc && (!in[i].commitments || !in[i].pok || !in[i].commitment_values)) MI_FAIL(ctx, MI_EINVAL, w + "commitments, pok or commitment_values is null");
        if (nc > 1 && !in[i].fold_challenge) MI_FAIL(ctx, MI_EINVAL, w + "fold_challenge is null with more than one commitment");
        refs[i] = VerifyProofRef{(const G1Aff *)&in[i].proof.ar, (const G2Aff *)&in[i].proof.bs, (const G1Aff *)&in[i].proof.krs,
                                 (const G1Aff *)in[i].commitments, (const G1Aff *)in[i].pok, (const Fr *)in[i].public_inputs,
                                 (const Fr *)in[i].commitment_values, (const Fr *)in[i].fold_challenge};
    }
    *st = VerifyStage(VerifyKeyRef{&vk->k[0], &vk->gamma2, &vk->delta2, (const G2Aff *)vk->ped.data(), n_pub, nc}, std::move(refs), decode_malformed, n_pub ? pub_dev : nullptr);
    return MI_OK;
}

int32_t mi_verify_stage_pairs(mi_ctx *ctx, const mi_vk *vk, const VerifyStage &st, size_t extra_bytes, VerifyPairs *out) {
    const size_t n = st.n();
    const u32 ns = st.ns, np = verify_pairs_per_proof(st.nc);
    WsCut cut;
    const size_t off_scal = cut.take(n * ns * sizeof(Fr)), off_p = cut.take(n * np * sizeof(G1Aff)), off_q = cut.take(n * np * sizeof(G2Aff));
    const size_t off_ml = cut.take(n * np * sizeof(Fp12)), off_fl = cut.take(n), off_vd = cut.take(n), off_extra = cut.take(extra_bytes);
    bool table = false;   // the key's window table carries the stage (ksum.hip); built here when no call has asked for one yet
    if (ctx->verify_ksum && n >= ctx->verify_ksum_min_batch) MI_TRY(mi_ksum_ready(ctx, vk, &table));
    if (!table) {
        MI_TRY(mi_reserve(ctx, ctx->ws[WS_VERIFY], cut.total));
        char *ws = (char *)ctx->ws[WS_VERIFY].p;
        // ---- kSum: the scalar part through the G1 MSM over the resident K[1..], the rest on the host
        out->host.resize(n * np * (sizeof(G1Aff) + sizeof(G2Aff)));
        G1Aff *P = (G1Aff *)out->host.data();
        G2Aff *Q = (G2Aff *)(out->host.data() + n * np * sizeof(G1Aff));
        MI_TRY(mi_verify_put_scalars(ctx, st, (Fr *)(ws + off_scal)));
        for (size_t i = 0; i < n; i++) {
            G1Aff msm{Fp::zero(), Fp::zero()};   // no MSM runs for a malformed proof
            if (ns && !st.flags[i]) MI_TRY(mi_verify_msm(ctx, vk->k_dev, (const Fr *)(ws + off_scal) + i * ns, ns, 0, &msm));
            verify_assemble(st.key, st.proofs[i], !st.flags[i], msm, &P[i * np], &Q[i * np]);
        }
        MI_CHECK_HIP(ctx, hipMemcpyAsync(ws + off_p, P, n * np * sizeof(G1Aff), hipMemcpyHostToDevice, ctx->stream));
        MI_CHECK_HIP(ctx, hipMemcpyAsync(ws + off_q, Q, n * np * sizeof(G2Aff), hipMemcpyHostToDevice, ctx->stream));
        MI_CHECK_HIP(ctx, hipMemcpyAsync(ws + off_fl, st.flags.data(), n, hipMemcpyHostToDevice, ctx->stream));
    } else {
        // ---- the host gathers (copies only), one upload; the sums of every row and the pairs of every proof on the device
        const u32 nc = st.nc;
        WsCut in;   // the gathered block, laid out as it lies on the device
        const size_t in_k0 = in.take(sizeof(G1Aff)), in_gamma = in.take(sizeof(G2Aff)), in_delta = in.take(sizeof(G2Aff)), in_ped = in.take(2 * (size_t)nc * sizeof(G2Aff));
        const size_t in_ar = in.take(n * sizeof(G1Aff)), in_bs = in.take(n * sizeof(G2Aff)), in_krs = in.take(n * sizeof(G1Aff));
        const size_t in_cm = in.take(n * nc * sizeof(G1Aff)), in_pok = in.take(n * sizeof(G1Aff)), in_fold = in.take(n * sizeof(Fr));
        const size_t off_in = cut.take(in.total), off_msm = cut.take(n * sizeof(G1Aff)), off_ksum = cut.take(mi_ksum_scratch_bytes(vk, n));
        MI_TRY(mi_reserve(ctx, ctx->ws[WS_VERIFY], cut.total));
        char *ws = (char *)ctx->ws[WS_VERIFY].p;
        out->host.assign(in.total, 0);   // a flagged proof's records stay zero: none of its words is read, here or there
        char *h = out->host.data();
        std::memcpy(h + in_k0, st.key.k0, sizeof(G1Aff));
        std::memcpy(h + in_gamma, st.key.gamma2, sizeof(G2Aff));
        std::memcpy(h + in_delta, st.key.delta2, sizeof(G2Aff));
        if (nc) std::memcpy(h + in_ped, st.key.ped, 2 * (size_t)nc * sizeof(G2Aff));
        for (size_t i = 0; i < n; i++) {
            if (st.flags[i]) continue;
            const VerifyProofRef &pr = st.proofs[i];
            std::memcpy(h + in_ar + i * sizeof(G1Aff), pr.ar, sizeof(G1Aff));
            std::memcpy(h + in_bs + i * sizeof(G2Aff), pr.bs, sizeof(G2Aff));
            std::memcpy(h + in_krs + i * sizeof(G1Aff), pr.krs, sizeof(G1Aff));
            if (nc) std::memcpy(h + in_cm + i * nc * sizeof(G1Aff), pr.commitments, nc * sizeof(G1Aff));
            if (nc) std::memcpy(h + in_pok + i * sizeof(G1Aff), pr.pok, sizeof(G1Aff));
            if (nc > 1) std::memcpy(h + in_fold + i * sizeof(Fr), pr.fold_challenge, sizeof(Fr));
        }
        MI_TRY(mi_verify_put_scalars(ctx, st, (Fr *)(ws + off_scal)));
        MI_CHECK_HIP(ctx, hipMemcpyAsync(ws + off_fl, st.flags.data(), n, hipMemcpyHostToDevice, ctx->stream));
        MI_CHECK_HIP(ctx, hipMemcpyAsync(ws + off_in, h, in.total, hipMemcpyHostToDevice, ctx->stream));
        uint64_t launches = 0;
        MI_TRY(mi_ksum_enqueue(ctx, vk, (const Fr *)(ws + off_scal), (const uint8_t *)(ws + off_fl), n, (G1Aff *)(ws + off_msm), ws + off_ksum, &launches));
        const char *d = ws + off_in;
        const VerifyAssembleArrays arrays{VerifyKeyRef{(const G1Aff *)(d + in_k0), (const G2Aff *)(d + in_gamma), (const G2Aff *)(d + in_delta),
                                                       (const G2Aff *)(d + in_ped), st.n_pub, nc},
                                          (const G1Aff *)(d + in_ar), (const G2Aff *)(d + in_bs), (const G1Aff *)(d + in_krs), (const G1Aff *)(d + in_cm),
                                          (const G1Aff *)(d + in_pok), (const Fr *)(d + in_fold), (const uint8_t *)(ws + off_fl), (const G1Aff *)(ws + off_msm)};
        MI_TRY(mi_launch64(ctx, k_verify_assemble, n, arrays, (G1Aff *)(ws + off_p), (G2Aff *)(ws + off_q), n));
        ctx->verify_ksum_batches++;
        ctx->verify_ksum_launches += launches + 1;
    }
    char *ws = (char *)ctx->ws[WS_VERIFY].p;
    out->np = np;
    out->p = (G1Aff *)(ws + off_p); out->q = (G2Aff *)(ws + off_q); out->ml = (Fp12 *)(ws + off_ml);
    out->flags = (uint8_t *)(ws + off_fl); out->verdicts = (uint8_t *)(ws + off_vd); out->extra = extra_bytes ? (uint8_t *)(ws + off_extra) : nullptr;
    return MI_OK;
}

int32_t mi_verify_run(mi_ctx *ctx, const mi_vk *vk, const mi_verify_input *in, size_t n, uint8_t *verdicts, const uint8_t *decode_malformed,
                      const Fr *pub_dev) {
    VerifyStage st;   // host: flags (range and curve checks), scalars
    MI_TRY(mi_verify_open(ctx, "verify: ", vk, in, n, verdicts || !n, decode_malformed, &st, pub_dev));
    if (!n) return MI_OK;
    VerifyPairs d;
    MI_TRY(mi_verify_stage_pairs(ctx, vk, st, 0, &d));
    // ---- device: Bs check (its answer joins the flags there, for the judgement), Miller loops, judgement
    MI_TRY(mi_verify_g2_check_enqueue(ctx, d.q, d.np, d.flags, n));
    MI_TRY(mi_pairing_enqueue(ctx, d.p, d.q, n * d.np, d.ml, false));
    MI_TRY(mi_launch64(ctx, k_verify_judge, n, (const Fp12 *)d.ml, d.np, (const Fp12 *)vk->e_alpha_beta_dev, (const uint8_t *)d.flags, d.verdicts, n));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(verdicts, d.verdicts, n, hipMemcpyDeviceToHost, ctx->stream));
    MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MI_OK;
}

extern "C" {

int32_t mi_vk_load(mi_ctx *ctx, const mi_vk_desc *d, mi_vk **out) {
    if (!ctx) return MI_EINVAL;
    if (!d || !out) MI_FAIL(ctx, MI_EINVAL, "vk load: null descriptor or output pointer");
    *out = nullptr;
    if (!d->k) MI_FAIL(ctx, MI_EINVAL, "vk load: k is null");
    if (d->nb_public == 0) MI_FAIL(ctx, MI_EINVAL, "vk load: nb_public is 0 (it counts the ONE wire)");
    if (d->n_commitments > MI_PK_RAW_MAX_COMMITMENTS) MI_FAIL(ctx, MI_EINVAL, "vk load: n_commitments above MI_PK_RAW_MAX_COMMITMENTS");
    if (d->n_k != (uint64_t)d->nb_public + d->n_commitments) MI_FAIL(ctx, MI_EINVAL, "vk load: n_k is not nb_public + n_commitments");
    if (d->n_commitments && !d->ped) MI_FAIL(ctx, MI_EINVAL, "vk load: ped is null");
    const G1Aff alpha = g1_of(d->alpha1);
    const G2Aff beta = g2_of(d->beta2), gamma = g2_of(d->gamma2), delta = g2_of(d->delta2);
    // every coordinate below p, before any arithmetic sees it: one encoding per element (pairing.cuh, fe_is_reduced)
    const std::string not_reduced = " has a coordinate that is not below p";
    if (!g1_reduced(alpha)) MI_FAIL(ctx, MI_EINVAL, "vk load: alpha1" + not_reduced);
    if (!g2_reduced(beta)) MI_FAIL(ctx, MI_EINVAL, "vk load: beta2" + not_reduced);
    if (!g2_reduced(gamma)) MI_FAIL(ctx, MI_EINVAL, "vk load: gamma2" + not_reduced);
    if (!g2_reduced(delta)) MI_FAIL(ctx, MI_EINVAL, "vk load: delta2" + not_reduced);
    for (uint64_t i = 0; i < d->n_k; i++)
        if (!g1_reduced(g1_of(d->k[i]))) MI_FAIL(ctx, MI_EINVAL, "vk load: k[" + std::to_string(i) + "]" + not_reduced);
    for (uint32_t k = 0; k < d->n_commitments; k++) {
        if (!g2_reduced(g2_of(d->ped[k].g))) MI_FAIL(ctx, MI_EINVAL, "vk load: ped[" + std::to_string(k) + "].g" + not_reduced);
        if (!g2_reduced(g2_of(d->ped[k].g_sigma_neg))) MI_FAIL(ctx, MI_EINVAL, "vk load: ped[" + std::to_string(k) + "].g_sigma_neg" + not_reduced);
    }
    if (!g1_on_curve(alpha)) MI_FAIL(ctx, MI_EINVAL, "vk load: alpha1 is not on the curve");
    if (!g2_in_subgroup(&beta)) MI_FAIL(ctx, MI_EINVAL, "vk load: beta2 is not in the r-torsion of the twist");
    if (gamma.is_inf() || !g2_in_subgroup(&gamma)) MI_FAIL(ctx, MI_EINVAL, "vk load: gamma2 is infinity or not in the r-torsion of the twist");
    if (delta.is_inf() || !g2_in_subgroup(&delta)) MI_FAIL(ctx, MI_EINVAL, "vk load: delta2 is infinity or not in the r-torsion of the twist");
    for (uint64_t i = 0; i < d->n_k; i++)
        if (!g1_on_curve(g1_of(d->k[i]))) MI_FAIL(ctx, MI_EINVAL, "vk load: k[" + std::to_string(i) + "] is not on the curve");
    for (uint32_t k = 0; k < d->n_commitments; k++) {
        const G2Aff g = g2_of(d->ped[k].g), gs = g2_of(d->ped[k].g_sigma_neg);
        if (std::memcmp(&d->ped[k].g, &d->ped[0].g, sizeof(mi_g2_affine)) != 0) MI_FAIL(ctx, MI_EINVAL, "vk load: the Pedersen keys do not share one G");
        if (g.is_inf() || !g2_in_subgroup(&g) || !g2_in_subgroup(&gs))
            MI_FAIL(ctx, MI_EINVAL, "vk load: ped[" + std::to_string(k) + "] is not in the r-torsion of the twist");
    }
    return mi_vk_build(ctx, d, nullptr, out);
}

}   // extern "C"

int32_t mi_vk_build(mi_ctx *ctx, const mi_vk_desc *d, G1Aff *k_dev_adopt, mi_vk **out) {
    const G1Aff alpha = g1_of(d->alpha1);
    const G2Aff beta = g2_of(d->beta2), gamma = g2_of(d->gamma2), delta = g2_of(d->delta2);
    mi_vk *vk = new (std::nothrow) mi_vk;
    if (!vk) {
        if (k_dev_adopt) (void)hipFree(k_dev_adopt);
        MI_FAIL(ctx, MI_ENOMEM, "vk load: out of host memory");
    }
    vk->k_dev = k_dev_adopt;
    vk->alpha1 = alpha; vk->beta2 = beta; vk->gamma2 = gamma; vk->delta2 = delta;
    vk->nb_public = d->nb_public; vk->n_commitments = d->n_commitments;
    vk->pc_off.assign((size_t)d->n_commitments + 1, 0);
    vk->k.resize(d->n_k);
    std::memcpy(vk->k.data(), d->k, d->n_k * sizeof(G1Aff));
    if (d->n_commitments) vk->ped.assign(d->ped, d->ped + d->n_commitments);
    auto body = [&]() -> int32_t {
        const size_t nb = (d->n_k - 1) * sizeof(G1Aff);
        if (!k_dev_adopt) MI_CHECK_HIP(ctx, hipMalloc((void **)&vk->k_dev, nb + 64));
        MI_CHECK_HIP(ctx, hipMalloc((void **)&vk->e_alpha_beta_dev, sizeof(Fp12)));
        if (nb && !k_dev_adopt) MI_CHECK_HIP(ctx, hipMemcpyAsync(vk->k_dev, vk->k.data() + 1, nb, hipMemcpyHostToDevice, ctx->stream));
        WsCut cut;
        const size_t off_alpha = cut.take(sizeof(alpha)), off_beta = cut.take(sizeof(beta));
        MI_TRY(mi_reserve(ctx, ctx->ws[WS_VERIFY], cut.total));
        char *ws = (char *)ctx->ws[WS_VERIFY].p;
        MI_CHECK_HIP(ctx, hipMemcpyAsync(ws + off_alpha, &alpha, sizeof(alpha), hipMemcpyHostToDevice, ctx->stream));
        MI_CHECK_HIP(ctx, hipMemcpyAsync(ws + off_beta, &beta, sizeof(beta), hipMemcpyHostToDevice, ctx->stream));
        MI_TRY(mi_pairing_enqueue(ctx, (const G1Aff *)(ws + off_alpha), (const G2Aff *)(ws + off_beta), 1, vk->e_alpha_beta_dev, true));
        MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return MI_OK;
    };
    const int32_t rc = body();
    if (rc != MI_OK) {
        if (vk->k_dev) (void)hipFree(vk->k_dev);
        if (vk->e_alpha_beta_dev) (void)hipFree(vk->e_alpha_beta_dev);
        delete vk;
        return rc;
    }
    *out = vk;
    return MI_OK;
}

extern "C" {

int32_t mi_vk_free(mi_ctx *ctx, mi_vk *vk) {
    if (!ctx) return MI_EINVAL;
    if (!vk) return MI_OK;
    hipError_t e1 = vk->k_dev ? hipFree(vk->k_dev) : hipSuccess, e2 = vk->e_alpha_beta_dev ? hipFree(vk->e_alpha_beta_dev) : hipSuccess;
    hipError_t e3 = vk->ksum.table ? hipFree(vk->ksum.table) : hipSuccess;   // the window table of K[1..] (ksum.hip)
    delete vk;
    MI_CHECK_HIP(ctx, e1);
    MI_CHECK_HIP(ctx, e2);
    MI_CHECK_HIP(ctx, e3);
    return MI_OK;
}

int32_t mi_pedersen_vk_make(mi_ctx *ctx, const mi_fr *sigma, uint32_t n, mi_pedersen_vk *out) {
    if (!ctx) return MI_EINVAL;
    if ((!sigma || !out) && n) MI_FAIL(ctx, MI_EINVAL, "pedersen vk: null sigma or output pointer");
    if (!n) return MI_OK;
    const G2Aff gen = g2_generator();
    mi_g2_affine g;
    std::memcpy(&g, &gen, sizeof(g));
    std::vector<mi_fr> neg(n);
    std::vector<mi_g2_affine> pts(n);
    for (uint32_t k = 0; k < n; k++) {
        Fr s;
        std::memcpy(&s, &sigma[k], sizeof(s));
        s = fe_neg(s);
        std::memcpy(&neg[k], &s, sizeof(s));
    }
    MI_TRY(mi_batch_scalar_mul_g2(ctx, &g, neg.data(), n, pts.data()));
    for (uint32_t k = 0; k < n; k++) { out[k].g = g; out[k].g_sigma_neg = pts[k]; }
    return MI_OK;
}

int32_t mi_groth16_verify(mi_ctx *ctx, const mi_vk *vk, const mi_verify_input *in, uint8_t *verdict) {
    if (ctx && (!in || !verdict)) MI_FAIL(ctx, MI_EINVAL, "verify: null input or verdict pointer");
    return mi_verify_run(ctx, vk, in, 1, verdict, nullptr);
}
int32_t mi_groth16_verify_batch(mi_ctx *ctx, const mi_vk *vk, const mi_verify_input *in, size_t n, uint8_t *verdicts) {
    return mi_verify_run(ctx, vk, in, n, verdicts, nullptr);
}

// ---------------------------------------------------------------- debug surface (include/mi355x_groth16_debug.h)
int32_t mi_debug_pairing_dev(mi_ctx *ctx, const mi_g1_affine *p_dev, const mi_g2_affine *q_dev, size_t n, mi_fp *gt_dev, uint32_t flags) {
    if (!ctx || (flags & ~MI_PAIRING_FINAL_EXP) || ((!p_dev || !q_dev || !gt_dev) && n) || n > ((size_t)1 << 24)) return MI_EINVAL;
    return mi_pairing_enqueue(ctx, (const G1Aff *)p_dev, (const G2Aff *)q_dev, n, (Fp12 *)gt_dev, (flags & MI_PAIRING_FINAL_EXP) != 0);
}
int32_t mi_debug_verify_pairs_dev(mi_ctx *ctx, const mi_vk *vk, const mi_verify_input *in, size_t n, mi_g1_affine *p_out, mi_g2_affine *q_out) {
    if (ctx && n && (!p_out || !q_out)) MI_FAIL(ctx, MI_EINVAL, "verify pairs: null output pointer");
    VerifyStage st;
    MI_TRY(mi_verify_open(ctx, "verify pairs: ", vk, in, n, true, nullptr, &st));
    if (!n) return MI_OK;
    VerifyPairs d;
    MI_TRY(mi_verify_stage_pairs(ctx, vk, st, 0, &d));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(p_out, d.p, n * d.np * sizeof(G1Aff), hipMemcpyDeviceToHost, ctx->stream));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(q_out, d.q, n * d.np * sizeof(G2Aff), hipMemcpyDeviceToHost, ctx->stream));
    MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MI_OK;
}
int32_t mi_debug_fp12_op_dev(mi_ctx *ctx, int op, mi_fp *z_dev, const mi_fp *x_dev, const mi_fp *y_dev, size_t n) {
    if (!ctx || op < 0 || op >= F12_OP_END || ((!z_dev || !x_dev) && n) || n > ((size_t)1 << 24)) return MI_EINVAL;
    return mi_launch64(ctx, k_fp12_op, n, op, (Fp12 *)z_dev, (const Fp12 *)x_dev, (const Fp12 *)y_dev, n);
}
}

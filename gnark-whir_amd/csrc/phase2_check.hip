// The checks of a ceremony (include/mi355x_groth16_phase2_check.h): the SRS rows are consistent powers, contributions carry a proof of
// knowledge, a claimed state is verified before it is taken over -- for delta (Z, K, the delta points) and for the commitment keys'
// sigma (BasisExpSigma, the points [-sigma_k]2), each with a chain of its own.  The hashes, the records and the judgement of a relation
// are ceremony_ops.cuh's text; the chains of records are verified on the host (phase2_records.hip).  The sigma calls at the end of this
// file add no kernel: they run the ones below and phase2.hip's scale kernels.
//
// Every pairing check here is a SAME-RATIO TEST  e(sum r_k P_k, s) = e(sum r_k Q_k, t):
//   k_ceremony_coeffs   one lane per k: r_k = 128 bits of SHA-256(tag | seed | k), stored as a Montgomery Fr -- ONE array per call, every
//                       relation reads a prefix of it
//   MSMs                mi_msm_g1_dev / mi_msm_g2_dev (msm.hip) over the row on the device and that array.  The two sides of a "powers"
//                       relation are two MSMs with the same scalars over row + 1 and row.  The MSM has no knob for scalars below 2^128
//                       (its plan knobs are about windows, items and levels): it is called as it is, and sorts the upper windows' zero
//                       digits away by itself
//   k_pairing_miller    (verify.hip, mi_pairing_enqueue) every pair of every relation in ONE launch; the second G1 point of a relation
//                       is negated on the host, so a relation is the product of its two Miller values
//   k_fp12_product      (verify_combined.hip, mi_fp12_product_level_enqueue) that product, a run of two values per relation
//   k_pairing_final_exp (verify.hip, mi_final_exp_enqueue) one lane per relation
//   k_ceremony_judge    one lane per relation: the result against one -> a byte
// An SRS row is uploaded, checked point by point (phase2.hip's mi_phase2_check_points: the refusals are mi_phase2_init's), summed and
// released before the next: the call holds one row, the coefficients and a few points (Arena, dev_arena.h).
#include "verify_internal.h"
#include "phase2_internal.h"
#include "ceremony_ops.cuh"
#include "point_check.cuh"
#include "stream_clock.h"
#include <cstring>
#include <string>
#include <vector>

namespace {

struct CeremonySeed { uint8_t b[32]; };

// out[k] = r_k, Montgomery
__global__ void __launch_bounds__(256) k_ceremony_coeffs(CeremonySeed seed, u64 n, Fr *out) {
    const u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    u32 w[4];
    ceremony_coefficient(seed.b, k, w);
    out[k] = fr_from_u128(w);
}
// bad[i] = relation i does not hold (res: the products after their final exponentiations)
__global__ void __launch_bounds__(64, 1) k_ceremony_judge(const Fp12 *res, u32 n_rel, uint8_t *bad) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rel) return;
    const Fp12 f = res[i];
    bad[i] = ceremony_relation_holds(&f) ? 0 : 1;
}

// seed, or 32 bytes of the operating system's into own
int32_t seed_or_random(mi_ctx *ctx, const char *who, const uint8_t *&seed, uint8_t own[32]) {
    if (seed) return MI_OK;
    MI_TRY(mi_os_random(ctx, std::string(who) + ": the operating system gave no randomness for the seed (getrandom)", own, 32));
    seed = own;
    return MI_OK;
}
int32_t coeffs_enqueue(mi_ctx *ctx, const uint8_t seed[32], u64 n, Fr *out_dev) {
    if (!n) return MI_OK;
    CeremonySeed s;
    std::memcpy(s.b, seed, 32);
    hipLaunchKernelGGL(k_ceremony_coeffs, dim3(mi_blocks_of(n, 256)), dim3(256), 0, ctx->stream, s, n, out_dev);
    MI_CHECK_HIP(ctx, hipGetLastError());
    return MI_OK;
}
// sum_k scalars[k] bases[k] over device arrays, affine, (0, 0) = infinity; Montgomery scalars.  A sum over no pair is infinity, whatever
// the pointers: nothing is launched for it
int32_t msm_g1(mi_ctx *ctx, const G1Aff *bases, const Fr *scalars, u64 n, G1Aff *out) {
    *out = G1Aff{Fp::zero(), Fp::zero()};
    return n ? mi_verify_msm(ctx, bases, scalars, (size_t)n, 0, out) : MI_OK;
}
int32_t msm_g2(mi_ctx *ctx, const G2Aff *bases, const Fr *scalars, u64 n, G2Aff *out) {
    *out = G2Aff{Fp2::zero(), Fp2::zero()};
    if (!n) return MI_OK;
    mi_g2_jac j;   // normalised as the G1 result is: Z = 1, or Z = 0 for infinity
    MI_TRY(mi_msm_g2_dev(ctx, (const mi_g2_affine *)bases, (const mi_fr *)scalars, (size_t)n, 0, &j));
    Fp2 z;
    std::memcpy(&z, &j.z, sizeof(z));
    if (!z.is_zero()) std::memcpy(out, &j, sizeof(*out));
    return MI_OK;
}

// a Schnorr nonce: the caller's (not 0, below r), or 48 bytes of the operating system's reduced mod r: uniform to within 2^-128
int32_t nonce_or_random(mi_ctx *ctx, const mi_fr *nonce, Fr &k) {
    if (nonce) {
        std::memcpy(&k, nonce, 32);
        if (k.is_zero()) MI_FAIL(ctx, MI_EINVAL, "phase2: nonce is 0");
        if (!fe_is_reduced(k)) MI_FAIL(ctx, MI_EINVAL, "phase2: nonce is not below r");
        return MI_OK;
    }
    return mi_draw_nonce(ctx, "phase2: the operating system gave no randomness for the nonce (getrandom)", "phase2: the drawn nonce is 0", k);
}

typedef CeremonyRelations Relations;   // phase2_internal.h
// bad[i] = relation i does not hold
int32_t judge(mi_ctx *ctx, Arena &ar, const Relations &rel, std::vector<uint8_t> &bad) {
    const u32 n = rel.count();
    bad.assign(n, 1);
    G1Aff *p = nullptr;
    G2Aff *q = nullptr;
    Fp12 *ml = nullptr, *res = nullptr;
    uint8_t *bad_dev = nullptr;
    MI_TRY(ar.alloc(ctx, &p, (size_t)2 * n));
    MI_TRY(ar.alloc(ctx, &q, (size_t)2 * n));
    MI_TRY(ar.alloc(ctx, &ml, (size_t)2 * n));
    MI_TRY(ar.alloc(ctx, &res, (size_t)n));
    MI_TRY(ar.alloc(ctx, &bad_dev, (size_t)n));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(p, rel.p.data(), (size_t)2 * n * sizeof(G1Aff), hipMemcpyHostToDevice, ctx->stream));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(q, rel.q.data(), (size_t)2 * n * sizeof(G2Aff), hipMemcpyHostToDevice, ctx->stream));
    MI_TRY(mi_pairing_enqueue(ctx, p, q, (size_t)2 * n, ml, false));
    for (u32 i = 0; i < n; i++) MI_TRY(mi_fp12_product_level_enqueue(ctx, ml + 2 * i, 2, res + i, 1));   // a relation's two values: a run of k_fp12_product
    MI_TRY(mi_final_exp_enqueue(ctx, res, n));
    MI_TRY(mi_launch64(ctx, k_ceremony_judge, n, (const Fp12 *)res, n, bad_dev));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(bad.data(), bad_dev, n, hipMemcpyDeviceToHost, ctx->stream));
    MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (void *x : {(void *)p, (void *)q, (void *)ml, (void *)res, (void *)bad_dev}) ar.release(x);
    return MI_OK;
}

// ---------------------------------------------------------------------------------------------------- the SRS
// srs: HOST rows, which go up and are checked point by point here, or (on_device) rows that are on the device and have passed those
// checks already -- beta_g2 then still sits in the descriptor, on the host
int32_t srs_check_run(mi_ctx *ctx, const mi_srs_desc *srs, bool on_device, u64 N, const uint8_t *seed, uint32_t flags, mi_srs_check_stats &stats, uint32_t *failed) {
    hipStream_t st = ctx->stream;
    Arena ar;
    HostClock ck;
    Fr *r = nullptr;
    MI_TRY(ar.alloc(ctx, &r, (size_t)(2 * N - 1)));
    MI_TRY(coeffs_enqueue(ctx, seed, 2 * N - 1, r));
    MI_TRY(sync_lap(ctx, ck, stats.coeff_ms));
    // one G1 row: up, checked, summed over [1, 1 + n_rel) and [0, n_rel) with the same scalars, (for tau_g1) over [0, N) too, released
    auto g1_row = [&](const char *name, const mi_g1_affine *host, u64 n, u64 n_rel, G1Aff *hi, G1Aff *lo, G1Aff *first_n) -> int32_t {
        G1Aff *row = (G1Aff *)host;
        if (!on_device) {
            MI_TRY(ar.alloc(ctx, &row, (size_t)n));
            MI_CHECK_HIP(ctx, hipMemcpyAsync(row, host, n * sizeof(G1Aff), hipMemcpyHostToDevice, st));
            MI_TRY(sync_lap(ctx, ck, stats.upload_ms));
            const Phase2Row pr{name, false, row, n};
            MI_TRY(mi_phase2_check_points(ctx, ar, &pr, 1, flags));
            ck.lap(stats.point_check_ms);
        }
        MI_TRY(msm_g1(ctx, row + 1, r, n_rel, hi));
        MI_TRY(msm_g1(ctx, row, r, n_rel, lo));
        if (first_n) MI_TRY(msm_g1(ctx, row, r, N, first_n));
        ck.lap(stats.msm_g1_ms);
        if (!on_device) ar.release(row);
        return MI_OK;
    };
    G1Aff t_hi, t_lo, t_n, a_hi, a_lo, b_hi, b_lo;
    MI_TRY(g1_row("tau_g1", srs->tau_g1, 2 * N, 2 * N - 1, &t_hi, &t_lo, &t_n));
    MI_TRY(g1_row("alpha_tau_g1", srs->alpha_tau_g1, N, N - 1, &a_hi, &a_lo, nullptr));
    MI_TRY(g1_row("beta_tau_g1", srs->beta_tau_g1, N, N - 1, &b_hi, &b_lo, nullptr));
    G2Aff t2_sum;
    if (on_device) {
        MI_TRY(msm_g2(ctx, (const G2Aff *)srs->tau_g2, r, N, &t2_sum));
        ck.lap(stats.msm_g2_ms);
    } else {
        G2Aff *row = nullptr, *b2 = nullptr;
        MI_TRY(ar.alloc(ctx, &row, (size_t)N));
        MI_TRY(ar.alloc(ctx, &b2, (size_t)1));
        MI_CHECK_HIP(ctx, hipMemcpyAsync(row, srs->tau_g2, N * sizeof(G2Aff), hipMemcpyHostToDevice, st));
        MI_CHECK_HIP(ctx, hipMemcpyAsync(b2, &srs->beta_g2, sizeof(G2Aff), hipMemcpyHostToDevice, st));
        MI_TRY(sync_lap(ctx, ck, stats.upload_ms));
        const Phase2Row pr[2] = {{"tau_g2", true, row, N}, {"beta_g2", true, b2, 1}};
        MI_TRY(mi_phase2_check_points(ctx, ar, pr, 2, flags));
        ck.lap(stats.point_check_ms);
        MI_TRY(msm_g2(ctx, row, r, N, &t2_sum));
        ck.lap(stats.msm_g2_ms);
        ar.release(row); ar.release(b2);
    }
    ar.release(r);
    // every point below has passed its checks
    mi_g1_affine first1[2];   // tau_g1[0], beta_tau_g1[0]
    mi_g2_affine first2[2];   // tau_g2[0], tau_g2[1]
    if (on_device) {
        MI_CHECK_HIP(ctx, hipMemcpyAsync(&first1[0], srs->tau_g1, sizeof(G1Aff), hipMemcpyDeviceToHost, st));
        MI_CHECK_HIP(ctx, hipMemcpyAsync(&first1[1], srs->beta_tau_g1, sizeof(G1Aff), hipMemcpyDeviceToHost, st));
        MI_CHECK_HIP(ctx, hipMemcpyAsync(first2, srs->tau_g2, 2 * sizeof(G2Aff), hipMemcpyDeviceToHost, st));
        MI_CHECK_HIP(ctx, hipStreamSynchronize(st));
    } else {
        first1[0] = srs->tau_g1[0]; first1[1] = srs->beta_tau_g1[0]; first2[0] = srs->tau_g2[0]; first2[1] = srs->tau_g2[1];
    }
    const G1Aff g1 = g1_generator(), tau1_0 = g1_of(first1[0]), beta1 = g1_of(first1[1]);
    const G2Aff g2 = g2_generator(), tau2_0 = g2_of(first2[0]), tau2 = g2_of(first2[1]), beta2 = g2_of(srs->beta_g2);
    Relations rel;
    rel.add(t_hi, g2, t_lo, tau2);     // MI_SRS_BAD_TAU_G1
    rel.add(a_hi, g2, a_lo, tau2);     // MI_SRS_BAD_ALPHA_G1
    rel.add(b_hi, g2, b_lo, tau2);     // MI_SRS_BAD_BETA_G1
    rel.add(t_n, g2, g1, t2_sum);      // MI_SRS_BAD_TAU_G2
    rel.add(beta1, g2, g1, beta2);     // MI_SRS_BAD_BETA_G2
    std::vector<uint8_t> bad;
    MI_TRY(judge(ctx, ar, rel, bad));
    ck.lap(stats.pairing_ms);
    uint32_t mask = 0;
    if (std::memcmp(&tau1_0, &g1, sizeof(g1)) != 0 || std::memcmp(&tau2_0, &g2, sizeof(g2)) != 0) mask |= MI_SRS_BAD_GENERATORS;
    const uint32_t bits[5] = {MI_SRS_BAD_TAU_G1, MI_SRS_BAD_ALPHA_G1, MI_SRS_BAD_BETA_G1, MI_SRS_BAD_TAU_G2, MI_SRS_BAD_BETA_G2};
    for (int i = 0; i < 5; i++) if (bad[i]) mask |= bits[i];
    *failed = mask;
    stats.peak_bytes = ar.peak;
    return MI_OK;
}

// ---------------------------------------------------------------------------------------------------- a claimed state
struct Claim { G1Aff *z = nullptr, *k = nullptr; };   // the claimed arrays on the device

int32_t verify_run(mi_ctx *ctx, mi_phase2 *S, const mi_phase2_claim *claim, const G1Aff &d1, const G2Aff &d2, const uint8_t *seed, Arena &ar, Claim &c,
                   bool *z_bad, bool *k_bad, bool *delta_bad) {
    hipStream_t st = ctx->stream;
    mi_srs_check_stats &stats = ctx->phase2_verify_stats;
    HostClock ck;
    const u64 N = S->N, nk = S->n_k;
    MI_TRY(ar.alloc(ctx, &c.z, (size_t)N));
    MI_TRY(ar.alloc(ctx, &c.k, (size_t)nk));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(c.z, claim->g1_z, N * sizeof(G1Aff), hipMemcpyHostToDevice, st));
    if (nk) MI_CHECK_HIP(ctx, hipMemcpyAsync(c.k, claim->g1_k, nk * sizeof(G1Aff), hipMemcpyHostToDevice, st));
    MI_TRY(sync_lap(ctx, ck, stats.upload_ms));
    {
        BadSlots bad;
        MI_TRY(bad.init(ctx, 2, &ar));
        MI_TRY(mi_points_check_enqueue(ctx, false, c.z, N, POINT_RULE_CLAIM, bad.dev));
        MI_TRY(mi_points_check_enqueue(ctx, false, c.k, nk, POINT_RULE_CLAIM, bad.dev + 1));
        MI_TRY(bad.fetch(ctx));
        ck.lap(stats.point_check_ms);
        if (bad.bad(0)) MI_FAIL(ctx, MI_EINVAL, "phase2 verify: claim.g1_z[" + std::to_string(bad.host[0]) + "] is not a point of the curve");
        if (bad.bad(1)) MI_FAIL(ctx, MI_EINVAL, "phase2 verify: claim.g1_k[" + std::to_string(bad.host[1]) + "] is not a point of the curve");
    }
    Fr *r = nullptr;
    const u64 nr = N > nk ? N : nk;
    MI_TRY(ar.alloc(ctx, &r, (size_t)nr));
    MI_TRY(coeffs_enqueue(ctx, seed, nr, r));
    MI_TRY(sync_lap(ctx, ck, stats.coeff_ms));
    G1Aff z_new, z_own, k_new, k_own;
    MI_TRY(msm_g1(ctx, c.z, r, N, &z_new));
    MI_TRY(msm_g1(ctx, (const G1Aff *)S->g1_z, r, N, &z_own));
    MI_TRY(msm_g1(ctx, c.k, r, nk, &k_new));
    MI_TRY(msm_g1(ctx, (const G1Aff *)S->g1_k, r, nk, &k_own));
    ck.lap(stats.msm_g1_ms);
    ar.release(r);
    Relations rel;
    rel.add(d1, g2_generator(), g1_generator(), d2);   // MI_PHASE2_BAD_DELTA's pairing
    rel.add(z_new, d2, z_own, S->delta2);              // MI_PHASE2_BAD_Z
    rel.add(k_new, d2, k_own, S->delta2);              // MI_PHASE2_BAD_K
    std::vector<uint8_t> bad;
    MI_TRY(judge(ctx, ar, rel, bad));
    ck.lap(stats.pairing_ms);
    *delta_bad = bad[0]; *z_bad = bad[1]; *k_bad = bad[2];
    stats.peak_bytes = ar.peak;
    return MI_OK;
}

// the claimed BasisExpSigma arrays on the device, and per commitment whether its relation fails.  No kernel here is new: the claim is
// checked by point_check.cuh's POINT_RULE_CLAIM, summed by the context's MSM and judged by judge() as Z and K are above
int32_t sigma_verify_run(mi_ctx *ctx, mi_phase2 *S, const mi_phase2_sigma_claim *claim, const uint8_t *seed, Arena &ar, std::vector<G1Aff *> &bes,
                         std::vector<uint8_t> &bad) {
    hipStream_t st = ctx->stream;
    mi_srs_check_stats &stats = ctx->phase2_verify_stats;
    HostClock ck;
    const u32 nc = S->n_commitments;
    u64 nr = 0;
    for (u32 k = 0; k < nc; k++) {
        const u64 n = S->ped[k].n;
        MI_TRY(ar.alloc(ctx, &bes[k], (size_t)n));
        if (n) MI_CHECK_HIP(ctx, hipMemcpyAsync(bes[k], claim->basis_exp_sigma[k], n * sizeof(G1Aff), hipMemcpyHostToDevice, st));
        if (n > nr) nr = n;
    }
    MI_TRY(sync_lap(ctx, ck, stats.upload_ms));
    {
        BadSlots bad;
        MI_TRY(bad.init(ctx, nc, &ar));
        for (u32 k = 0; k < nc; k++) MI_TRY(mi_points_check_enqueue(ctx, false, bes[k], S->ped[k].n, POINT_RULE_CLAIM, bad.dev + k));
        MI_TRY(bad.fetch(ctx));
        ck.lap(stats.point_check_ms);
        for (u32 k = 0; k < nc; k++)
            if (bad.bad(k))
                MI_FAIL(ctx, MI_EINVAL, "phase2 verify sigma: claim.basis_exp_sigma[" + std::to_string(k) + "][" + std::to_string(bad.host[k]) + "] is not a point of the curve");
    }
    Fr *r = nullptr;
    MI_TRY(ar.alloc(ctx, &r, (size_t)nr));
    MI_TRY(coeffs_enqueue(ctx, seed, nr, r));
    MI_TRY(sync_lap(ctx, ck, stats.coeff_ms));
    std::vector<G1Aff> sum_basis(nc), sum_bes(nc);
    for (u32 k = 0; k < nc; k++) {
        MI_TRY(msm_g1(ctx, (const G1Aff *)S->ped[k].basis, r, S->ped[k].n, &sum_basis[k]));
        MI_TRY(msm_g1(ctx, bes[k], r, S->ped[k].n, &sum_bes[k]));
    }
    ck.lap(stats.msm_g1_ms);
    ar.release(r);
    Relations rel;   // e(sum r_i Basis_k[i], g_sigma_neg'_k) e(sum r_i BES'_k[i], g2) = 1
    for (u32 k = 0; k < nc; k++) rel.add(sum_basis[k], g2_of(claim->g_sigma_neg[k]), g1_aff_neg(sum_bes[k]), g2_generator());
    MI_TRY(judge(ctx, ar, rel, bad));
    ck.lap(stats.pairing_ms);
    stats.peak_bytes = ar.peak;
    return MI_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------- shared with keyaudit.hip
void CeremonyRelations::add(const G1Aff &pa, const G2Aff &qa, const G1Aff &pb, const G2Aff &qb) {
    p.push_back(pa); q.push_back(qa);
    p.push_back(g1_aff_neg(pb)); q.push_back(qb);
}
int32_t mi_ceremony_seed_or_random(mi_ctx *ctx, const char *who, const uint8_t *&seed, uint8_t own[32]) { return seed_or_random(ctx, who, seed, own); }
int32_t mi_ceremony_coeffs_enqueue(mi_ctx *ctx, const uint8_t seed[32], u64 n, Fr *out_dev) { return coeffs_enqueue(ctx, seed, n, out_dev); }
int32_t mi_ceremony_msm_g1(mi_ctx *ctx, const void *bases, const Fr *scalars, u64 n, G1Aff *out) { return msm_g1(ctx, (const G1Aff *)bases, scalars, n, out); }
int32_t mi_ceremony_msm_g2(mi_ctx *ctx, const void *bases, const Fr *scalars, u64 n, G2Aff *out) { return msm_g2(ctx, (const G2Aff *)bases, scalars, n, out); }
int32_t mi_ceremony_judge(mi_ctx *ctx, Arena &ar, const CeremonyRelations &rel, std::vector<uint8_t> &bad) { return judge(ctx, ar, rel, bad); }

// ---------------------------------------------------------------------------------------------------- shared with phase1.hip
// abi_glue.h: the drawn nonce of a proved contribution, phase 1's and phase 2's
int32_t mi_draw_nonce(mi_ctx *ctx, const char *msg_no_random, const char *msg_zero, Fr &k) {
    uint8_t b[MI_H2F_BYTES];
    MI_TRY(mi_os_random(ctx, msg_no_random, b, sizeof(b)));
    k = fr_from_be48(b);
    if (k.is_zero()) MI_FAIL(ctx, MI_ENODEV, msg_zero);
    return MI_OK;
}
int32_t mi_srs_check_rows_dev(mi_ctx *ctx, const char *who, const mi_srs_desc *rows_dev, u64 N, const uint8_t *seed, mi_srs_check_stats &stats, uint32_t *failed) {
    uint8_t own_seed[32];
    MI_TRY(seed_or_random(ctx, who, seed, own_seed));
    const double t0 = now_ms();
    stats = mi_srs_check_stats{};
    const int32_t rc = srs_check_run(ctx, rows_dev, true, N, seed, 0, stats, failed);
    if (rc != MI_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    stats.total_ms = (float)(now_ms() - t0);
    return MI_OK;
}

extern "C" {

int32_t mi_debug_ceremony_coeffs_dev(mi_ctx *ctx, const uint8_t seed[32], size_t n, mi_fr *out_dev) {
    if (!ctx || !seed || (!out_dev && n) || n > MI_MSM_MAX_PAIRS) return MI_EINVAL;
    return coeffs_enqueue(ctx, seed, n, (Fr *)out_dev);
}

int32_t mi_srs_check_get_stats(mi_ctx *ctx, mi_srs_check_stats *out) {
    if (!ctx || !out) return MI_EINVAL;
    *out = ctx->srs_check_stats;
    return MI_OK;
}
int32_t mi_phase2_verify_get_stats(mi_ctx *ctx, mi_srs_check_stats *out) {
    if (!ctx || !out) return MI_EINVAL;
    *out = ctx->phase2_verify_stats;
    return MI_OK;
}

int32_t mi_srs_check_powers(mi_ctx *ctx, const mi_srs_desc *srs, uint64_t n_domain, const uint8_t *seed, uint32_t flags, uint32_t *failed) {
    if (!ctx) return MI_EINVAL;
    if (!failed) MI_FAIL(ctx, MI_EINVAL, "srs check: failed is null");
    if (flags & ~MI_KEYFILE_NO_SUBGROUP_CHECK) MI_FAIL(ctx, MI_EINVAL, "srs check: unknown flag");
    if (n_domain < 2 || (n_domain & (n_domain - 1)) || n_domain > ((uint64_t)1 << MI_SETUP_MAX_LOG_N))
        MI_FAIL(ctx, MI_EINVAL, "srs check: n_domain is " + std::to_string(n_domain) + ", not a power of two from 2 to 2^" + std::to_string(MI_SETUP_MAX_LOG_N));
    MI_TRY(mi_phase2_srs_host_check(ctx, srs, n_domain));
    uint8_t own_seed[32];
    MI_TRY(seed_or_random(ctx, "srs check", seed, own_seed));
    const double t0 = now_ms();
    ctx->srs_check_stats = mi_srs_check_stats{};
    const int32_t rc = srs_check_run(ctx, srs, false, n_domain, seed, flags, ctx->srs_check_stats, failed);
    if (rc != MI_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }   // the arena has freed everything
    ctx->srs_check_stats.total_ms = (float)(now_ms() - t0);
    return MI_OK;
}

int32_t mi_phase2_set_transcript_id(mi_ctx *ctx, mi_phase2 *S, const uint8_t id[32]) {
    if (!ctx) return MI_EINVAL;
    if (!S || !id) MI_FAIL(ctx, MI_EINVAL, "phase2: the state or the transcript id is null");
    if (S->n_records) MI_FAIL(ctx, MI_EINVAL, "phase2: the transcript id is set before the first record only; the state holds " + std::to_string(S->n_records));
    if (S->n_sigma_records)
        MI_FAIL(ctx, MI_EINVAL, "phase2: the transcript id is set before the first record only; the state's sigma chain holds " + std::to_string(S->n_sigma_records));
    std::memcpy(S->chain, id, 32);
    std::memcpy(S->sigma_chain, id, 32);
    return MI_OK;
}

int32_t mi_phase2_contribute_proved(mi_ctx *ctx, mi_phase2 *S, const mi_fr *delta, const mi_fr *nonce, mi_phase2_record *out) {
    if (!ctx) return MI_EINVAL;
    if (!S) MI_FAIL(ctx, MI_EINVAL, "phase2: the state is null");
    if (!delta) MI_FAIL(ctx, MI_EINVAL, "phase2: delta is null");
    if (!out) MI_FAIL(ctx, MI_EINVAL, "phase2: the record's out is null");
    Fr d, k;
    std::memcpy(&d, delta, 32);
    if (d.is_zero()) MI_FAIL(ctx, MI_EINVAL, "phase2: delta is 0");
    if (!fe_is_reduced(d)) MI_FAIL(ctx, MI_EINVAL, "phase2: delta is not below r");
    MI_TRY(nonce_or_random(ctx, nonce, k));
    const G1Aff before = S->delta1;
    MI_TRY(mi_phase2_contribute(ctx, S, delta, nullptr));
    CeremonyRecord rec;
    ceremony_record_make(S->chain, S->n_records, before, S->delta1, d, k, &rec);
    std::memcpy(out, &rec, sizeof(rec));
    std::memcpy(S->chain, rec.hash, 32);
    S->n_records++;
    return MI_OK;
}

int32_t mi_phase2_verify_adopt(mi_ctx *ctx, mi_phase2 *S, const mi_phase2_claim *claim, const mi_phase2_record *rec, size_t m, const uint8_t *seed,
                               uint32_t *failed, uint64_t *first_bad_record) {
    if (!ctx) return MI_EINVAL;
    if (!S) MI_FAIL(ctx, MI_EINVAL, "phase2 verify: the state is null");
    if (!m) MI_FAIL(ctx, MI_EINVAL, "phase2 verify: m is 0: a claimed state comes with the records of its contributions");
    if (!claim || !rec || !failed) MI_FAIL(ctx, MI_EINVAL, "phase2 verify: claim, rec or failed is null");
    if (claim->n_z != S->N) MI_FAIL(ctx, MI_EINVAL, "phase2 verify: claim.n_z is " + std::to_string(claim->n_z) + ", the state's Z holds " + std::to_string(S->N) + " points");
    if (claim->n_k != S->n_k) MI_FAIL(ctx, MI_EINVAL, "phase2 verify: claim.n_k is " + std::to_string(claim->n_k) + ", the state's K holds " + std::to_string(S->n_k) + " points");
    if (!claim->g1_z || (!claim->g1_k && claim->n_k)) MI_FAIL(ctx, MI_EINVAL, "phase2 verify: claim.g1_z or claim.g1_k is null");
    const G1Aff d1 = g1_of(claim->delta1);
    const G2Aff d2 = g2_of(claim->delta2);
    if (d1.is_inf() || !g1_on_curve(d1)) MI_FAIL(ctx, MI_EINVAL, "phase2 verify: claim.delta1 is at infinity or not on its curve");
    if (d2.is_inf() || !g2_reduced(d2) || !g2_on_twist(d2)) MI_FAIL(ctx, MI_EINVAL, "phase2 verify: claim.delta2 is at infinity or not on its curve");
    if (!g2_in_subgroup_psi(&d2)) MI_FAIL(ctx, MI_EINVAL, "phase2 verify: claim.delta2 is not in the r-torsion");
    uint8_t own_seed[32];
    MI_TRY(seed_or_random(ctx, "phase2 verify", seed, own_seed));
    const double t0 = now_ms();
    ctx->phase2_verify_stats = mi_srs_check_stats{};
    Arena ar;
    Claim c;
    bool z_bad = true, k_bad = true, delta_bad = true;
    const int32_t rc = verify_run(ctx, S, claim, d1, d2, seed, ar, c, &z_bad, &k_bad, &delta_bad);
    if (rc != MI_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    // the chain, on the host: from where this state stands
    const uint64_t fb = ceremony_records_first_bad(S->delta1, S->chain, S->n_records, (const CeremonyRecord *)rec, m);
    const G1Aff last = g1_of(rec[m - 1].delta1);
    uint32_t mask = 0;
    if (fb != m) mask |= MI_PHASE2_BAD_RECORD;
    if (delta_bad || std::memcmp(&last, &d1, sizeof(d1)) != 0) mask |= MI_PHASE2_BAD_DELTA;
    if (z_bad) mask |= MI_PHASE2_BAD_Z;
    if (k_bad) mask |= MI_PHASE2_BAD_K;
    *failed = mask;
    if (first_bad_record) *first_bad_record = fb;
    if (!mask) {   // the state takes the claimed arrays as they stand on the device; nothing below can fail
        (void)hipFree(S->g1_z); (void)hipFree(S->g1_k);
        S->g1_z = c.z; S->g1_k = c.k;
        ar.disown(c.z); ar.disown(c.k);
        S->delta1 = d1; S->delta2 = d2;
        std::memcpy(S->chain, rec[m - 1].hash, 32);
        S->n_records += m;
    }
    ctx->phase2_verify_stats.total_ms = (float)(now_ms() - t0);
    return MI_OK;
}

// ---------------------------------------------------------------------------------------------------- sigma
int32_t mi_phase2_get_chain_info(mi_ctx *ctx, const mi_phase2 *S, mi_phase2_chain_info *out) {
    if (!ctx) return MI_EINVAL;
    if (!S || !out) MI_FAIL(ctx, MI_EINVAL, "phase2: the state or out is null");
    std::memset(out, 0, sizeof(*out));
    out->n_commitments = S->n_commitments;
    out->n_records = S->n_records;
    std::memcpy(out->chain, S->chain, 32);
    out->n_sigma_records = S->n_sigma_records;
    std::memcpy(out->sigma_chain, S->sigma_chain, 32);
    return MI_OK;
}

int32_t mi_phase2_contribute_sigma_proved(mi_ctx *ctx, mi_phase2 *S, const mi_fr *sigma_factor, const mi_fr *nonce, mi_phase2_sigma_proof *out, uint8_t hash_out[32]) {
    if (!ctx) return MI_EINVAL;
    if (!S) MI_FAIL(ctx, MI_EINVAL, "phase2: the state is null");
    if (!sigma_factor) MI_FAIL(ctx, MI_EINVAL, "phase2: sigma_factor is null");
    if (!out || !hash_out) MI_FAIL(ctx, MI_EINVAL, "phase2: the step's out or hash_out is null");
    const u32 nc = S->n_commitments;
    if (!nc) MI_FAIL(ctx, MI_EINVAL, "phase2: the state has no commitments, so no sigma to contribute to");
    std::vector<Fr> s(nc), n(nc);
    for (u32 k = 0; k < nc; k++) {
        std::memcpy(&s[k], &sigma_factor[k], 32);
        if (s[k].is_zero()) MI_FAIL(ctx, MI_EINVAL, "phase2: sigma_factor[" + std::to_string(k) + "] is 0");
        if (!fe_is_reduced(s[k])) MI_FAIL(ctx, MI_EINVAL, "phase2: sigma_factor[" + std::to_string(k) + "] is not below r");
    }
    for (u32 k = 0; k < nc; k++) MI_TRY(nonce_or_random(ctx, nonce ? nonce + k : nullptr, n[k]));
    std::vector<G2Aff> before(nc), after(nc);
    for (u32 k = 0; k < nc; k++) before[k] = S->ped[k].g_sigma_neg;
    MI_TRY(mi_phase2_scale_sigma(ctx, S, s.data()));
    for (u32 k = 0; k < nc; k++) after[k] = S->ped[k].g_sigma_neg;
    std::vector<CeremonySigmaProof> step(nc);
    uint8_t h[32];
    ceremony_sigma_step_make(S->sigma_chain, S->n_sigma_records, nc, before.data(), after.data(), s.data(), n.data(), step.data(), h);
    std::memcpy(out, step.data(), (size_t)nc * sizeof(CeremonySigmaProof));
    std::memcpy(hash_out, h, 32);
    std::memcpy(S->sigma_chain, h, 32);
    S->n_sigma_records++;
    return MI_OK;
}

int32_t mi_phase2_verify_adopt_sigma(mi_ctx *ctx, mi_phase2 *S, const mi_phase2_sigma_claim *claim, const mi_phase2_sigma_proof *proofs, const uint8_t (*hashes)[32],
                                     size_t m, const uint8_t *seed, uint32_t *failed, uint64_t *bad_commitments, uint64_t *first_bad_record) {
    if (!ctx) return MI_EINVAL;
    if (!S) MI_FAIL(ctx, MI_EINVAL, "phase2 verify sigma: the state is null");
    if (!m) MI_FAIL(ctx, MI_EINVAL, "phase2 verify sigma: m is 0: a claimed state comes with the steps of its contributions");
    if (!claim || !proofs || !hashes || !failed || !bad_commitments) MI_FAIL(ctx, MI_EINVAL, "phase2 verify sigma: claim, proofs, hashes, failed or bad_commitments is null");
    const u32 nc = S->n_commitments;
    if (!nc) MI_FAIL(ctx, MI_EINVAL, "phase2 verify sigma: the state has no commitments");
    if (nc > 64) MI_FAIL(ctx, MI_EINVAL, "phase2 verify sigma: bad_commitments has a bit for 64 commitments, the state has " + std::to_string(nc));
    if (!claim->basis_exp_sigma || !claim->n || !claim->g_sigma_neg) MI_FAIL(ctx, MI_EINVAL, "phase2 verify sigma: claim.basis_exp_sigma, claim.n or claim.g_sigma_neg is null");
    for (u32 k = 0; k < nc; k++) {
        const std::string name = "claim.g_sigma_neg[" + std::to_string(k) + "]";
        if (claim->n[k] != S->ped[k].n)
            MI_FAIL(ctx, MI_EINVAL, "phase2 verify sigma: claim.n[" + std::to_string(k) + "] is " + std::to_string(claim->n[k]) + ", the state's commitment holds " + std::to_string(S->ped[k].n) + " points");
        if (!claim->basis_exp_sigma[k] && claim->n[k]) MI_FAIL(ctx, MI_EINVAL, "phase2 verify sigma: claim.basis_exp_sigma[" + std::to_string(k) + "] is null");
        const G2Aff gs = g2_of(claim->g_sigma_neg[k]);
        if (gs.is_inf() || !g2_reduced(gs) || !g2_on_twist(gs)) MI_FAIL(ctx, MI_EINVAL, "phase2 verify sigma: " + name + " is at infinity or not on its curve");
        if (!g2_in_subgroup_psi(&gs)) MI_FAIL(ctx, MI_EINVAL, "phase2 verify sigma: " + name + " is not in the r-torsion");
    }
    uint8_t own_seed[32];
    MI_TRY(seed_or_random(ctx, "phase2 verify sigma", seed, own_seed));
    const double t0 = now_ms();
    ctx->phase2_verify_stats = mi_srs_check_stats{};
    Arena ar;
    std::vector<G1Aff *> bes(nc, nullptr);
    std::vector<uint8_t> bad;
    const int32_t rc = sigma_verify_run(ctx, S, claim, seed, ar, bes, bad);
    if (rc != MI_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    // the chain, on the host: from where this state stands
    std::vector<G2Aff> start(nc);
    for (u32 k = 0; k < nc; k++) start[k] = S->ped[k].g_sigma_neg;
    const uint64_t fb = ceremony_sigma_first_bad(start.data(), nc, S->sigma_chain, S->n_sigma_records, (const CeremonySigmaProof *)proofs, hashes, m);
    uint32_t mask = 0;
    uint64_t bad_k = 0;
    if (fb != m) mask |= MI_PHASE2_BAD_SIGMA_RECORD;
    for (u32 k = 0; k < nc; k++) {
        if (std::memcmp(&proofs[(m - 1) * nc + k].g_sigma_neg, &claim->g_sigma_neg[k], sizeof(mi_g2_affine)) != 0) mask |= MI_PHASE2_BAD_SIGMA_LINK;
        if (bad[k]) { mask |= MI_PHASE2_BAD_BES; bad_k |= (uint64_t)1 << k; }
    }
    *failed = mask;
    *bad_commitments = bad_k;
    if (first_bad_record) *first_bad_record = fb;
    if (!mask) {   // the state takes the claimed arrays as they stand on the device; nothing below can fail
        for (u32 k = 0; k < nc; k++) {
            (void)hipFree(S->ped[k].bes);
            S->ped[k].bes = bes[k];
            ar.disown(bes[k]);
            S->ped[k].g_sigma_neg = g2_of(claim->g_sigma_neg[k]);
            S->ped[k].sigma_known = false;   // points from outside: the scalar the state once had says nothing about them
        }
        std::memcpy(S->sigma_chain, hashes[m - 1], 32);
        S->n_sigma_records += m;
    }
    ctx->phase2_verify_stats.total_ms = (float)(now_ms() - t0);
    return MI_OK;
}

}  // extern "C"

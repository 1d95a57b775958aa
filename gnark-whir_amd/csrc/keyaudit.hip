// The audit of a key against its circuit and an SRS (include/mi355x_groth16_keyaudit.h): every array of the key is checked by ONE random
// linear combination instead of being derived again.  With r_j per wire (the ceremony checks' coefficient stream) and a wire class X,
//     sum_{j in X} r_j [M_j]1 = sum_i (M r^X)_i [L_i(tau)]1 = MSM(iNTT_N(M r^X), tau row)
// so the SRS side of a relation is a product by rows (r1cs.hip, as it is), an Fr transform (ntt.hip) and an MSM (msm.hip); the key side
// is an MSM over the claimed array with the coefficients gathered into its compacted order.  What is new on the device is small and is
// keyaudit_ops.cuh's text, one lane per element, 64 lanes per workgroup:
//   k_keyaudit_mask        r^X from r and the wire classes
//   k_keyaudit_gather      out[s] = r[wire[s]]: the coefficients in the order of pk.A / B / K, vk.K, a basis
//   k_keyaudit_bitrev      out[i] = in[bitrev(i)]: the Z coefficients in stored order
//   k_keyaudit_unreverse   a DIF transform's output to natural order, and (acc != null) its sum into the unmasked vector
// The points of mi_key_claim_from_arrays go through point_check.cuh's k_points_check_g1 / _g2 under POINT_RULE_AUDIT.
// Coefficients, MSMs and the judgement of the pairing relations are phase2_check.hip's (phase2_internal.h); a stream is decoded by the
// loaders' own code (keyfile_internal.h).  The wire classes, the slot lists and the shape refusals are host code in keyaudit_ops.cuh.
// A = sum of the three class vectors, so nine masked products and nine transforms give every relation.  A host SRS goes up one row at a
// time, is checked by mi_phase2_check_points, summed and released, as mi_srs_check_powers does.
#include "verify_internal.h"
#include "phase2_internal.h"
#include "keyfile_internal.h"
#include "r1cs_internal.h"
#include "keyaudit_ops.cuh"
#include "keyfile_ops.cuh"
#include "point_check.cuh"
#include "stream_clock.h"
#include <cstring>
#include <string>
#include <vector>

struct mi_key_claim {
    const mi_phase2 *borrowed = nullptr;   // the state whose arrays these are (then nothing here is freed and all of it is re-read per audit)
    u64 nb_wires = 0;
    std::vector<uint8_t> inf_a, inf_b;
    void *arr[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // mi_pk_desc's order: G1.A, G1.B, G1.K, G1.Z, G2.B
    u64 n[5] = {0, 0, 0, 0, 0};
    struct Ped { void *basis = nullptr, *bes = nullptr; u64 n = 0; };
    std::vector<Ped> ped;
    G1Aff alpha1, beta1, delta1;   // the proving key's
    G2Aff beta2, delta2;
    G1Aff vk_alpha1;               // the verifying key's
    G2Aff vk_beta2, vk_gamma2, vk_delta2;
    void *vk_k = nullptr;
    u64 n_vk = 0;
    std::vector<mi_pedersen_vk> vk_ped;
};

namespace {

enum { ARR_A, ARR_B, ARR_K, ARR_Z, ARR_G2B };

__global__ void __launch_bounds__(64) k_keyaudit_mask(const Fr *r, const uint8_t *cls, uint8_t want, u64 n, Fr *out) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) out[j] = keyaudit_masked(r[j], cls[j], want);
}
__global__ void __launch_bounds__(64) k_keyaudit_gather(const Fr *r, const u32 *wire, u64 n, Fr *out) {
    const u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < n) out[s] = r[wire[s]];
}
__global__ void __launch_bounds__(64) k_keyaudit_bitrev(const Fr *in, u32 log_n, Fr *out) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < ((u64)1 << log_n)) out[i] = in[keyaudit_bitrev(i, log_n)];
}
__global__ void __launch_bounds__(64) k_keyaudit_unreverse(const Fr *in, u32 log_n, Fr *out, Fr *acc) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ((u64)1 << log_n)) return;
    const Fr v = in[keyaudit_bitrev(i, log_n)];
    out[i] = v;
    if (acc) acc[i] = acc[i] + v;
}

bool same(const G1Aff &a, const G1Aff &b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }
bool same(const G2Aff &a, const G2Aff &b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }
G1Aff g1_sum(const G1Aff &a, const G1Aff &b, bool negate_b = false) {
    G1X acc = G1X::from_affine(a);
    xyzz_madd(acc, b, negate_b);
    return xyzz_to_affine(acc);
}

void free_claim(mi_key_claim *c) {
    if (!c) return;
    if (!c->borrowed) {
        for (void *a : c->arr) if (a) (void)hipFree(a);
        for (const auto &p : c->ped) { if (p.basis) (void)hipFree(p.basis); if (p.bes) (void)hipFree(p.bes); }
        if (c->vk_k) (void)hipFree(c->vk_k);
    }
    delete c;
}
// the state's arrays where they are now, its small points and the Pedersen pairs of its [-sigma]2 points
int32_t view_state(mi_ctx *ctx, const mi_phase2 *S, mi_key_claim &c) {
    c.borrowed = S;
    c.nb_wires = S->nb_wires;
    c.inf_a = S->inf_a; c.inf_b = S->inf_b;
    c.arr[ARR_A] = S->g1_a; c.arr[ARR_B] = S->g1_b; c.arr[ARR_K] = S->g1_k; c.arr[ARR_Z] = S->g1_z; c.arr[ARR_G2B] = S->g2_b;
    c.n[ARR_A] = S->n_a; c.n[ARR_B] = c.n[ARR_G2B] = S->n_b; c.n[ARR_K] = S->n_k; c.n[ARR_Z] = S->N;
    c.ped.clear();
    for (size_t k = 0; k < S->ped.size(); k++) {
        mi_key_claim::Ped p;
        p.basis = S->ped[k].basis; p.bes = S->ped[k].bes; p.n = S->ped[k].n;
        c.ped.push_back(p);
    }
    c.alpha1 = c.vk_alpha1 = S->alpha1; c.beta1 = S->beta1; c.delta1 = S->delta1;
    c.beta2 = c.vk_beta2 = S->beta2; c.delta2 = c.vk_delta2 = S->delta2; c.vk_gamma2 = S->gamma2;
    c.vk_k = S->vk_k; c.n_vk = S->n_vk;
    c.vk_ped.assign(S->ped.size(), mi_pedersen_vk{});
    mi_phase2_pedersen_vk_of(S, c.vk_ped.data());
    return MI_OK;
}

// ---------------------------------------------------------------------------------------------------- the points of plain arrays
struct ClaimArray { std::string name; bool g2, allow_inf; const void *pts; u64 n; };
int32_t check_arrays(mi_ctx *ctx, const std::vector<ClaimArray> &arrs) {
    BadSlots bad;   // word 2 i: array i on its curve; 2 i + 1: a G2 array in the r-torsion
    auto body = [&]() -> int32_t {
        MI_TRY(bad.init(ctx, 2 * arrs.size()));
        for (size_t i = 0; i < arrs.size(); i++) {
            const ClaimArray &a = arrs[i];
            MI_TRY(mi_points_check_enqueue(ctx, a.g2, a.pts, a.n, point_rule_audit(a.allow_inf), bad.dev + 2 * i));
            if (a.g2) MI_TRY(mi_keyfile_subgroup_enqueue(ctx, a.pts, (size_t)a.n, false, bad.dev + 2 * i + 1));   // a word that is no point fails the curve check, which is reported first
        }
        return bad.fetch(ctx);
    };
    const int32_t rc = body();
    if (rc != MI_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    for (size_t i = 0; i < arrs.size(); i++) {
        if (bad.bad(2 * i))
            MI_FAIL(ctx, MI_EINVAL, "key claim: " + arrs[i].name + "[" + std::to_string(bad.host[2 * i]) + "] is not a point of its curve" + (arrs[i].allow_inf ? "" : " or is at infinity"));
        if (bad.bad(2 * i + 1)) MI_FAIL(ctx, MI_EINVAL, "key claim: " + arrs[i].name + "[" + std::to_string(bad.host[2 * i + 1]) + "] is not in the r-torsion");
    }
    return MI_OK;
}
int32_t small_g1(mi_ctx *ctx, const char *name, const G1Aff &p) {
    if (p.is_inf() || !g1_on_curve(p)) MI_FAIL(ctx, MI_EINVAL, std::string("key claim: ") + name + " is at infinity or not on its curve");
    return MI_OK;
}
int32_t small_g2(mi_ctx *ctx, const char *name, const G2Aff &q, bool allow_inf = false) {
    if ((q.is_inf() && !allow_inf) || !g2_reduced(q) || !g2_on_twist(q)) MI_FAIL(ctx, MI_EINVAL, std::string("key claim: ") + name + " is at infinity or not on its curve");
    if (!g2_in_subgroup_psi(&q)) MI_FAIL(ctx, MI_EINVAL, std::string("key claim: ") + name + " is not in the r-torsion");
    return MI_OK;
}

// ---------------------------------------------------------------------------------------------------- the audit
struct AuditIn {
    const mi_r1cs_desc *d;
    const R1csShape *sh;
    const mi_srs_desc *rows;
    bool on_device;
    const mi_key_claim *c;
    const KeyAuditWires *w;
    const uint8_t *seed;
    uint32_t flags;
};
int32_t audit_run(mi_ctx *ctx, const AuditIn &in, const mi_r1cs *R, Arena &ar, mi_key_audit_stats &stats, mi_key_audit_sums &sums, uint32_t *failed) {
    hipStream_t st = ctx->stream;
    const R1csShape &sh = *in.sh;
    const mi_key_claim &c = *in.c;
    const KeyAuditWires &w = *in.w;
    const u64 N = sh.N, nw = sh.nb_wires, nc = sh.nc;
    const u32 n_ped = sh.n_commitments;
    HostClock ck;
    // ---- the wire classes and the slot lists go up
    uint8_t *cls = nullptr;
    MI_TRY(ar.alloc(ctx, &cls, (size_t)nw));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(cls, w.cls.data(), nw, hipMemcpyHostToDevice, st));
    auto up_list = [&](const std::vector<u32> &l, u32 **dev) -> int32_t {
        MI_TRY(ar.alloc(ctx, dev, l.size()));
        if (!l.empty()) MI_CHECK_HIP(ctx, hipMemcpyAsync(*dev, l.data(), l.size() * 4, hipMemcpyHostToDevice, st));
        return MI_OK;
    };
    u32 *l_a = nullptr, *l_b = nullptr, *l_k = nullptr, *l_v = nullptr;
    std::vector<u32 *> l_c(n_ped, nullptr);
    MI_TRY(up_list(w.a, &l_a)); MI_TRY(up_list(w.b, &l_b)); MI_TRY(up_list(w.k, &l_k)); MI_TRY(up_list(w.v, &l_v));
    for (u32 k = 0; k < n_ped; k++) MI_TRY(up_list(w.c[k], &l_c[k]));
    MI_TRY(sync_lap(ctx, ck, stats.upload_ms));
    // ---- coefficients: r_j = stream[j], q_i = stream[nb_wires + i]; the class vectors; the coefficients in every array's own order
    Fr *r = nullptr, *rx[KEYAUDIT_CLASSES] = {nullptr, nullptr, nullptr};
    Fr *s_a = nullptr, *s_b = nullptr, *s_k = nullptr, *s_v = nullptr, *s_z = nullptr;
    std::vector<Fr *> s_c(n_ped, nullptr);
    MI_TRY(ar.alloc(ctx, &r, (size_t)(nw + N)));
    MI_TRY(mi_ceremony_coeffs_enqueue(ctx, in.seed, nw + N, r));
    for (int x = 0; x < KEYAUDIT_CLASSES; x++) {
        MI_TRY(ar.alloc(ctx, &rx[x], (size_t)nw));
        MI_TRY(mi_launch64(ctx, k_keyaudit_mask, (size_t)nw, (const Fr *)r, (const uint8_t *)cls, (uint8_t)x, nw, rx[x]));
    }
    auto gather = [&](const std::vector<u32> &l, const u32 *dev, Fr **out) -> int32_t {
        MI_TRY(ar.alloc(ctx, out, l.size()));
        return mi_launch64(ctx, k_keyaudit_gather, l.size(), (const Fr *)r, dev, (u64)l.size(), *out);
    };
    MI_TRY(gather(w.a, l_a, &s_a)); MI_TRY(gather(w.b, l_b, &s_b)); MI_TRY(gather(w.k, l_k, &s_k)); MI_TRY(gather(w.v, l_v, &s_v));
    for (u32 k = 0; k < n_ped; k++) MI_TRY(gather(w.c[k], l_c[k], &s_c[k]));
    MI_TRY(ar.alloc(ctx, &s_z, (size_t)N));
    MI_TRY(mi_launch64(ctx, k_keyaudit_bitrev, (size_t)N, (const Fr *)(r + nw), sh.log_n, s_z));
    MI_TRY(sync_lap(ctx, ck, stats.coeff_ms));
    for (void *x : {(void *)cls, (void *)l_a, (void *)l_b, (void *)l_k, (void *)l_v}) ar.release(x);
    for (u32 *x : l_c) ar.release(x);
    // ---- per class: three products by rows, three inverse transforms (natural in, bit-reversed out), back to natural order; the
    // unmasked vectors of A and B are the sums over the classes
    Fr *tmp[3] = {nullptr, nullptr, nullptr}, *nat[KEYAUDIT_CLASSES][3], *p_a = nullptr, *p_b = nullptr;
    for (int m = 0; m < 3; m++) MI_TRY(ar.alloc(ctx, &tmp[m], (size_t)N));
    MI_TRY(ar.alloc(ctx, &p_a, (size_t)N));
    MI_TRY(ar.alloc(ctx, &p_b, (size_t)N));
    MI_CHECK_HIP(ctx, hipMemsetAsync(p_a, 0, N * sizeof(Fr), st));
    MI_CHECK_HIP(ctx, hipMemsetAsync(p_b, 0, N * sizeof(Fr), st));
    for (int x = 0; x < KEYAUDIT_CLASSES; x++) {
        for (int m = 0; m < 3; m++) {
            MI_TRY(ar.alloc(ctx, &nat[x][m], (size_t)N));
            if (N > nc) MI_CHECK_HIP(ctx, hipMemsetAsync(tmp[m] + nc, 0, (N - nc) * sizeof(Fr), st));
        }
        MI_TRY(mi_r1cs_eval_dev(ctx, R, (const mi_fr *)rx[x], MI_R1CS_A | MI_R1CS_B | MI_R1CS_C, (mi_fr *)tmp[0], (mi_fr *)tmp[1], (mi_fr *)tmp[2]));
        MI_TRY(sync_lap(ctx, ck, stats.sparse_ms));
        for (int m = 0; m < 3; m++) {
            if (sh.log_n) MI_TRY(mi_ntt_dev(ctx, (mi_fr *)tmp[m], sh.log_n, MI_NTT_INVERSE));
            MI_TRY(mi_launch64(ctx, k_keyaudit_unreverse, (size_t)N, (const Fr *)tmp[m], sh.log_n, nat[x][m], m == 0 ? p_a : m == 1 ? p_b : (Fr *)nullptr));
        }
        MI_TRY(sync_lap(ctx, ck, stats.transform_ms));
        ar.release(rx[x]);
    }
    for (Fr *x : tmp) ar.release(x);
    // ---- the SRS side, a row at a time
    const mi_srs_desc *srs = in.rows;
    auto g1_row = [&](const char *name, const mi_g1_affine *src, u64 n, G1Aff **row) -> int32_t {
        *row = (G1Aff *)src;
        if (in.on_device) return MI_OK;
        MI_TRY(ar.alloc(ctx, row, (size_t)n));
        MI_CHECK_HIP(ctx, hipMemcpyAsync(*row, src, n * sizeof(G1Aff), hipMemcpyHostToDevice, st));
        MI_TRY(sync_lap(ctx, ck, stats.upload_ms));
        const Phase2Row pr{name, false, *row, n};
        MI_TRY(mi_phase2_check_points(ctx, ar, &pr, 1, in.flags));
        ck.lap(stats.point_check_ms);
        return MI_OK;
    };
    auto first_of = [&](const G1Aff *row, const mi_g1_affine *host, G1Aff *out) -> int32_t {
        if (!in.on_device) { *out = g1_of(host[0]); return MI_OK; }
        MI_CHECK_HIP(ctx, hipMemcpyAsync(out, row, sizeof(G1Aff), hipMemcpyDeviceToHost, st));
        MI_CHECK_HIP(ctx, hipStreamSynchronize(st));
        return MI_OK;
    };
    G1Aff srs_a, srs_b1, t_part[3][KEYAUDIT_CLASSES], z_lo, z_hi, alpha0, beta0;
    G2Aff srs_b2;
    G1Aff *row = nullptr;
    MI_TRY(g1_row("tau_g1", srs->tau_g1, 2 * N, &row));
    MI_TRY(mi_ceremony_msm_g1(ctx, row, p_a, N, &srs_a));
    MI_TRY(mi_ceremony_msm_g1(ctx, row, p_b, N, &srs_b1));
    for (int x = 0; x < KEYAUDIT_CLASSES; x++) MI_TRY(mi_ceremony_msm_g1(ctx, row, nat[x][2], N, &t_part[2][x]));
    MI_TRY(mi_ceremony_msm_g1(ctx, row, r + nw, N, &z_lo));
    MI_TRY(mi_ceremony_msm_g1(ctx, row + N, r + nw, N, &z_hi));
    ck.lap(stats.srs_msm_g1_ms);
    if (!in.on_device) ar.release(row);
    MI_TRY(g1_row("alpha_tau_g1", srs->alpha_tau_g1, N, &row));
    MI_TRY(first_of(row, srs->alpha_tau_g1, &alpha0));
    for (int x = 0; x < KEYAUDIT_CLASSES; x++) MI_TRY(mi_ceremony_msm_g1(ctx, row, nat[x][1], N, &t_part[1][x]));
    ck.lap(stats.srs_msm_g1_ms);
    if (!in.on_device) ar.release(row);
    MI_TRY(g1_row("beta_tau_g1", srs->beta_tau_g1, N, &row));
    MI_TRY(first_of(row, srs->beta_tau_g1, &beta0));
    for (int x = 0; x < KEYAUDIT_CLASSES; x++) MI_TRY(mi_ceremony_msm_g1(ctx, row, nat[x][0], N, &t_part[0][x]));
    ck.lap(stats.srs_msm_g1_ms);
    if (!in.on_device) ar.release(row);
    if (in.on_device) {
        MI_TRY(mi_ceremony_msm_g2(ctx, srs->tau_g2, p_b, N, &srs_b2));
        ck.lap(stats.srs_msm_g2_ms);
    } else {
        G2Aff *row2 = nullptr, *b2 = nullptr;
        MI_TRY(ar.alloc(ctx, &row2, (size_t)N));
        MI_TRY(ar.alloc(ctx, &b2, (size_t)1));
        MI_CHECK_HIP(ctx, hipMemcpyAsync(row2, srs->tau_g2, N * sizeof(G2Aff), hipMemcpyHostToDevice, st));
        MI_CHECK_HIP(ctx, hipMemcpyAsync(b2, &srs->beta_g2, sizeof(G2Aff), hipMemcpyHostToDevice, st));
        MI_TRY(sync_lap(ctx, ck, stats.upload_ms));
        const Phase2Row pr[2] = {{"tau_g2", true, row2, N}, {"beta_g2", true, b2, 1}};
        MI_TRY(mi_phase2_check_points(ctx, ar, pr, 2, in.flags));
        ck.lap(stats.point_check_ms);
        MI_TRY(mi_ceremony_msm_g2(ctx, row2, p_b, N, &srs_b2));
        ck.lap(stats.srs_msm_g2_ms);
        ar.release(row2); ar.release(b2);
    }
    for (int x = 0; x < KEYAUDIT_CLASSES; x++) for (int m = 0; m < 3; m++) ar.release(nat[x][m]);
    ar.release(p_a); ar.release(p_b);
    // ---- the key side
    G1Aff key_a, key_b1, key_k, key_v, key_z, key_basis = G1Aff{Fp::zero(), Fp::zero()};
    G2Aff key_b2;
    std::vector<G1Aff> sum_basis(n_ped), sum_bes(n_ped);
    MI_TRY(mi_ceremony_msm_g1(ctx, c.arr[ARR_A], s_a, c.n[ARR_A], &key_a));
    MI_TRY(mi_ceremony_msm_g1(ctx, c.arr[ARR_B], s_b, c.n[ARR_B], &key_b1));
    MI_TRY(mi_ceremony_msm_g1(ctx, c.arr[ARR_K], s_k, c.n[ARR_K], &key_k));
    MI_TRY(mi_ceremony_msm_g1(ctx, c.vk_k, s_v, c.n_vk, &key_v));
    MI_TRY(mi_ceremony_msm_g1(ctx, c.arr[ARR_Z], s_z, N, &key_z));
    for (u32 k = 0; k < n_ped; k++) {
        MI_TRY(mi_ceremony_msm_g1(ctx, c.ped[k].basis, s_c[k], c.ped[k].n, &sum_basis[k]));
        MI_TRY(mi_ceremony_msm_g1(ctx, c.ped[k].bes, s_c[k], c.ped[k].n, &sum_bes[k]));
        key_basis = g1_sum(key_basis, sum_basis[k]);
    }
    ck.lap(stats.key_msm_g1_ms);
    MI_TRY(mi_ceremony_msm_g2(ctx, c.arr[ARR_G2B], s_b, c.n[ARR_G2B], &key_b2));
    ck.lap(stats.key_msm_g2_ms);
    // ---- the relations
    G1Aff T[KEYAUDIT_CLASSES];
    for (int x = 0; x < KEYAUDIT_CLASSES; x++) T[x] = g1_sum(g1_sum(t_part[0][x], t_part[1][x]), t_part[2][x]);
    const G1Aff srs_z = g1_sum(z_hi, z_lo, true);
    sums = mi_key_audit_sums{};
    auto put1 = [](mi_g1_affine out[2], const G1Aff &key, const G1Aff &s) { std::memcpy(&out[0], &key, 64); std::memcpy(&out[1], &s, 64); };
    put1(sums.a, key_a, srs_a); put1(sums.b1, key_b1, srs_b1); put1(sums.k_private, key_k, T[KEYAUDIT_P]); put1(sums.k_public, key_v, T[KEYAUDIT_V]);
    put1(sums.basis, key_basis, T[KEYAUDIT_C]); put1(sums.z, key_z, srs_z);
    std::memcpy(&sums.b2[0], &key_b2, 128); std::memcpy(&sums.b2[1], &srs_b2, 128);
    for (u32 k = 0; k < n_ped; k++) put1(sums.sigma[k], sum_basis[k], sum_bes[k]);
    sums.n_sigma = n_ped; sums.valid = 1;
    const G1Aff g1 = g1_generator();
    const G2Aff g2 = g2_generator();
    CeremonyRelations rel;
    rel.add(c.delta1, g2, g1, c.delta2);              // MI_KEY_BAD_SMALL's pairing
    rel.add(key_k, c.delta2, T[KEYAUDIT_P], g2);      // MI_KEY_BAD_K_PRIVATE
    rel.add(key_v, c.vk_gamma2, T[KEYAUDIT_V], g2);   // MI_KEY_BAD_K_PUBLIC
    rel.add(key_basis, c.vk_gamma2, T[KEYAUDIT_C], g2);   // MI_KEY_BAD_BASIS
    rel.add(key_z, c.delta2, srs_z, g2);              // MI_KEY_BAD_Z
    for (u32 k = 0; k < n_ped; k++)                   // MI_KEY_BAD_SIGMA: e(basis, g_sigma_neg) e(bes, g) = 1
        rel.add(sum_basis[k], g2_of(c.vk_ped[k].g_sigma_neg), g1_aff_neg(sum_bes[k]), g2_of(c.vk_ped[k].g));
    std::vector<uint8_t> bad;
    MI_TRY(mi_ceremony_judge(ctx, ar, rel, bad));
    ck.lap(stats.pairing_ms);
    stats.relations = rel.count();
    uint32_t mask = 0;
    if (!same(c.alpha1, c.vk_alpha1) || !same(c.alpha1, alpha0) || !same(c.beta1, beta0) || !same(c.beta2, c.vk_beta2) ||
        !same(c.beta2, g2_of(srs->beta_g2)) || !same(c.delta2, c.vk_delta2) || bad[0])
        mask |= MI_KEY_BAD_SMALL;
    if (!same(key_a, srs_a)) mask |= MI_KEY_BAD_A;
    if (!same(key_b1, srs_b1)) mask |= MI_KEY_BAD_B1;
    if (!same(key_b2, srs_b2)) mask |= MI_KEY_BAD_B2;
    const uint32_t bits[4] = {MI_KEY_BAD_K_PRIVATE, MI_KEY_BAD_K_PUBLIC, MI_KEY_BAD_BASIS, MI_KEY_BAD_Z};
    for (int i = 0; i < 4; i++) if (bad[1 + i]) mask |= bits[i];
    for (u32 k = 0; k < n_ped; k++) if (bad[5 + k]) mask |= MI_KEY_BAD_SIGMA;
    *failed = mask;
    return MI_OK;
}

}  // namespace

extern "C" {

int32_t mi_key_claim_free(mi_ctx *ctx, mi_key_claim *c) {
    if (!ctx || !c) return MI_EINVAL;
    (void)hipStreamSynchronize(ctx->stream);
    free_claim(c);
    return MI_OK;
}

int32_t mi_key_claim_from_phase2(mi_ctx *ctx, const mi_phase2 *S, mi_key_claim **out) {
    if (!ctx) return MI_EINVAL;
    if (!out) MI_FAIL(ctx, MI_EINVAL, "key claim: out is null");
    *out = nullptr;
    if (!S) MI_FAIL(ctx, MI_EINVAL, "key claim: the state is null");
    mi_key_claim *c = new (std::nothrow) mi_key_claim();
    if (!c) return MI_ENOMEM;
    const int32_t rc = view_state(ctx, S, *c);
    if (rc != MI_OK) { delete c; return rc; }
    *out = c;
    return MI_OK;
}

int32_t mi_key_claim_from_streams(mi_ctx *ctx, const uint8_t *pk_buf, size_t pk_len, const uint8_t *vk_buf, size_t vk_len, uint32_t flags, mi_key_claim **out) {
    if (!ctx) return MI_EINVAL;
    if (!out) MI_FAIL(ctx, MI_EINVAL, "key claim: out is null");
    *out = nullptr;
    if (!pk_buf || !vk_buf) MI_FAIL(ctx, MI_EINVAL, "key claim: a null stream");
    mi_key_claim *c = new (std::nothrow) mi_key_claim();
    if (!c) return MI_ENOMEM;
    auto body = [&]() -> int32_t {
        PkStreamDecoded pk;
        MI_TRY(mi_pk_stream_decode(ctx, pk_buf, pk_len, flags, true, pk));
        VkStreamDecoded vk;
        MI_TRY(mi_vk_stream_decode(ctx, vk_buf, vk_len, flags, vk));
        const mi_pk_raw_info &in = pk.in;
        c->nb_wires = in.nb_wires;
        c->inf_a.swap(pk.inf_a); c->inf_b.swap(pk.inf_b);
        const u64 counts[5] = {in.n_g1_a, in.n_g1_b, in.n_g1_k, in.n_g1_z, in.n_g2_b};
        for (int i = 0; i < 5; i++) { c->arr[i] = pk.arr[i]; pk.arr[i] = nullptr; c->n[i] = counts[i]; }
        for (size_t k = 0; k < pk.ped.size() / 2; k++) {
            mi_key_claim::Ped p;
            p.basis = pk.ped[2 * k]; p.bes = pk.ped[2 * k + 1]; p.n = in.n_basis[k];
            pk.ped[2 * k] = pk.ped[2 * k + 1] = nullptr;
            c->ped.push_back(p);
        }
        c->alpha1 = g1_of(pk.small1[0]); c->beta1 = g1_of(pk.small1[1]); c->delta1 = g1_of(pk.small1[2]);
        c->beta2 = g2_of(pk.small2[0]); c->delta2 = g2_of(pk.small2[1]);
        c->vk_alpha1 = g1_of(vk.g1[0]);
        c->vk_beta2 = g2_of(vk.g2[0]); c->vk_gamma2 = g2_of(vk.g2[1]); c->vk_delta2 = g2_of(vk.g2[2]);
        c->n_vk = vk.in.n_k;
        for (uint32_t k = 0; k < vk.in.n_commitment_keys; k++) {
            mi_pedersen_vk p;
            p.g = vk.g2[3 + 2 * k]; p.g_sigma_neg = vk.g2[4 + 2 * k];
            c->vk_ped.push_back(p);
        }
        // all of K in one array: K[0], then what the decoder left on the device
        MI_CHECK_HIP(ctx, hipMalloc(&c->vk_k, (size_t)c->n_vk * sizeof(G1Aff) + 64));
        MI_CHECK_HIP(ctx, hipMemcpyAsync(c->vk_k, vk.k.data(), (size_t)c->n_vk * sizeof(G1Aff), hipMemcpyHostToDevice, ctx->stream));
        MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return MI_OK;
    };
    const int32_t rc = body();
    if (rc != MI_OK) { (void)hipStreamSynchronize(ctx->stream); free_claim(c); return rc; }
    *out = c;
    return MI_OK;
}

int32_t mi_key_claim_from_arrays(mi_ctx *ctx, const mi_pk_desc *d, const mi_pedersen_arrays *ped, uint32_t n_ped, const mi_vk_desc *vk, mi_key_claim **out) {
    if (!ctx) return MI_EINVAL;
    if (!out) MI_FAIL(ctx, MI_EINVAL, "key claim: out is null");
    *out = nullptr;
    if (!d || !vk) MI_FAIL(ctx, MI_EINVAL, "key claim: desc or vk_desc is null");
    if (n_ped > MI_PK_RAW_MAX_COMMITMENTS || vk->n_commitments > MI_PK_RAW_MAX_COMMITMENTS) MI_FAIL(ctx, MI_EINVAL, "key claim: more than MI_PK_RAW_MAX_COMMITMENTS Pedersen keys");
    if ((n_ped && !ped) || (vk->n_commitments && !vk->ped)) MI_FAIL(ctx, MI_EINVAL, "key claim: ped or vk_desc.ped is null");
    if (d->nb_wires == 0 || d->nb_wires > MI_MSM_MAX_PAIRS || !d->infinity_a || !d->infinity_b) MI_FAIL(ctx, MI_EINVAL, "key claim: nb_wires is 0 or above 2^27, or a null infinity mask");
    const struct { const void *p; u64 n; } src[5] = {{d->g1_a, d->n_g1_a}, {d->g1_b, d->n_g1_b}, {d->g1_k, d->n_g1_k}, {d->g1_z, d->n_g1_z}, {d->g2_b, d->n_g2_b}};
    for (const auto &a : src) {
        if (!a.p && a.n) MI_FAIL(ctx, MI_EINVAL, "key claim: a null point array with a count that is not 0");
        if (a.n > ((u64)1 << 28)) MI_FAIL(ctx, MI_EINVAL, "key claim: an array of more than 2^28 points");
    }
    for (uint32_t k = 0; k < n_ped; k++) if ((!ped[k].basis_dev || !ped[k].basis_exp_sigma_dev) && ped[k].n) MI_FAIL(ctx, MI_EINVAL, "key claim: a null Pedersen array");
    if (!vk->k && vk->n_k) MI_FAIL(ctx, MI_EINVAL, "key claim: vk_desc.k is null");
    mi_key_claim *c = new (std::nothrow) mi_key_claim();
    if (!c) return MI_ENOMEM;
    auto body = [&]() -> int32_t {
        hipStream_t st = ctx->stream;
        c->nb_wires = d->nb_wires;
        c->inf_a.assign(d->infinity_a, d->infinity_a + d->nb_wires);
        c->inf_b.assign(d->infinity_b, d->infinity_b + d->nb_wires);
        c->alpha1 = g1_of(d->alpha1); c->beta1 = g1_of(d->beta1); c->delta1 = g1_of(d->delta1);
        c->beta2 = g2_of(d->beta2); c->delta2 = g2_of(d->delta2);
        c->vk_alpha1 = g1_of(vk->alpha1); c->vk_beta2 = g2_of(vk->beta2); c->vk_gamma2 = g2_of(vk->gamma2); c->vk_delta2 = g2_of(vk->delta2);
        MI_TRY(small_g1(ctx, "desc.alpha1", c->alpha1)); MI_TRY(small_g1(ctx, "desc.beta1", c->beta1)); MI_TRY(small_g1(ctx, "desc.delta1", c->delta1));
        MI_TRY(small_g2(ctx, "desc.beta2", c->beta2)); MI_TRY(small_g2(ctx, "desc.delta2", c->delta2));
        MI_TRY(small_g1(ctx, "vk_desc.alpha1", c->vk_alpha1));
        MI_TRY(small_g2(ctx, "vk_desc.beta2", c->vk_beta2)); MI_TRY(small_g2(ctx, "vk_desc.gamma2", c->vk_gamma2)); MI_TRY(small_g2(ctx, "vk_desc.delta2", c->vk_delta2));
        for (uint32_t k = 0; k < vk->n_commitments; k++) {
            MI_TRY(small_g2(ctx, ("vk_desc.ped[" + std::to_string(k) + "].g").c_str(), g2_of(vk->ped[k].g)));
            MI_TRY(small_g2(ctx, ("vk_desc.ped[" + std::to_string(k) + "].g_sigma_neg").c_str(), g2_of(vk->ped[k].g_sigma_neg)));
            c->vk_ped.push_back(vk->ped[k]);
        }
        auto copy = [&](void **dst, const void *from, size_t bytes, hipMemcpyKind kind) -> int32_t {
            MI_CHECK_HIP(ctx, hipMalloc(dst, bytes ? bytes : 64));
            if (bytes) MI_CHECK_HIP(ctx, hipMemcpyAsync(*dst, from, bytes, kind, st));
            return MI_OK;
        };
        for (int i = 0; i < 5; i++) {
            c->n[i] = src[i].n;
            MI_TRY(copy(&c->arr[i], src[i].p, (size_t)src[i].n * (i == ARR_G2B ? 128 : 64), hipMemcpyDeviceToDevice));
        }
        c->ped.assign(n_ped, mi_key_claim::Ped());
        for (uint32_t k = 0; k < n_ped; k++) {
            c->ped[k].n = ped[k].n;
            MI_TRY(copy(&c->ped[k].basis, ped[k].basis_dev, (size_t)ped[k].n * 64, hipMemcpyDeviceToDevice));
            MI_TRY(copy(&c->ped[k].bes, ped[k].basis_exp_sigma_dev, (size_t)ped[k].n * 64, hipMemcpyDeviceToDevice));
        }
        c->n_vk = vk->n_k;
        MI_TRY(copy(&c->vk_k, vk->k, (size_t)vk->n_k * 64, hipMemcpyHostToDevice));
        std::vector<ClaimArray> arrs = {{"desc.g1_a", false, false, c->arr[ARR_A], c->n[ARR_A]}, {"desc.g1_b", false, false, c->arr[ARR_B], c->n[ARR_B]},
                                        {"desc.g1_k", false, true, c->arr[ARR_K], c->n[ARR_K]}, {"desc.g1_z", false, true, c->arr[ARR_Z], c->n[ARR_Z]},
                                        {"desc.g2_b", true, false, c->arr[ARR_G2B], c->n[ARR_G2B]}, {"vk_desc.k", false, true, c->vk_k, c->n_vk}};
        for (uint32_t k = 0; k < n_ped; k++) {
            arrs.push_back({"ped[" + std::to_string(k) + "].basis_dev", false, true, c->ped[k].basis, c->ped[k].n});
            arrs.push_back({"ped[" + std::to_string(k) + "].basis_exp_sigma_dev", false, true, c->ped[k].bes, c->ped[k].n});
        }
        return check_arrays(ctx, arrs);
    };
    const int32_t rc = body();
    if (rc != MI_OK) { (void)hipStreamSynchronize(ctx->stream); free_claim(c); return rc; }
    *out = c;
    return MI_OK;
}

int32_t mi_key_audit_get_stats(mi_ctx *ctx, mi_key_audit_stats *out) {
    if (!ctx || !out) return MI_EINVAL;
    *out = ctx->key_audit_stats;
    return MI_OK;
}
int32_t mi_debug_key_audit_sums(mi_ctx *ctx, mi_key_audit_sums *out) {
    if (!ctx || !out) return MI_EINVAL;
    if (!ctx->key_audit_sums.valid) MI_FAIL(ctx, MI_EINVAL, "key audit: this context has run no audit as far as its sums");
    *out = ctx->key_audit_sums;
    return MI_OK;
}

int32_t mi_key_audit(mi_ctx *ctx, const mi_r1cs_desc *r1cs, const mi_srs_desc *srs, const mi_phase1 *p1, const mi_key_claim *claim, const uint8_t *seed,
                     uint32_t flags, uint32_t *failed) {
    if (!ctx) return MI_EINVAL;
    if (!failed) MI_FAIL(ctx, MI_EINVAL, "key audit: failed is null");
    if (!r1cs) MI_FAIL(ctx, MI_EINVAL, "key audit: r1cs is null");
    if (!claim) MI_FAIL(ctx, MI_EINVAL, "key audit: the claim is null");
    if (flags & ~MI_KEYFILE_NO_SUBGROUP_CHECK) MI_FAIL(ctx, MI_EINVAL, "key audit: unknown flag");
    if ((srs != nullptr) == (p1 != nullptr)) MI_FAIL(ctx, MI_EINVAL, "key audit: exactly one of srs and p1 is given, not both and not neither");
    R1csShape sh;
    MI_TRY(mi_r1cs_validate(ctx, "key audit", r1cs, sh));
    mi_srs_desc rows;
    if (p1) rows = mi_phase1_rows_desc(p1); else rows = *srs;
    MI_TRY(mi_phase2_srs_host_check(ctx, &rows, sh.N));   // a circuit above a phase-1 state's N is refused as a short row is
    // the claim as it stands now: a borrowed one is read again from its state
    mi_key_claim view;
    const mi_key_claim *c = claim;
    if (claim->borrowed) { MI_TRY(view_state(ctx, claim->borrowed, view)); c = &view; }
    if (c->nb_wires != sh.nb_wires)
        MI_FAIL(ctx, MI_EINVAL, "key audit: claim.nb_wires is " + std::to_string(c->nb_wires) + ", the circuit has " + std::to_string(sh.nb_wires));
    KeyAuditCircuit cs;
    cs.N = sh.N; cs.nb_wires = sh.nb_wires; cs.nb_public = sh.nb_public; cs.n_commitments = sh.n_commitments;
    cs.committed = r1cs->committed; cs.n_committed = r1cs->n_committed; cs.commitment_wire = r1cs->commitment_wire;
    KeyAuditCounts cnt;
    cnt.nb_wires = c->nb_wires; cnt.n_a = c->n[ARR_A]; cnt.n_b = c->n[ARR_B]; cnt.n_g2_b = c->n[ARR_G2B]; cnt.n_k = c->n[ARR_K]; cnt.n_z = c->n[ARR_Z];
    cnt.n_vk = c->n_vk; cnt.n_vk_ped = c->vk_ped.size();
    for (const auto &p : c->ped) cnt.n_basis.push_back(p.n);
    KeyAuditWires w;
    keyaudit_wire_lists(cs, c->inf_a.data(), c->inf_b.data(), w);
    const std::string refusal = keyaudit_shape_refusal(cs, cnt, w);
    if (!refusal.empty()) MI_FAIL(ctx, MI_EINVAL, refusal);
    uint8_t own_seed[32];
    MI_TRY(mi_ceremony_seed_or_random(ctx, "key audit", seed, own_seed));
    const double t0 = now_ms();
    ctx->key_audit_stats = mi_key_audit_stats{};
    ctx->key_audit_sums = mi_key_audit_sums{};
    mi_r1cs *R = nullptr;
    MI_TRY(mi_r1cs_load(ctx, r1cs, &R));
    ctx->key_audit_stats.upload_ms = (float)(now_ms() - t0);
    const AuditIn in{r1cs, &sh, &rows, p1 != nullptr, c, &w, seed, flags};
    int32_t rc;
    size_t peak = 0;
    {
        Arena ar;
        rc = audit_run(ctx, in, R, ar, ctx->key_audit_stats, ctx->key_audit_sums, failed);
        if (rc != MI_OK) (void)hipStreamSynchronize(ctx->stream);
        peak = ar.peak;
    }
    uint64_t r1cs_bytes = 0;
    (void)mi_r1cs_bytes(R, &r1cs_bytes);
    (void)mi_r1cs_free(ctx, R);
    if (rc != MI_OK) return rc;
    ctx->key_audit_stats.peak_bytes = peak + r1cs_bytes;
    ctx->key_audit_stats.total_ms = (float)(now_ms() - t0);
    return MI_OK;
}

}  // extern "C"

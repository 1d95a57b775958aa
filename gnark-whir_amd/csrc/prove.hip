// Proving key residency and the fused prove path: everything groth16.Prove does after the solve
// (gnark v0.11.0 backend/groth16/bn254/prove.go, reached from /root/reference/mt.go:496; SURVEY.md
// section 3.3 steps 4-8, 8a rows a7 and a9).
//
//   mi_pk_load   uploads pk.G1.{A,B,K,Z}, pk.G2.B once and turns the static masks pk.InfinityA/B and the
//                public / committed wire sets into device gather-index arrays (row a7).
//   prove        computeH on the device -> three gathers of W -> five MSMs -> O(1)-point blinding and
//                assembly on the host (Ar, Bs1, Krs, Bs exactly as prove.go composes them).
#include "prove_internal.h"
#include "r1cs_internal.h"
#include <cstring>
#include <vector>
#include <chrono>
#include <cstdlib>

__global__ void k_expand_points(G1Aff *full, const G1Aff *compact, const u32 *idx, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) full[idx[i]] = compact[i];
}
__global__ void k_gather_fr(Fr *out, const Fr *W, const u32 *idx, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = W[idx[i]];
}

static size_t point_bytes(int curve) { return curve == 1 ? sizeof(G1Aff) : sizeof(G2Aff); }
static int32_t upload(mi_ctx *ctx, void **dst, const void *src, size_t bytes) {
    MI_CHECK_HIP(ctx, hipMalloc(dst, bytes ? bytes : 32));
    if (bytes) MI_CHECK_HIP(ctx, hipMemcpyAsync(*dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return MI_OK;
}

// ---------------------------------------------------------------- mi_pk_load_range, step by step
// 1: the header, and the range this load covers (the whole key without sr; slices, mi_pk_load_sharded_dev: the arrays ARE this part's slices,
// counts = points of the slice).  Step 2 is wire_indices (key_plan.h).
static int32_t check_header(mi_ctx *ctx, const mi_pk_desc *d, bool slices, const ShardRange *sr, ShardRange *r) {
    if (d->log_n > 28 || d->nb_public > d->nb_wires || !d->infinity_a || !d->infinity_b) MI_FAIL(ctx, MI_EINVAL, "pk: bad header");
    const u64 N = (u64)1 << d->log_n;
    if (!slices && d->n_g1_z + 1 < N) MI_FAIL(ctx, MI_EINVAL, "pk: G1.Z needs at least 2^log_n - 1 points");
    if (d->nb_wires >= ((u64)1 << 31)) MI_FAIL(ctx, MI_EINVAL, "pk: too many wires");
    if (d->n_g2_b != d->n_g1_b) MI_FAIL(ctx, MI_EINVAL, "pk: G1.B and G2.B differ in length");
    *r = sr ? *sr : ShardRange{0, d->nb_wires, 0, N - 1};
    if (r->w_lo > r->w_hi || r->w_hi > d->nb_wires || r->z_lo > r->z_hi || r->z_hi > N - 1) MI_FAIL(ctx, MI_EINVAL, "pk: bad shard range");
    // one device runs every MSM of its part, and a single-device MSM takes at most 2^27 pairs (mi_msm_enqueue): A and K run over the
    // part's wires, B over a subset of them, Z over its Z range.  Refused here, before anything is allocated or enqueued.
    if (r->w_hi - r->w_lo > MI_MSM_MAX_PAIRS || r->z_hi - r->z_lo > MI_MSM_MAX_PAIRS)
        MI_FAIL(ctx, MI_EINVAL, "pk: a per-device MSM would exceed 2^27 pairs (log_n = 28, or more than 2^27 wires on one device): "
                                "load the key with mi_pk_load_sharded over enough devices");
    return MI_OK;
}
// 3: the point arrays in the order of their uploads -- this range's share of the host arrays, or the device arrays as they stand, the
// key's own from here on when it adopts them -- and the index arrays of A, B, K
enum { ARR_A, ARR_B1, ARR_K, ARR_Z, ARR_B2 };
static int32_t take_arrays(mi_ctx *ctx, mi_pk *pk, const mi_pk_desc *d, const WireIndices &wi, u64 n_z, bool device_points, bool adopt, void *arr[5], u32 *idx[3]) {
    const void *given[5] = {d->g1_a, d->g1_b, d->g1_k, d->g1_z, d->g2_b};
    const u64 first[5] = {wi.a0, wi.b0, wi.k0, pk->z_lo, wi.b0}, n[5] = {wi.a.size(), wi.b.size(), wi.k.size(), n_z, wi.b.size()};
    // an upload is the key's from its allocation on: a failing copy leaves it to mi_pk_free
    auto key_upload = [&](void **dst, const void *src, size_t bytes, int kind) { const int32_t rc = upload(ctx, dst, src, bytes); if (*dst) pk->own(*dst, bytes, kind); return rc; };
    for (int i = 0; i < 5; i++) {
        const size_t size = point_bytes(i == ARR_B2 ? 2 : 1);
        if (!device_points) MI_TRY(key_upload(&arr[i], (const char *)given[i] + first[i] * size, n[i] * size, KEY_MEM_BASES));
        else { arr[i] = (void *)given[i]; if (adopt) pk->own(arr[i], n[i] * size, KEY_MEM_BASES); }
    }
    const std::vector<u32> *wires[3] = {&wi.a, &wi.b, &wi.k};
    for (int i = 0; i < 3; i++) MI_TRY(key_upload((void **)&idx[i], wires[i]->data(), wires[i]->size() * 4, KEY_MEM_INDICES));
    return MI_OK;
}
// 4: pk.G1.A / pk.G1.K with one slot per wire of the range
static int32_t expand_per_wire(mi_ctx *ctx, mi_pk *pk, void **full, const void *compact, const u32 *idx, size_t n) {
    const size_t bytes = (size_t)pk->nb_wires * sizeof(G1Aff);
    MI_CHECK_HIP(ctx, hipMalloc(full, bytes ? bytes : 64));
    pk->own(*full, bytes, KEY_MEM_BASES);
    MI_CHECK_HIP(ctx, hipMemsetAsync(*full, 0, bytes, ctx->stream));
    if (n) hipLaunchKernelGGL(k_expand_points, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (G1Aff *)*full, (const G1Aff *)compact, idx, n);
    MI_CHECK_HIP(ctx, hipGetLastError());
    return MI_OK;
}
// 5: the table plan.  The key's own: fixed_base_plan over a third of the device memory that is free NOW, after the uploads and the
// expansions (the rest stays for the contexts' workspaces).  forced: that plan, except for the groups whose knob the caller set.
static void plan_tables(mi_ctx *ctx, mi_pk *pk, const FixedBasePlan *forced) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
    const FixedBasePlan own = fixed_base_plan(ctx->fixed_knob, free_b / 3, pk->group[KEY_AK].n, pk->group[KEY_B].n, pk->group[KEY_Z].n);
    for (int g = 0; g < 3; g++) pk->group[g].c = forced && !ctx->fixed_knob[g] ? forced->c[g] : own.c[g];
}
// 6: the tables of one group from its plain bases; without room for them after all (the budget is an estimate) the group stays generic
static int32_t build_table(mi_ctx *ctx, mi_pk *pk, void **table, const void *plain, size_t n, int curve, u32 c) {
    const size_t bytes = msm_nwin(c) * n * point_bytes(curve);
    MI_CHECK_HIP(ctx, hipMalloc(table, bytes ? bytes : 64));
    pk->own(*table, bytes, KEY_MEM_TABLES);
    return mi_msm_precompute(ctx, curve, plain, *table, n, c);
}
static int32_t build_tables(mi_ctx *ctx, mi_pk *pk, int g, void *const plain[2]) {
    KeyGroup &G = pk->group[g];
    void *t[2] = {nullptr, nullptr};
    int32_t rc = MI_OK;
    for (int i = 0; i < KEY_GROUP_MSMS[g] && G.c && rc == MI_OK; i++) rc = build_table(ctx, pk, &t[i], plain[i], G.n, KEY_GROUP_CURVE[g][i], G.c);
    if (rc == MI_ENOMEM) { (void)hipGetLastError(); pk->drop(t[0]); pk->drop(t[1]); G.c = 0; rc = MI_OK; }
    for (int i = 0; i < KEY_GROUP_MSMS[g]; i++) G.bases[i].pts = G.c ? t[i] : plain[i];
    return rc;
}
// 8: what the level-1 accumulation gathers from goes into the R' packed form: in place where the array is the key's own (tables, the
// per-wire copies, uploaded or adopted bases), into a converted copy of the key's where it is the caller's
static int32_t to_rprime_form(mi_ctx *ctx, mi_pk *pk, bool arrays_mine) {
    for (int g = 0; g < 3; g++) for (int i = 0; i < KEY_GROUP_MSMS[g]; i++) {
        KeyGroup &G = pk->group[g];
        const int curve = KEY_GROUP_CURVE[g][i];
        const size_t n = (G.c ? msm_nwin(G.c) : 1) * G.n, bytes = n * point_bytes(curve);
        const bool in_place = G.c || g == KEY_AK || arrays_mine;
        void *src = G.bases[i].pts, *dst = in_place ? src : nullptr;
        if (!src || !n) continue;
        if (!in_place) {
            if (curve == 1) MI_CHECK_HIP(ctx, hipMalloc(&dst, bytes));
            else if (hipMalloc(&dst, bytes) != hipSuccess) { (void)hipGetLastError(); MI_FAIL(ctx, MI_ENOMEM, "pk: no room for the converted copy of pk.G2.B"); }
            pk->own(dst, bytes, KEY_MEM_BASES);
        }
        mi_msm_ops(curve).to_rprime(ctx->stream, dst, src, n);
        G.bases[i].pts = dst;
    }
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) MI_FAIL(ctx, MI_EHIP, "pk: conversion of the G1 arrays failed");
    pk->rprime = true;
    return MI_OK;
}
// steps 3 to 8 on the key under construction: whatever fails, the caller frees the key and with it all it owns by then
static int32_t fill_key(mi_ctx *ctx, mi_pk *pk, const mi_pk_desc *d, const WireIndices &wi, u64 n_z, bool device_points, const FixedBasePlan *forced, bool adopt) {
    const bool mine = !device_points || adopt;   // the five arrays are the key's, not the caller's
    void *arr[5] = {}, *a_full = nullptr, *k_full = nullptr;
    u32 *idx[3] = {};
    MI_TRY(take_arrays(ctx, pk, d, wi, n_z, device_points, adopt, arr, idx));
    pk->idx_b = idx[1];
    MI_TRY(expand_per_wire(ctx, pk, &a_full, arr[ARR_A], idx[0], wi.a.size()));
    MI_TRY(expand_per_wire(ctx, pk, &k_full, arr[ARR_K], idx[2], wi.k.size()));
    void *const plain[3][2] = {{a_full, k_full}, {arr[ARR_B1], arr[ARR_B2]}, {arr[ARR_Z], nullptr}};
    plan_tables(ctx, pk, forced);
    for (int g : {KEY_Z, KEY_B, KEY_AK}) MI_TRY(build_tables(ctx, pk, g, plain[g]));
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) MI_FAIL(ctx, MI_EHIP, "pk upload sync failed");
    // 7: the compact A and K are not needed any more when they are the key's; nor are plain bases of the key's that have tables
    if (mine) { pk->drop(arr[ARR_A]); pk->drop(arr[ARR_K]); }
    for (int g = 0; g < 3; g++) for (int i = 0; i < KEY_GROUP_MSMS[g]; i++) if (pk->group[g].c && (g == KEY_AK || mine)) pk->drop(plain[g][i]);
    return mi_msm_limb29_enabled(ctx) ? to_rprime_form(ctx, pk, mine) : MI_OK;
}
int32_t mi_pk_load_range(mi_ctx *ctx, const mi_pk_desc *d, mi_pk **out, bool device_points, const ShardRange *sr, const FixedBasePlan *forced,
                         bool adopt, bool *took_arrays) {
    if (took_arrays) *took_arrays = false;
    if (!ctx || !d || !out) return MI_EINVAL;
    *out = nullptr;
    const bool slices = sr && device_points;
    ShardRange r;
    MI_TRY(check_header(ctx, d, slices, sr, &r));
    const WireIndices wi = wire_indices(d->infinity_a, d->infinity_b, d->nb_wires, d->nb_public, d->committed_wires, d->n_committed, r.w_lo, r.w_hi);
    if (slices && (wi.a.size() != d->n_g1_a || wi.b.size() != d->n_g1_b || wi.k.size() != d->n_g1_k || d->n_g1_z < r.z_hi - r.z_lo))
        MI_FAIL(ctx, MI_EINVAL, "pk: slice point counts do not match the infinity masks / public / committed wire sets of this rank's wire range");
    if (!slices && (wi.n_a != d->n_g1_a || wi.n_b != d->n_g1_b || wi.n_k != d->n_g1_k))
        MI_FAIL(ctx, MI_EINVAL, "pk: point counts do not match the infinity masks / public / committed wire sets");
    mi_pk *pk = new (std::nothrow) mi_pk();
    if (!pk) return MI_ENOMEM;
    pk->log_n = d->log_n; pk->nb_wires = r.w_hi - r.w_lo;
    pk->nb_public = (u32)(d->nb_public <= r.w_lo ? 0 : (d->nb_public >= r.w_hi ? r.w_hi - r.w_lo : d->nb_public - r.w_lo));
    pk->wire_lo = r.w_lo; pk->z_lo = r.z_lo; pk->n_z_msm = r.z_hi - r.z_lo;
    pk->group[KEY_AK].n = pk->nb_wires; pk->group[KEY_B].n = wi.b.size(); pk->group[KEY_Z].n = pk->n_z_msm;
    pk->group[KEY_AK].bases[0].stat_pairs = wi.a.size(); pk->group[KEY_AK].bases[1].stat_pairs = wi.k.size();
    std::memcpy(&pk->alpha1, &d->alpha1, 64); std::memcpy(&pk->beta1, &d->beta1, 64); std::memcpy(&pk->delta1, &d->delta1, 64);
    std::memcpy(&pk->beta2, &d->beta2, 128); std::memcpy(&pk->delta2, &d->delta2, 128);
    // adopt: from here on the arrays are the key's, on success AND on every failure path (mi_pk_free releases what is still there)
    if (device_points && adopt && took_arrays) *took_arrays = true;
    const int32_t rc = fill_key(ctx, pk, d, wi, sr ? pk->n_z_msm : d->n_g1_z, device_points, forced, adopt);   // (Z of a whole key: every point given)
    if (rc == MI_OK) *out = pk; else mi_pk_free(ctx, pk);
    return rc;
}

// k * p on the host, k canonical 8 x u32
template <class F>
static XYZZ<F> host_scalar_mul(const Affine<F> &p, const Fr &k_canon) { return xyzz_mul_256(XYZZ<F>::from_affine(p), k_canon.l); }

// ---------------------------------------------------------------- BSB22 Pedersen key
struct mi_pedersen_pk {
    void *basis = nullptr, *basis_exp_sigma = nullptr;
    size_t n = 0;
    // fixed-base window tables of both arrays (as for pk.G1.*: ONE bucket set for all windows, the level-1 additions in 29-bit limbs over
    // the R' form) when the key has >= 2^15 points and they fit: a commitment over 2^18 WHIR-mix values is then 15 windows into 2^16 buckets
    // instead of 19 windows x 2^13 -- the bucket reduce of the generic plan was most of what a Pedersen MSM cost a busy GPU (r4: 3.5 % of
    // the proofs/s at 2^18 committed wires, 8.6 % at 2^20)
    void *pre_basis = nullptr, *pre_sigma = nullptr;
    u32 c_tab = 0;
};
static constexpr u32 PEDERSEN_TABLE_C = 17;
// best effort: without room (or below 2^15 points) the key stays on the generic path
static void pedersen_build_tables(mi_ctx *ctx, mi_pedersen_pk *pk) {
    if (pk->n < ((size_t)1 << 15) || !mi_msm_limb29_enabled(ctx)) return;
    const u32 c = PEDERSEN_TABLE_C;
    const size_t nwin = msm_nwin(c), bytes = nwin * pk->n * sizeof(G1Aff);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || 2 * bytes > free_b / 4) { (void)hipGetLastError(); return; }
    void *t[2] = {nullptr, nullptr};
    const void *src[2] = {pk->basis, pk->basis_exp_sigma};
    bool ok = true;
    for (int k = 0; k < 2 && ok; k++) {
        ok = hipMalloc(&t[k], bytes) == hipSuccess && mi_msm_precompute(ctx, 1, src[k], t[k], pk->n, c) == MI_OK;
        if (ok) mi_msm_ops(1).to_rprime(ctx->stream, t[k], t[k], nwin * pk->n);
    }
    if (ok) ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(ctx->stream) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); for (void *q : t) if (q) (void)hipFree(q); return; }
    pk->pre_basis = t[0]; pk->pre_sigma = t[1]; pk->c_tab = c;
}
// One Pedersen MSM on MSM_SLOT_POK of ctx (its own stream: it runs beside the five MSMs of a proof), in two halves so that a prover-pool job
// can enqueue its proof's ProveKnowledge MSM, prove, and collect (pool.hip); host values in, affine point out.
static int32_t pedersen_enqueue(mi_ctx *ctx, const void *bases_dev, const void *tables_dev, u32 c_tab, size_t key_n, const mi_fr *values, size_t n) {
    if (!ctx || (!values && n)) return MI_EINVAL;
    if (n > key_n) MI_FAIL(ctx, MI_EINVAL, "pedersen: more values than basis points");   // gnark: "must have as many values as basis elements"
    MI_TRY(mi_reserve(ctx, ctx->ws[WS_POK_VALUES], n * sizeof(mi_fr) + 64));
    if (n) MI_CHECK_HIP(ctx, hipMemcpyAsync(ctx->ws[WS_POK_VALUES].p, values, n * sizeof(mi_fr), hipMemcpyHostToDevice, ctx->msm[MSM_SLOT_POK].stream));
    // the tables are laid out [window][key_n]: they serve exactly the full-length call (gnark's: as many values as basis elements)
    if (tables_dev && n == key_n) return mi_msm_enqueue(ctx, MSM_SLOT_POK, -1, 1, tables_dev, ctx->ws[WS_POK_VALUES].p, n, MI_MSM_PTS_RPRIME, nullptr, false, c_tab);
    return mi_msm_enqueue(ctx, MSM_SLOT_POK, -1, 1, bases_dev, ctx->ws[WS_POK_VALUES].p, n, 0, nullptr, false);
}
static int32_t pedersen_collect(mi_ctx *ctx, mi_g1_affine *out) {
    G1X r;
    MI_TRY(mi_msm_finish(ctx, MSM_SLOT_POK, 1, &r));
    G1Aff a = xyzz_to_affine(r);
    if (out) std::memcpy(out, &a, sizeof(a));
    return MI_OK;
}
static int32_t pedersen_msm(mi_ctx *ctx, const mi_pedersen_pk *pk, bool sigma, const mi_fr *values, size_t n, mi_g1_affine *out) {
    if (!out) return MI_EINVAL;
    MI_TRY(pedersen_enqueue(ctx, sigma ? pk->basis_exp_sigma : pk->basis, sigma ? pk->pre_sigma : pk->pre_basis, pk->c_tab, pk->n, values, n));
    return pedersen_collect(ctx, out);
}
int32_t mi_pedersen_pok_enqueue(mi_ctx *ctx, mi_pedersen_pk *pk, const mi_fr *values, size_t n) {
    if (!pk) return MI_EINVAL;
    return pedersen_enqueue(ctx, pk->basis_exp_sigma, pk->pre_sigma, pk->c_tab, pk->n, values, n);
}
int32_t mi_pedersen_pok_collect(mi_ctx *ctx, mi_g1_affine *pok) { return pedersen_collect(ctx, pok); }

extern "C" {
int32_t mi_pedersen_pk_load(mi_ctx *ctx, const mi_g1_affine *basis, const mi_g1_affine *basis_exp_sigma, size_t n, mi_pedersen_pk **out) {
    if (!ctx || !out || ((!basis || !basis_exp_sigma) && n)) return MI_EINVAL;
    *out = nullptr;
    mi_pedersen_pk *pk = new (std::nothrow) mi_pedersen_pk();
    if (!pk) return MI_ENOMEM;
    pk->n = n;
    int32_t rc = upload(ctx, &pk->basis, basis, n * 64);
    if (rc == MI_OK) rc = upload(ctx, &pk->basis_exp_sigma, basis_exp_sigma, n * 64);
    if (rc == MI_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) { mi_set_err(ctx, "pedersen key upload failed"); rc = MI_EHIP; }
    if (rc != MI_OK) { mi_pedersen_pk_free(ctx, pk); return rc; }
    pedersen_build_tables(ctx, pk);
    *out = pk;
    return MI_OK;
}
int32_t mi_pedersen_pk_adopt(mi_ctx *ctx, void *basis_dev, void *basis_exp_sigma_dev, size_t n, mi_pedersen_pk **out) {
    if (!ctx || !out) return MI_EINVAL;
    mi_pedersen_pk *pk = new (std::nothrow) mi_pedersen_pk();
    if (!pk) return MI_ENOMEM;
    pk->basis = basis_dev; pk->basis_exp_sigma = basis_exp_sigma_dev; pk->n = n;
    pedersen_build_tables(ctx, pk);
    *out = pk;
    return MI_OK;
}
int32_t mi_pedersen_pk_free(mi_ctx *ctx, mi_pedersen_pk *pk) {
    if (!ctx || !pk) return MI_EINVAL;
    (void)hipStreamSynchronize(ctx->stream);
    for (void *q : {pk->basis, pk->basis_exp_sigma, pk->pre_basis, pk->pre_sigma}) if (q) (void)hipFree(q);
    delete pk;
    return MI_OK;
}
int32_t mi_pedersen_commit(mi_ctx *ctx, mi_pedersen_pk *pk, const mi_fr *values, size_t n, mi_g1_affine *commitment) {
    if (!pk) return MI_EINVAL;
    return pedersen_msm(ctx, pk, false, values, n, commitment);
}
int32_t mi_pedersen_prove_knowledge(mi_ctx *ctx, mi_pedersen_pk *pk, const mi_fr *values, size_t n, mi_g1_affine *pok) {
    if (!pk) return MI_EINVAL;
    return pedersen_msm(ctx, pk, true, values, n, pok);
}
// sum_i challenge^i * points[i] on the host (a handful of points: one per commitment)
int32_t mi_pedersen_fold(const mi_g1_affine *points, size_t n, const mi_fr *challenge, mi_g1_affine *out) {
    if ((!points && n) || !challenge || !out) return MI_EINVAL;
    Fr ch, pw = Fr::one();
    std::memcpy(&ch, challenge, 32);
    G1X acc = G1X::inf();
    for (size_t i = 0; i < n; i++) {
        G1Aff p;
        std::memcpy(&p, &points[i], sizeof(p));
        G1X t = i ? host_scalar_mul<Fp>(p, fe_from_mont(pw)) : G1X::from_affine(p);   // challenge^0 = 1: no 256-bit ladder for the first (usually only) point
        xyzz_add(acc, t);
        pw = pw * ch;
    }
    if (n == 1) { std::memcpy(out, &points[0], sizeof(*out)); return MI_OK; }   // one commitment: the fold is the point itself, bit for bit
    G1Aff a = xyzz_to_affine(acc);
    std::memcpy(out, &a, sizeof(a));
    return MI_OK;
}
int32_t mi_get_mem_ledger(mi_ctx *ctx, const mi_pk *pk, mi_mem_ledger *out) {
    if (!ctx || !out) return MI_EINVAL;
    std::memset(out, 0, sizeof(*out));
    if (pk) { out->key_bases = pk->mem[KEY_MEM_BASES]; out->key_tables = pk->mem[KEY_MEM_TABLES]; out->key_indices = pk->mem[KEY_MEM_INDICES]; }
    out->ctx_ntt_tables = mi_ntt_table_bytes(ctx);
    for (int i = 0; i < WS_COUNT; i++) {
        const size_t cap = ctx->ws[i].cap;
        if (i == WS_H_B || i == WS_H_C || i == WS_H) out->ctx_ntt_vectors += cap; else out->ctx_other += cap;
    }
    for (const auto &sl : ctx->msm) for (const auto &b : sl.buf) out->ctx_msm += b.cap;
    return MI_OK;
}
int32_t mi_pk_table_plan(const mi_pk *pk, uint32_t c_out[3]) {
    if (!pk || !c_out) return MI_EINVAL;
    for (int g = 0; g < 3; g++) c_out[g] = pk->group[g].c;
    return MI_OK;
}
int32_t mi_pk_load(mi_ctx *ctx, const mi_pk_desc *d, mi_pk **out) {
    if (d && (!d->g1_a && d->n_g1_a)) return MI_EINVAL;
    return mi_pk_load_range(ctx, d, out, false, nullptr);
}
int32_t mi_pk_load_dev(mi_ctx *ctx, const mi_pk_desc *d, mi_pk **out) { return mi_pk_load_range(ctx, d, out, true, nullptr); }
int32_t mi_pk_free(mi_ctx *ctx, mi_pk *pk) {
    if (!ctx || !pk) return MI_EINVAL;
    (void)hipStreamSynchronize(ctx->stream);
    for (const mi_pk::Alloc &a : pk->owned) if (a.p) (void)hipFree(a.p);
    delete pk;
    return MI_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- the pieces of a proof (shared with group.hip)
// step 5 + the wire MSMs: they depend on W only (ev_w = "W is on the device").  Two independent groups, each with ONE sort:
// B1 + B2 and A + K.  Enqueueing a group waits once, on the host, for the count pass of its sort (msm.hip,
// MI_MSM_EXACT_SIZE), so a proof enqueues the two groups from two helper threads while its own thread enqueues computeH and the Z MSM
// (prove_common): measured on one proof alone, the A + K sort used to start 10 ms into the proof because the host was still busy
// enqueueing Z's and B's ~130 launches, and the memory-bound sorts then ran beside the bucket accumulations instead of beside the NTT.
static void arm_accum_gate(mi_ctx *ctx, int slot, const std::function<hipEvent_t()> *accum_gate) { ctx->msm[slot].accum_gate = accum_gate; }
static int32_t enqueue_b_msms(mi_ctx *ctx, mi_pk *pk, const mi_fr *W, hipEvent_t ev_w, bool defer, const std::function<hipEvent_t()> *accum_gate) {
    (void)hipSetDevice(ctx->dev);   // the current device is per host thread
    // wire values are skewed (45 % of them 0 or 1): their sorts are sized by the counted entries, not by windows * n (msm.hip)
    const uint32_t fl = (defer ? MI_MSM_DEFER_REDUCE : 0) | MI_MSM_EXACT_SIZE | (pk->rprime ? MI_MSM_PTS_RPRIME : 0);
    // wireValuesB by the static gather indices, on its MSM's stream; B2 (G2) shares B1's sort (same scalars)
    const KeyGroup &B = pk->group[KEY_B];
    MI_TRY(mi_reserve(ctx, ctx->ws[WS_B_WIRES], (B.n + 1) * sizeof(Fr)));
    hipStream_t st = ctx->msm[MSM_SLOT_B1].stream;
    if (ev_w) MI_CHECK_HIP(ctx, hipStreamWaitEvent(st, ev_w, 0));
    if (B.n) hipLaunchKernelGGL(k_gather_fr, dim3((unsigned)((B.n + 255) / 256)), dim3(256), 0, st, (Fr *)ctx->ws[WS_B_WIRES].p, (const Fr *)W, pk->idx_b, B.n);
    MI_CHECK_HIP(ctx, hipGetLastError());
    // the group's record says which: fixed-base tables, or the plain bases with the window bits the parts of a sharded key agree on
    arm_accum_gate(ctx, MSM_SLOT_B1, accum_gate);
    // (B1 and K are not timed: their chains interleave on one stream, so the event pair around one's level-1 launch may bracket kernels
    //  of the other; mi_stats.g1_accum_* then cover A and Z, the two launches with a stream of their own)
    MI_TRY(mi_msm_enqueue(ctx, MSM_SLOT_B1, -1, 1, B.bases[0].pts, ctx->ws[WS_B_WIRES].p, B.n, fl, nullptr, false, B.c, B.bases[0].stat_pairs, B.gen_c));
    arm_accum_gate(ctx, MSM_SLOT_B2, accum_gate);
    return mi_msm_enqueue(ctx, MSM_SLOT_B2, MSM_SLOT_B1, 2, B.bases[1].pts, nullptr, B.n, fl, nullptr, false, B.c, B.bases[1].stat_pairs);
}
static int32_t enqueue_ak_msms(mi_ctx *ctx, mi_pk *pk, const mi_fr *W, hipEvent_t ev_w, bool defer, const std::function<hipEvent_t()> *accum_gate) {
    (void)hipSetDevice(ctx->dev);
    const uint32_t fl = (defer ? MI_MSM_DEFER_REDUCE : 0) | MI_MSM_EXACT_SIZE | (pk->rprime ? MI_MSM_PTS_RPRIME : 0);
    // A and K are both multiplied by W itself: one sort of all wires (A's slot) serves both, against the per-wire expanded
    // point arrays (a wire without a point reads (0,0) = infinity and is skipped); no gather, one sort less
    const KeyGroup &AK = pk->group[KEY_AK];
    arm_accum_gate(ctx, MSM_SLOT_A, accum_gate);
    MI_TRY(mi_msm_enqueue(ctx, MSM_SLOT_A, -1, 1, AK.bases[0].pts, W, AK.n, fl, ev_w, true, AK.c, AK.bases[0].stat_pairs, AK.gen_c));
    arm_accum_gate(ctx, MSM_SLOT_K, accum_gate);
    return mi_msm_enqueue(ctx, MSM_SLOT_K, MSM_SLOT_A, 1, AK.bases[1].pts, nullptr, AK.n, fl, nullptr, false, AK.c, AK.bases[1].stat_pairs);   // (not timed: K and B1 share a stream, msm.hip)
}
void WireMsms::start(mi_ctx *ctx, mi_pk *pk, const mi_fr *W, hipEvent_t ev_w, bool defer, const std::function<hipEvent_t()> *accum_gate) {
    auto group = [&](std::future<int32_t> &f, int32_t (*enqueue)(mi_ctx *, mi_pk *, const mi_fr *, hipEvent_t, bool, const std::function<hipEvent_t()> *)) {
        try {
            f = std::async(std::launch::async, [=]() -> int32_t { try { return enqueue(ctx, pk, W, ev_w, defer, accum_gate); } catch (...) { return MI_ENOMEM; } });
        } catch (...) {   // no thread to be had: this thread does it (without the gate: it would wait for itself); no exception crosses the C-ABI
            int32_t r = MI_ENOMEM;
            try { r = enqueue(ctx, pk, W, ev_w, defer, nullptr); } catch (...) {}
            if (rc_inline == MI_OK) rc_inline = r;
        }
    };
    group(f_b, enqueue_b_msms);
    group(f_ak, enqueue_ak_msms);
}
int32_t WireMsms::join() {
    int32_t rc = rc_inline;
    for (std::future<int32_t> *f : {&f_b, &f_ak})
        if (f->valid()) { const int32_t r = f->get(); if (rc == MI_OK) rc = r; }
    return rc;
}
int32_t mi_prove_enqueue_wire_msms(mi_ctx *ctx, mi_pk *pk, const mi_fr *W, hipEvent_t ev_w, bool defer) {
    WireMsms wires;
    wires.start(ctx, pk, W, ev_w, defer, nullptr);
    return wires.join();
}
// the Z MSM over this key's h coefficients against the bit-reversed pk.G1.Z (ev_h = "h is ready")
int32_t mi_prove_enqueue_z_msm(mi_ctx *ctx, mi_pk *pk, const mi_fr *h, hipEvent_t ev_h, bool defer) {
    const uint32_t fl = (defer ? MI_MSM_DEFER_REDUCE : 0) | (pk->rprime ? MI_MSM_PTS_RPRIME : 0);
    const KeyGroup &Z = pk->group[KEY_Z];
    return mi_msm_enqueue(ctx, MSM_SLOT_Z, -1, 1, Z.bases[0].pts, h, Z.n, fl, ev_h, true, Z.c, Z.bases[0].stat_pairs, Z.gen_c);
}

// a host helper thread for one independent scalar multiplication; without a thread to be had the work runs here (no exception may
// cross the C-ABI: std::async throws std::system_error when the process is out of threads)
template <class Fn>
static auto async_or_inline(Fn fn) -> std::future<decltype(fn())> {
    try {
        return std::async(std::launch::async, fn);
    } catch (...) {
        std::promise<decltype(fn())> p;
        p.set_value(fn());
        return p.get_future();
    }
}
void ProofAssembler::start(const mi_pk *pk_, const mi_fr *r_m, const mi_fr *s_m) {
    pk = pk_;
    Fr r, s;
    std::memcpy(&r, r_m, 32); std::memcpy(&s, s_m, 32);
    rc = fe_from_mont(r); sc = fe_from_mont(s); krc = fe_from_mont(fe_neg(r * s));
    // (independent 256-bit scalar multiplications: one host thread each; for small circuits they are the longest chain)
    f_r = async_or_inline([this] { return host_scalar_mul<Fp>(pk->delta1, rc); });
    f_s = async_or_inline([this] { return host_scalar_mul<Fp>(pk->delta1, sc); });
    f_kr = async_or_inline([this] { return host_scalar_mul<Fp>(pk->delta1, krc); });
    s_delta2 = host_scalar_mul<Fp2>(pk->delta2, sc);
    r_delta = f_r.get(); s_delta = f_s.get(); kr_delta = f_kr.get();
}
void ProofAssembler::have_a_b1(const G1X &msm_a, const G1X &msm_b1) {
    G1X ar = msm_a;
    xyzz_madd(ar, pk->alpha1, false);
    xyzz_add(ar, r_delta);
    G1X bs1 = msm_b1;
    xyzz_madd(bs1, pk->beta1, false);
    xyzz_add(bs1, s_delta);
    ar_aff = xyzz_to_affine(ar); bs1_aff = xyzz_to_affine(bs1);
    f_sar = async_or_inline([this] { return host_scalar_mul<Fp>(ar_aff, sc); });   // overlaps the remaining MSMs
    r_bs1 = host_scalar_mul<Fp>(bs1_aff, rc);
}
void ProofAssembler::finish(const G1X &msm_k, const G2X &msm_b2, const G1X &msm_z, mi_proof_out *out) {
    G1X s_ar = f_sar.get();
    G1X krs = msm_k;
    xyzz_add(krs, msm_z);
    xyzz_add(krs, kr_delta);
    xyzz_add(krs, s_ar);
    xyzz_add(krs, r_bs1);
    G2X bs = msm_b2;
    xyzz_madd(bs, pk->beta2, false);
    xyzz_add(bs, s_delta2);
    G1Aff krs_aff = xyzz_to_affine(krs);
    G2Aff bs_aff = xyzz_to_affine(bs);
    std::memcpy(&out->ar, &ar_aff, 64); std::memcpy(&out->bs, &bs_aff, 128); std::memcpy(&out->krs, &krs_aff, 64);
}

// Host-pointer inputs of mi_groth16_prove (null for the device-pointer entry point).
struct HostInputs { const mi_fr *W, *a, *b, *c; };
// Device inputs that are still ARRIVING (the prover pool's upload stage, pool.hip): W is resident when the call is made; abc() blocks
// the host until a, b, c are resident too and returns true (false: their upload failed).  Host-side waits on purpose: events recorded
// on the pool's copy stream between its pageable copies slowed those copies down (round 3: uploads of 50-70 ms instead of 19).
// Proving from W alone (mi_groth16_prove_w*): a = A W and b = B W (and c = C W with eval_c) come from the resident R1CS, evaluated into
// context workspace on the context's stream; a, b, c of prove_common are ignored.
struct WEval { const mi_r1cs *r1cs; bool eval_c; };
struct AbcGate { const std::function<bool(int)> *abc; /* abc(k): blocks until k of a, b, c are resident */ bool abc_arrived; /* they all were when the job was picked up */ };

// what every prove entry point refuses about the key before anything is enqueued
static int32_t check_key_fits(mi_ctx *ctx, const mi_pk *pk, size_t n_wires) {
    if (pk->wire_lo || pk->n_z_msm != ((u64)1 << pk->log_n) - 1) MI_FAIL(ctx, MI_EINVAL, "prove: this key is one part of a sharded key (use mi_groth16_prove_sharded)");
    if (n_wires != pk->nb_wires) MI_FAIL(ctx, MI_EINVAL, "prove: witness size (n_wires) does not match the proving key");
    return MI_OK;
}

// W, a, b, c: device buffers (for host inputs: staging areas the uploads below fill).
static int32_t prove_common(mi_ctx *ctx, mi_pk *pk, const mi_fr *W, size_t n_wires, const mi_fr *a, const mi_fr *b, const mi_fr *c,
                            size_t n_constraints, const mi_fr *r_m, const mi_fr *s_m, mi_proof_out *out, mi_stats *stats, const HostInputs *host,
                            const AbcGate *gate = nullptr, const WEval *weval = nullptr) {
    if (!ctx || !pk || !r_m || !s_m || !out) return MI_EINVAL;
    const MiRange range_all("mi.prove");
    if (weval) n_constraints = weval->r1cs->nc;   // a, b, c are not given: the evaluation below produces them
    // null W / a / b only where the matching count is 0 (the header's rule, as the pool's submit applies it); c == null: c = a o b on the device
    if ((!W && n_wires) || (!weval && (!a || !b) && n_constraints)) MI_FAIL(ctx, MI_EINVAL, "prove: null W, a or b with a non-zero count");
    if (host && ((!host->W && n_wires) || (!weval && (!host->a || !host->b) && n_constraints))) MI_FAIL(ctx, MI_EINVAL, "prove: null host W, a or b with a non-zero count");
    const bool derive_c = weval ? !weval->eval_c : host ? !host->c : !c;
    const size_t N = (size_t)1 << pk->log_n;
    MI_TRY(check_key_fits(ctx, pk, n_wires));   // (the W-only entry points have asked already, ahead of their own refusals: asked of every arrival here)
    if (n_constraints > N) MI_FAIL(ctx, MI_EINVAL, "prove: witness size does not match the proving key");
    std::memset(&ctx->stats, 0, sizeof(ctx->stats));
    const auto t_begin = std::chrono::steady_clock::now();
    hipEvent_t *ev = ctx->ev;
    // Stream plan: computeH on the caller's stream; MSM A, B1, B2, K, Z on their slots (MSM_SLOT_*, own streams).  A, B and
    // K depend only on W and start at once; B2 (G2) reuses B1's sort; Z waits for h.  The latency-bound tails
    // (levels >= 2, bucket reduce, scans) of one MSM overlap the throughput-bound accumulation of the others.
    MI_TRY(mi_reserve(ctx, ctx->ws[WS_H], N * sizeof(Fr)));
    mi_fr *h = (mi_fr *)ctx->ws[WS_H].p;
    // step 4: h = computeH(a, b, c)  (bit-reversed, like gnark leaves it), then the Z MSM over h[:N-1] against the bit-reversed pk.G1.Z
    // "computeH is enqueued and its end event recorded": what the wire MSMs' accumulations wait for (hold, below).  Always fulfilled
    // before the helper threads are joined -- with a null event on a failure path, which releases them without a wait.
    std::promise<hipEvent_t> h_recorded;
    bool h_promised = false;
    const std::shared_future<hipEvent_t> h_fut = h_recorded.get_future().share();
    const std::function<hipEvent_t()> h_gate = [h_fut] { return h_fut.get(); };
    // The two wire-MSM groups are enqueued by two helper threads (each waits once for its sort's count pass) while this thread
    // enqueues computeH and the Z MSM -- or is held by the uploads of a, b, c: all sorts start at the head of the proof, beside the NTT.
    // Whatever fails, the helpers are joined and every slot is collected before the error is returned (nothing of this proof may stay
    // queued on the slots).
    // hold: the wire MSMs SORT at once (memory-bound, beside the NTT) but their bucket accumulations wait for computeH.  Measured on
    // one proof alone: let loose, the accumulations' resident waves starved the NTT passes (stream priorities order dispatch, they do
    // not preempt), computeH ended at 18 instead of 9 ms, the Z MSM's sort -- which needs h -- could no longer hide beside the other
    // accumulations and the GPU idled for 3 ms before the Z accumulation.  Not for host inputs whose a, b, c are still on the PCIe
    // bus: there the accumulations are what fills the GPU meanwhile.
    const bool hold = ctx->hold_accum && !host && (!gate || gate->abc_arrived);
    WireMsms wires;

    // How the inputs arrive.  The schedule below is the same for all of them; they differ in what "make it resident" means:
    //   w_resident(&ev_w)  makes W resident; ev_w = the event the wire MSMs must wait for, null when the host already knows W is there
    //   make_abc(k)        k = 0, 1, 2: makes a, b, c resident at abc[k]
    struct { std::function<int32_t(hipEvent_t *)> w_resident; std::function<int32_t(int)> make_abc; } arrival;
    const mi_fr *abc[3] = {a, b, c};
    std::chrono::steady_clock::time_point t_up;
    hipStream_t cps = nullptr;
    if (host) {
        // inputs in host memory (the cgo path): upload W, start the wire MSMs, and upload a, b, c WHILE they run; the
        // PCIe time of a, b, c (3/4 of the bytes) disappears behind the MSMs instead of preceding the whole proof.  The copies run on
        // the context's copy stream, which carries nothing else, and are ordered by synchronising it on this thread (a pageable copy
        // holds the calling thread anyway): events between them cost 2-3.5x on every later copy (the pool's lesson).
        // Order on the bus: W, a, b, c.  The wire MSMs start as soon as W is resident; computeH heads the proof's longest chain (h -> Z
        // MSM), so a's inverse and coset transforms start as soon as a is resident (mi_compute_h_part), b's behind b, and what needs
        // all three behind c: h is ready ~2.5 ms after c has crossed instead of a whole computeH later.  (a first: measured 2 ms worse
        // -- the wire MSMs' 14 ms of work then start 5 ms later and nothing else can fill the bus time.)
        // h2d_ms: wall clock from before the first upload to after the last one -- they overlap the wire MSMs.
        auto upload = [&, ctx](const mi_fr *dst, const mi_fr *src, size_t bytes) -> int32_t {
            const MiRange range("mi.prove.upload");
            if (bytes) MI_CHECK_HIP(ctx, hipMemcpyAsync((void *)dst, src, bytes, hipMemcpyHostToDevice, cps));
            MI_CHECK_HIP(ctx, hipStreamSynchronize(cps));
            ctx->stats.h2d_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_up).count();
            return MI_OK;
        };
        arrival.w_resident = [&, upload](hipEvent_t *ev_w) -> int32_t {
            t_up = std::chrono::steady_clock::now();
            MI_TRY(mi_copy_stream(ctx, &cps));
            MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the staging area may still be read by an earlier call's kernels
            *ev_w = nullptr;   // once the upload has returned W is resident: nothing to wait for
            return upload(W, host->W, n_wires * sizeof(mi_fr));
        };
        arrival.make_abc = [&, upload](int k) -> int32_t { return upload(abc[k], k == 0 ? host->a : k == 1 ? host->b : host->c, n_constraints * sizeof(mi_fr)); };
    } else if (gate) {
        // inputs on their way into HBM (pool upload stage): the wire MSMs start as soon as W is there; a, b, c (3/4 of the bytes)
        // finish arriving behind them, and computeH waits for exactly that, one vector at a time: a's transforms run while b is on
        // the bus; h is ready ~2.5 ms after the last vector instead of a whole computeH later
        arrival.w_resident = [](hipEvent_t *ev_w) -> int32_t { *ev_w = nullptr; return MI_OK; };   // W is resident (the pool synchronised its copy stream before handing the job over)
        arrival.make_abc = [&](int k) -> int32_t { if (!(*gate->abc)(k + 1)) MI_FAIL(ctx, MI_EHIP, "prove: the upload of a, b, c failed"); return MI_OK; };
    } else {
        // inputs already in HBM: the begin event orders the wire MSMs behind whatever wrote W on the context's stream
        arrival.w_resident = [&](hipEvent_t *ev_w) -> int32_t { *ev_w = ev[EV_PROVE_BEGIN]; return MI_OK; };
        arrival.make_abc = [](int) -> int32_t { return MI_OK; };
    }
    // W alone, from host or device memory: a and b (and c) are evaluated on the context's stream, behind the start of the wire MSMs,
    // and computeH runs behind them part by part.  Nothing but W crosses the bus, so nothing holds this thread.
    if (weval) arrival.make_abc = [&](int k) -> int32_t { return k ? MI_OK : mi_r1cs_eval_ws(ctx, weval->r1cs, W, weval->eval_c, &abc[0], &abc[1], &abc[2]); };

    auto main_part = [&]() -> int32_t {
        MI_CHECK_HIP(ctx, hipEventRecord(ev[EV_PROVE_BEGIN], ctx->stream));
        hipEvent_t ev_w = nullptr;
        MI_TRY(arrival.w_resident(&ev_w));
        wires.start(ctx, pk, W, ev_w, false, hold ? &h_gate : nullptr);
        MI_TRY(arrival.make_abc(0));
        MI_TRY(mi_compute_h_part(ctx, pk->log_n, 0, abc[0], n_constraints, h));
        MI_TRY(arrival.make_abc(1));
        MI_TRY(mi_compute_h_part(ctx, pk->log_n, 1, abc[1], n_constraints, h));
        if (derive_c) MI_TRY(mi_compute_h_part(ctx, pk->log_n, 2, abc[0], n_constraints, h, abc[1]));   // c = a o b on the device: c is never asked for (a quarter of a host proof's PCIe bytes never crosses)
        else { MI_TRY(arrival.make_abc(2)); MI_TRY(mi_compute_h_part(ctx, pk->log_n, 2, abc[2], n_constraints, h)); }
        // the Z MSM's digit count rides in computeH's last launch (mi_ctx::zhook): armed for exactly that launch
        if (pk->group[KEY_Z].c) MI_TRY(mi_msm_z_count_arm(ctx, MSM_SLOT_Z, pk->n_z_msm, pk->group[KEY_Z].c));
        const int32_t rc_h = mi_compute_h_part(ctx, pk->log_n, 3, nullptr, n_constraints, h);
        ctx->zhook.armed = false;
        MI_TRY(rc_h);
        MI_CHECK_HIP(ctx, hipEventRecord(ev[EV_H_READY], ctx->stream));
        h_recorded.set_value(ev[EV_H_READY]); h_promised = true;
        return mi_prove_enqueue_z_msm(ctx, pk, h, ev[EV_H_READY]);
    };
    {
        int32_t rc = main_part();
        if (!h_promised) h_recorded.set_value(nullptr);   // a failure before computeH's event: release the helpers
        { const int32_t r = wires.join(); if (rc == MI_OK) rc = r; }
        // a digit count computeH's last launch produced for a Z sort that never came must not meet a later sort of the same shape
        // (the sort also compares the counted vector's address)
        if (rc != MI_OK) {
            ctx->zhook.armed = ctx->zhook.done = false;
            const std::string keep = ctx->err;   // the collection below may overwrite it
            G1X t1; G2X t2;
            for (int sl : {MSM_SLOT_A, MSM_SLOT_B1, MSM_SLOT_K, MSM_SLOT_Z}) (void)mi_msm_finish(ctx, sl, 1, &t1);
            (void)mi_msm_finish(ctx, MSM_SLOT_B2, 2, &t2);
            (void)hipStreamSynchronize(ctx->stream);
            mi_set_err(ctx, keep);
            return rc;
        }
    }
    // step 6 while the GPU works: blinding multiples of delta on the host (O(1) points)
    ProofAssembler as;
    { const MiRange range("mi.prove.blinding"); as.start(pk, r_m, s_m); }
    // step 7: collect the five MSMs
    G1X msm_a, msm_b1, msm_k, msm_z;
    G2X msm_b2;
    MI_TRY(mi_msm_finish(ctx, MSM_SLOT_A, 1, &msm_a));
    MI_TRY(mi_msm_finish(ctx, MSM_SLOT_B1, 1, &msm_b1));
    const auto t_asm0 = std::chrono::steady_clock::now();
    as.have_a_b1(msm_a, msm_b1);
    MI_TRY(mi_msm_finish(ctx, MSM_SLOT_K, 1, &msm_k));
    MI_TRY(mi_msm_finish(ctx, MSM_SLOT_B2, 2, &msm_b2));
    MI_TRY(mi_msm_finish(ctx, MSM_SLOT_Z, 1, &msm_z));
    MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const auto t_gpu_done = std::chrono::steady_clock::now();
    { const MiRange range("mi.prove.assemble"); as.finish(msm_k, msm_b2, msm_z, out); }
    const auto t_end = std::chrono::steady_clock::now();
    mi_stats &st = ctx->stats;
    auto ms = [](std::chrono::steady_clock::time_point x, std::chrono::steady_clock::time_point y) {
        return std::chrono::duration<float, std::milli>(y - x).count();
    };
    auto slot_ms = [&](int slot, float *dst) -> int32_t {
        MI_CHECK_HIP(ctx, hipEventElapsedTime(dst, ctx->msm[slot].ev[MSM_EV_JOB_BEGIN], ctx->msm[slot].ev[MSM_EV_JOB_END]));
        return MI_OK;
    };
    // per-phase spans overlap (five streams): they do not add up to total_ms
    MI_CHECK_HIP(ctx, hipEventElapsedTime(&st.compute_h_ms, ev[EV_PROVE_BEGIN], ev[EV_H_READY]));
    if (pk->nb_wires) MI_TRY(slot_ms(MSM_SLOT_A, &st.msm_a_ms));
    if (pk->group[KEY_B].n) { MI_TRY(slot_ms(MSM_SLOT_B1, &st.msm_b1_ms)); MI_TRY(slot_ms(MSM_SLOT_B2, &st.msm_b2_ms)); }
    if (pk->nb_wires) MI_TRY(slot_ms(MSM_SLOT_K, &st.msm_k_ms));
    if (N > 1) MI_TRY(slot_ms(MSM_SLOT_Z, &st.msm_z_ms));
    st.assemble_ms = ms(t_gpu_done, t_end);     // host work left after the last MSM landed
    st.filter_ms = ms(t_asm0, t_gpu_done);      // host blinding work hidden under the GPU
    st.total_ms = ms(t_begin, t_end);
    if (stats) *stats = st;
    return MI_OK;
}

int32_t mi_groth16_prove_dev_gated(mi_ctx *ctx, mi_pk *pk, const mi_fr *W, size_t n_wires, const mi_fr *a, const mi_fr *b, const mi_fr *c, size_t n_constraints,
                                   const mi_fr *r, const mi_fr *s, mi_proof_out *out, mi_stats *stats, const std::function<bool(int)> &abc_ready, bool abc_arrived) {
    const AbcGate gate{&abc_ready, abc_arrived};
    return prove_common(ctx, pk, W, n_wires, a, b, c, n_constraints, r, s, out, stats, nullptr, &gate);
}

// what both W-only entry points refuse before anything is enqueued
static int32_t check_w_inputs(mi_ctx *ctx, const mi_pk *pk, const mi_r1cs *r1cs, const mi_fr *W, size_t n_wires, uint32_t flags) {
    if (!r1cs) MI_FAIL(ctx, MI_EINVAL, "prove_w: r1cs is null");
    if (!W) MI_FAIL(ctx, MI_EINVAL, "prove_w: W is null");
    if (flags & ~MI_PROVE_W_EVAL_C) MI_FAIL(ctx, MI_EINVAL, "prove_w: unknown flag");
    if (r1cs->dev != ctx->dev) MI_FAIL(ctx, MI_EINVAL, "prove_w: the r1cs was loaded on another device");
    MI_TRY(check_key_fits(ctx, pk, n_wires));
    if (n_wires != r1cs->nb_wires) MI_FAIL(ctx, MI_EINVAL, "prove_w: n_wires does not match the r1cs");
    if (pk->log_n != r1cs->log_n) MI_FAIL(ctx, MI_EINVAL, "prove_w: the key's log_n is not the domain of the r1cs's n_constraints");
    return MI_OK;
}

extern "C" {
int32_t mi_groth16_prove_w_dev(mi_ctx *ctx, mi_pk *pk, const mi_r1cs *r1cs, const mi_fr *W_dev, size_t n_wires, uint32_t flags,
                               const mi_fr *r, const mi_fr *s, mi_proof_out *out, mi_stats *stats) {
    if (!ctx || !pk || !r || !s || !out) return MI_EINVAL;
    MI_TRY(check_w_inputs(ctx, pk, r1cs, W_dev, n_wires, flags));
    const WEval we{r1cs, (flags & MI_PROVE_W_EVAL_C) != 0};
    return prove_common(ctx, pk, W_dev, n_wires, nullptr, nullptr, nullptr, 0, r, s, out, stats, nullptr, nullptr, &we);
}
int32_t mi_groth16_prove_w(mi_ctx *ctx, mi_pk *pk, const mi_r1cs *r1cs, const mi_fr *W, size_t n_wires, uint32_t flags,
                           const mi_fr *r, const mi_fr *s, mi_proof_out *out, mi_stats *stats) {
    if (!ctx || !pk || !r || !s || !out) return MI_EINVAL;
    MI_TRY(check_w_inputs(ctx, pk, r1cs, W, n_wires, flags));
    MI_TRY(mi_reserve(ctx, ctx->ws[WS_PROVE_IN], n_wires * 32 + 128));
    const HostInputs host{W, nullptr, nullptr, nullptr};
    const WEval we{r1cs, (flags & MI_PROVE_W_EVAL_C) != 0};
    return prove_common(ctx, pk, (mi_fr *)ctx->ws[WS_PROVE_IN].p, n_wires, nullptr, nullptr, nullptr, 0, r, s, out, stats, &host, nullptr, &we);
}
int32_t mi_groth16_prove_dev(mi_ctx *ctx, mi_pk *pk, const mi_fr *W, size_t n_wires, const mi_fr *a, const mi_fr *b, const mi_fr *c,
                             size_t n_constraints, const mi_fr *r, const mi_fr *s, mi_proof_out *out, mi_stats *stats) {
    return prove_common(ctx, pk, W, n_wires, a, b, c, n_constraints, r, s, out, stats, nullptr);
}
int32_t mi_groth16_prove(mi_ctx *ctx, mi_pk *pk, const mi_fr *W, size_t n_wires, const mi_fr *a, const mi_fr *b, const mi_fr *c,
                         size_t n_constraints, const mi_fr *r, const mi_fr *s, mi_proof_out *out, mi_stats *stats) {
    if (!ctx || !pk || !r || !s || !out) return MI_EINVAL;   // W, a, b: checked against their counts in prove_common; c == null: c = a o b
    const size_t wb = n_wires * 32, cb = n_constraints * 32;
    MI_TRY(mi_reserve(ctx, ctx->ws[WS_PROVE_IN], wb + 3 * cb + 128));
    char *base = (char *)ctx->ws[WS_PROVE_IN].p;
    const HostInputs host{W, a, b, c};
    return prove_common(ctx, pk, (mi_fr *)base, n_wires, (mi_fr *)(base + wb), (mi_fr *)(base + wb + cb), (mi_fr *)(base + wb + 2 * cb),
                        n_constraints, r, s, out, stats, &host);
}
}

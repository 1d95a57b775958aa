// Phase 1 on the device (include/mi355x_groth16_phase1.h): the state that holds a powers-of-tau SRS, contributions, their records, the
// verification of claimed rows and the handover to phase 2.
//
// A contribution is 5 N scalar multiplications, each point by its own dense scalar c t^k.  The lane text is scale_powers.cuh's:
//   k_phase1_table_*    one lane per point of a chunk: the table (m + 1) P, m < 2^(W-1), into the call's workspace, lane-interleaved
//   k_phase1_ladder_*   one lane per point: the scalar made in the lane, recoded, the fixed-window ladder over that table -> XYZZ
//   k_phase1_bits_*     the yardstick (knob "scale_powers_window" = 0): point_ntt.cuh's xyzz_scale, bit by bit, on the same scalars
//   k_xyzz_batch_to_affine   batch_affine.cuh's mi_xyzz_to_affine_enqueue: the chunk's XYZZ results to affine
// The driver (scale_row) walks a row chunk by chunk, so the table is sized for a chunk of lanes and not for the row.
// The records are phase1_ops.cuh's, verified on the host; the same-ratio tests are phase2_check.hip's over the rows where they are.
#include "verify_internal.h"
#include "prove_internal.h"
#include "phase2_internal.h"
#include "batch_affine.cuh"
#include "point_ntt.cuh"
#include "scale_powers.cuh"
#include "phase1_ops.cuh"
#include "stream_clock.h"
#include <algorithm>
#include <cstring>
#include <string>

struct mi_phase1 {
    u32 log_n = 0;
    u64 N = 0;
    G1Aff *tau_g1 = nullptr, *alpha_tau_g1 = nullptr, *beta_tau_g1 = nullptr;   // device: 2 N, N, N
    G2Aff *tau_g2 = nullptr;                                                    // device: N
    G2Aff beta_g2;
    G1Aff watch[3];   // host copies of tau_g1[1], alpha_tau_g1[0], beta_tau_g1[0]: what the records are about
    u64 n_records = 0;
    uint8_t chain[32] = {0};
};

namespace {

constexpr u32 DEFAULT_CHUNK = 1u << 18;    // lanes per chunk: four waves on every SIMD of 256 CUs; the width and the chunk measured fastest (profiles/phase1.txt)
constexpr u64 MAX_DEBUG_POINTS = (u64)1 << 28;

// ---------------------------------------------------------------------------------------------------- kernels
template <class F, int W>
MI_D void lane_table(XYZZ<F> *tab, u64 stride, const Affine<F> *pts, u64 m) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) scale_powers_table_lane<F, W>(tab + i, stride, pts[i]);
}
template <class F, int W>
MI_D void lane_ladder(XYZZ<F> *out, const XYZZ<F> *tab, u64 stride, u64 m, const Fr &t, const Fr &c, u64 k0) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    u32 s[8];
    scale_powers_scalar(t, c, k0 + i, s);
    out[i] = scale_powers_ladder_lane<F, W>(tab + i, stride, s);
}
template <class F>
MI_D void lane_bits(XYZZ<F> *out, const Affine<F> *pts, u64 m, const Fr &t, const Fr &c, u64 k0) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) out[i] = xyzz_scale(XYZZ<F>::from_affine(pts[i]), fe_pow_u64(t, k0 + i) * c);
}
template <int W> __global__ void __launch_bounds__(64) k_phase1_table_g1(G1X *tab, u64 stride, const G1Aff *pts, u64 m) { lane_table<Fp, W>(tab, stride, pts, m); }
template <int W> __global__ void __launch_bounds__(64) k_phase1_table_g2(G2X *tab, u64 stride, const G2Aff *pts, u64 m) { lane_table<Fp2, W>(tab, stride, pts, m); }
template <int W> __global__ void __launch_bounds__(64) k_phase1_ladder_g1(G1X *out, const G1X *tab, u64 stride, u64 m, Fr t, Fr c, u64 k0) { lane_ladder<Fp, W>(out, tab, stride, m, t, c, k0); }
template <int W> __global__ void __launch_bounds__(64) k_phase1_ladder_g2(G2X *out, const G2X *tab, u64 stride, u64 m, Fr t, Fr c, u64 k0) { lane_ladder<Fp2, W>(out, tab, stride, m, t, c, k0); }
__global__ void __launch_bounds__(64) k_phase1_bits_g1(G1X *out, const G1Aff *pts, u64 m, Fr t, Fr c, u64 k0) { lane_bits(out, pts, m, t, c, k0); }
__global__ void __launch_bounds__(64) k_phase1_bits_g2(G2X *out, const G2Aff *pts, u64 m, Fr t, Fr c, u64 k0) { lane_bits(out, pts, m, t, c, k0); }
__global__ void __launch_bounds__(256) k_phase1_fill_g1(G1Aff *out, u64 n, G1Aff p) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = p;
}
__global__ void __launch_bounds__(256) k_phase1_fill_g2(G2Aff *out, u64 n, G2Aff p) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = p;
}

template <class F> struct Launch;
template <> struct Launch<Fp> {
    template <int W> static void table(hipStream_t st, unsigned g, G1X *tab, u64 stride, const G1Aff *pts, u64 m) { hipLaunchKernelGGL(k_phase1_table_g1<W>, dim3(g), dim3(64), 0, st, tab, stride, pts, m); }
    template <int W> static void ladder(hipStream_t st, unsigned g, G1X *out, const G1X *tab, u64 stride, u64 m, const Fr &t, const Fr &c, u64 k0) { hipLaunchKernelGGL(k_phase1_ladder_g1<W>, dim3(g), dim3(64), 0, st, out, tab, stride, m, t, c, k0); }
    static void bits(hipStream_t st, unsigned g, G1X *out, const G1Aff *pts, u64 m, const Fr &t, const Fr &c, u64 k0) { hipLaunchKernelGGL(k_phase1_bits_g1, dim3(g), dim3(64), 0, st, out, pts, m, t, c, k0); }
};
template <> struct Launch<Fp2> {
    template <int W> static void table(hipStream_t st, unsigned g, G2X *tab, u64 stride, const G2Aff *pts, u64 m) { hipLaunchKernelGGL(k_phase1_table_g2<W>, dim3(g), dim3(64), 0, st, tab, stride, pts, m); }
    template <int W> static void ladder(hipStream_t st, unsigned g, G2X *out, const G2X *tab, u64 stride, u64 m, const Fr &t, const Fr &c, u64 k0) { hipLaunchKernelGGL(k_phase1_ladder_g2<W>, dim3(g), dim3(64), 0, st, out, tab, stride, m, t, c, k0); }
    static void bits(hipStream_t st, unsigned g, G2X *out, const G2Aff *pts, u64 m, const Fr &t, const Fr &c, u64 k0) { hipLaunchKernelGGL(k_phase1_bits_g2, dim3(g), dim3(64), 0, st, out, pts, m, t, c, k0); }
};

// ---------------------------------------------------------------------------------------------------- the chunk driver
// what the knobs say for this call
struct Plan { u32 window, chunk; };
Plan plan_of(const mi_ctx *ctx) { return Plan{ctx->scale_powers_window, ctx->scale_powers_chunk ? ctx->scale_powers_chunk : DEFAULT_CHUNK}; }

// the workspace of one call for one curve: sized for a chunk of lanes
template <class F> struct Workspace {
    XYZZ<F> *tab = nullptr, *x = nullptr;
    F *prefix = nullptr;
    u64 lanes = 0;
    int32_t reserve(mi_ctx *ctx, Arena &ar, const Plan &pl, u64 n) {
        lanes = std::min<u64>(pl.chunk, std::max<u64>(n, 1));
        if (pl.window) MI_TRY(ar.alloc(ctx, &tab, (size_t)(lanes << (pl.window - 1))));
        MI_TRY(ar.alloc(ctx, &x, (size_t)lanes));
        MI_TRY(ar.alloc(ctx, &prefix, (size_t)lanes));
        return MI_OK;
    }
    void release(Arena &ar) { ar.release(tab); ar.release(x); ar.release(prefix); tab = nullptr; x = nullptr; prefix = nullptr; }
};

// out[i] = [c t^(k0 + i)] in[i], i < n, device arrays of affine points (out may be in).  mul_ms / aff_ms take the device times.
template <class F>
int32_t scale_row(mi_ctx *ctx, StreamLaps &laps, const Plan &pl, const Workspace<F> &ws, const Affine<F> *in, Affine<F> *out, u64 n, const Fr &t, const Fr &c, u64 k0,
                  float &mul_ms, float &aff_ms) {
    hipStream_t st = ctx->stream;
    float skip = 0;
    MI_TRY(laps.lap(ctx, skip));   // what came before this row is nobody's time
    for (u64 off = 0; off < n; off += ws.lanes) {
        const u64 m = std::min<u64>(ws.lanes, n - off);
        const unsigned g = mi_blocks_of(m, 64);
        switch (pl.window) {
        case 0: Launch<F>::bits(st, g, ws.x, in + off, m, t, c, k0 + off); break;
#define MI_PHASE1_CASE(W) \
        case W: Launch<F>::template table<W>(st, g, ws.tab, ws.lanes, in + off, m); \
                Launch<F>::template ladder<W>(st, g, ws.x, ws.tab, ws.lanes, m, t, c, k0 + off); break;
        MI_PHASE1_CASE(2) MI_PHASE1_CASE(3) MI_PHASE1_CASE(4) MI_PHASE1_CASE(5)
#undef MI_PHASE1_CASE
        default: MI_FAIL(ctx, MI_EINVAL, "phase1: scale_powers_window is " + std::to_string(pl.window));
        }
        MI_CHECK_HIP(ctx, hipGetLastError());
        MI_TRY(laps.lap(ctx, mul_ms));
        MI_TRY(mi_xyzz_to_affine_enqueue<F>(ctx, (const XYZZ<F> *)ws.x, out + off, ws.prefix, (size_t)m));
        MI_TRY(laps.lap(ctx, aff_ms));
    }
    return MI_OK;
}

void free_rows(mi_phase1 *S) {
    for (void *p : {(void *)S->tau_g1, (void *)S->alpha_tau_g1, (void *)S->beta_tau_g1, (void *)S->tau_g2}) if (p) (void)hipFree(p);
    S->tau_g1 = S->alpha_tau_g1 = S->beta_tau_g1 = nullptr; S->tau_g2 = nullptr;
}
// the rows of a state, or of arrays about to become one, as a descriptor of DEVICE pointers
mi_srs_desc rows_desc(const G1Aff *t1, const G1Aff *al, const G1Aff *be, const G2Aff *t2, const G2Aff &b2, u64 N) {
    mi_srs_desc d{};
    d.tau_g1 = (const mi_g1_affine *)t1; d.alpha_tau_g1 = (const mi_g1_affine *)al; d.beta_tau_g1 = (const mi_g1_affine *)be; d.tau_g2 = (const mi_g2_affine *)t2;
    std::memcpy(&d.beta_g2, &b2, sizeof(b2));
    d.n_tau_g1 = 2 * N; d.n_alpha_tau_g1 = d.n_beta_tau_g1 = d.n_tau_g2 = N;
    return d;
}
// tau_g1[1], alpha_tau_g1[0], beta_tau_g1[0] of device rows
int32_t fetch_watch(mi_ctx *ctx, const G1Aff *t1, const G1Aff *al, const G1Aff *be, G1Aff out[3]) {
    MI_CHECK_HIP(ctx, hipMemcpyAsync(&out[0], t1 + 1, sizeof(G1Aff), hipMemcpyDeviceToHost, ctx->stream));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(&out[1], al, sizeof(G1Aff), hipMemcpyDeviceToHost, ctx->stream));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(&out[2], be, sizeof(G1Aff), hipMemcpyDeviceToHost, ctx->stream));
    MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MI_OK;
}

// the new rows of a contribution, built beside the state's; the caller swaps them in
struct NewRows { G1Aff *t1 = nullptr, *al = nullptr, *be = nullptr; G2Aff *t2 = nullptr; G2Aff b2; };
int32_t contribute_run(mi_ctx *ctx, const mi_phase1 *S, const Fr &t, const Fr &a, const Fr &b, Arena &ar, NewRows &nr) {
    mi_phase1_stats &stats = ctx->phase1_stats;
    const Plan pl = plan_of(ctx);
    const u64 N = S->N;
    stats.window = pl.window; stats.chunk = pl.chunk;
    StreamLaps laps;
    MI_TRY(laps.init(ctx));
    MI_TRY(ar.alloc(ctx, &nr.t1, (size_t)(2 * N)));
    MI_TRY(ar.alloc(ctx, &nr.al, (size_t)N));
    MI_TRY(ar.alloc(ctx, &nr.be, (size_t)N));
    MI_TRY(ar.alloc(ctx, &nr.t2, (size_t)N));
    const Fr one = Fr::one();
    {
        Workspace<Fp> ws;
        MI_TRY(ws.reserve(ctx, ar, pl, 2 * N));
        MI_TRY(scale_row<Fp>(ctx, laps, pl, ws, S->tau_g1, nr.t1, 2 * N, t, one, 0, stats.scalar_mul_ms[0], stats.affine_ms[0]));
        MI_TRY(scale_row<Fp>(ctx, laps, pl, ws, S->alpha_tau_g1, nr.al, N, t, a, 0, stats.scalar_mul_ms[1], stats.affine_ms[1]));
        MI_TRY(scale_row<Fp>(ctx, laps, pl, ws, S->beta_tau_g1, nr.be, N, t, b, 0, stats.scalar_mul_ms[2], stats.affine_ms[2]));
        ws.release(ar);
    }
    {
        Workspace<Fp2> ws;
        G2Aff *b2 = nullptr;
        MI_TRY(ws.reserve(ctx, ar, pl, N));
        MI_TRY(ar.alloc(ctx, &b2, (size_t)1));
        MI_TRY(scale_row<Fp2>(ctx, laps, pl, ws, S->tau_g2, nr.t2, N, t, one, 0, stats.scalar_mul_ms[3], stats.affine_ms[3]));
        // beta_g2: a row of one point, its scalar b t^0
        MI_CHECK_HIP(ctx, hipMemcpyAsync(b2, &S->beta_g2, sizeof(G2Aff), hipMemcpyHostToDevice, ctx->stream));
        MI_TRY(scale_row<Fp2>(ctx, laps, pl, ws, b2, b2, 1, one, b, 0, stats.scalar_mul_ms[3], stats.affine_ms[3]));
        MI_CHECK_HIP(ctx, hipMemcpyAsync(&nr.b2, b2, sizeof(G2Aff), hipMemcpyDeviceToHost, ctx->stream));
        MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ar.release(b2);
        ws.release(ar);
    }
    stats.peak_bytes = ar.peak - (size_t)N * (2 * 64 + 64 + 64 + 128);   // the new rows are the state's to be, not the call's scratch
    return MI_OK;
}
// t, a, b of a contribution: none 0, all below r
int32_t read_factors(mi_ctx *ctx, const mi_phase1 *S, const mi_fr *tau, const mi_fr *alpha, const mi_fr *beta, Fr d[3]) {
    if (!S) MI_FAIL(ctx, MI_EINVAL, "phase1: the state is null");
    const struct { const char *name; const mi_fr *p; } in[3] = {{"tau", tau}, {"alpha", alpha}, {"beta", beta}};
    for (int x = 0; x < 3; x++) {
        if (!in[x].p) MI_FAIL(ctx, MI_EINVAL, std::string("phase1: ") + in[x].name + " is null");
        d[x] = fr_of(*in[x].p);
        if (d[x].is_zero()) MI_FAIL(ctx, MI_EINVAL, std::string("phase1: ") + in[x].name + " is 0");
        if (!fe_is_reduced(d[x])) MI_FAIL(ctx, MI_EINVAL, std::string("phase1: ") + in[x].name + " is not below r");
    }
    return MI_OK;
}
// the contribution itself: the rows swapped in and `before` (may be null) = the watched points it started from
int32_t contribute(mi_ctx *ctx, mi_phase1 *S, const Fr d[3], G1Aff *before) {
    const double t0 = now_ms();
    ctx->phase1_stats = mi_phase1_stats{};
    Arena ar;
    NewRows nr;
    G1Aff watch[3];
    int32_t rc = contribute_run(ctx, S, d[0], d[1], d[2], ar, nr);
    if (rc == MI_OK) rc = fetch_watch(ctx, nr.t1, nr.al, nr.be, watch);
    if (rc != MI_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }   // the arena frees the new rows; the state is as it was
    if (before) for (int x = 0; x < 3; x++) before[x] = S->watch[x];
    free_rows(S);
    S->tau_g1 = nr.t1; S->alpha_tau_g1 = nr.al; S->beta_tau_g1 = nr.be; S->tau_g2 = nr.t2; S->beta_g2 = nr.b2;
    for (void *p : {(void *)nr.t1, (void *)nr.al, (void *)nr.be, (void *)nr.t2}) ar.disown(p);
    for (int x = 0; x < 3; x++) S->watch[x] = watch[x];
    ctx->phase1_stats.total_ms = (float)(now_ms() - t0);
    return MI_OK;
}

int32_t check_log_n(mi_ctx *ctx, uint64_t log_n) {
    if (log_n < 1 || log_n > MI_SETUP_MAX_LOG_N) MI_FAIL(ctx, MI_EINVAL, "phase1: log_n is " + std::to_string(log_n) + ", not from 1 to " + std::to_string(MI_SETUP_MAX_LOG_N));
    return MI_OK;
}
// host rows of an SRS to device arrays of the arena, point-checked as mi_phase2_init checks them
int32_t upload_rows(mi_ctx *ctx, Arena &ar, const mi_srs_desc *srs, u64 N, uint32_t flags, NewRows &nr) {
    hipStream_t st = ctx->stream;
    G2Aff *b2 = nullptr;
    MI_TRY(ar.alloc(ctx, &nr.t1, (size_t)(2 * N)));
    MI_TRY(ar.alloc(ctx, &nr.al, (size_t)N));
    MI_TRY(ar.alloc(ctx, &nr.be, (size_t)N));
    MI_TRY(ar.alloc(ctx, &nr.t2, (size_t)N));
    MI_TRY(ar.alloc(ctx, &b2, (size_t)1));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(nr.t1, srs->tau_g1, 2 * N * sizeof(G1Aff), hipMemcpyHostToDevice, st));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(nr.al, srs->alpha_tau_g1, N * sizeof(G1Aff), hipMemcpyHostToDevice, st));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(nr.be, srs->beta_tau_g1, N * sizeof(G1Aff), hipMemcpyHostToDevice, st));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(nr.t2, srs->tau_g2, N * sizeof(G2Aff), hipMemcpyHostToDevice, st));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(b2, &srs->beta_g2, sizeof(G2Aff), hipMemcpyHostToDevice, st));
    MI_CHECK_HIP(ctx, hipStreamSynchronize(st));
    const Phase2Row rows[5] = {{"tau_g1", false, nr.t1, 2 * N}, {"alpha_tau_g1", false, nr.al, N}, {"beta_tau_g1", false, nr.be, N}, {"tau_g2", true, nr.t2, N}, {"beta_g2", true, b2, 1}};
    MI_TRY(mi_phase2_check_points(ctx, ar, rows, 5, flags));
    ar.release(b2);
    std::memcpy(&nr.b2, &srs->beta_g2, sizeof(G2Aff));
    return MI_OK;
}
int32_t check_domain(mi_ctx *ctx, uint64_t n_domain, u32 *log_n) {
    if (n_domain < 2 || (n_domain & (n_domain - 1)) || n_domain > ((uint64_t)1 << MI_SETUP_MAX_LOG_N))
        MI_FAIL(ctx, MI_EINVAL, "phase1: n_domain is " + std::to_string(n_domain) + ", not a power of two from 2 to 2^" + std::to_string(MI_SETUP_MAX_LOG_N));
    u32 l = 0;
    while (((uint64_t)1 << l) < n_domain) l++;
    *log_n = l;
    return MI_OK;
}

}  // namespace

// phase2_internal.h: for the audit of a key against a phase-1 state's rows (keyaudit.hip)
mi_srs_desc mi_phase1_rows_desc(const mi_phase1 *p1) { return rows_desc(p1->tau_g1, p1->alpha_tau_g1, p1->beta_tau_g1, p1->tau_g2, p1->beta_g2, p1->N); }

extern "C" {

int32_t mi_phase1_get_stats(mi_ctx *ctx, mi_phase1_stats *out) {
    if (!ctx || !out) return MI_EINVAL;
    *out = ctx->phase1_stats;
    return MI_OK;
}

int32_t mi_phase1_init(mi_ctx *ctx, uint32_t log_n, mi_phase1 **out) {
    if (!ctx) return MI_EINVAL;
    if (!out) MI_FAIL(ctx, MI_EINVAL, "phase1: out is null");
    *out = nullptr;
    MI_TRY(check_log_n(ctx, log_n));
    const u64 N = (u64)1 << log_n;
    mi_phase1 *S = new (std::nothrow) mi_phase1();
    if (!S) return MI_ENOMEM;
    S->log_n = log_n; S->N = N;
    auto body = [&]() -> int32_t {
        Arena ar;
        MI_TRY(ar.alloc(ctx, &S->tau_g1, (size_t)(2 * N)));
        MI_TRY(ar.alloc(ctx, &S->alpha_tau_g1, (size_t)N));
        MI_TRY(ar.alloc(ctx, &S->beta_tau_g1, (size_t)N));
        MI_TRY(ar.alloc(ctx, &S->tau_g2, (size_t)N));
        const G1Aff g1 = g1_generator();
        const G2Aff g2 = g2_generator();
        hipLaunchKernelGGL(k_phase1_fill_g1, dim3(mi_blocks_of(2 * N, 256)), dim3(256), 0, ctx->stream, S->tau_g1, 2 * N, g1);
        hipLaunchKernelGGL(k_phase1_fill_g1, dim3(mi_blocks_of(N, 256)), dim3(256), 0, ctx->stream, S->alpha_tau_g1, N, g1);
        hipLaunchKernelGGL(k_phase1_fill_g1, dim3(mi_blocks_of(N, 256)), dim3(256), 0, ctx->stream, S->beta_tau_g1, N, g1);
        hipLaunchKernelGGL(k_phase1_fill_g2, dim3(mi_blocks_of(N, 256)), dim3(256), 0, ctx->stream, S->tau_g2, N, g2);
        MI_CHECK_HIP(ctx, hipGetLastError());
        MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        S->beta_g2 = g2;
        S->watch[0] = S->watch[1] = S->watch[2] = g1;
        for (void *p : {(void *)S->tau_g1, (void *)S->alpha_tau_g1, (void *)S->beta_tau_g1, (void *)S->tau_g2}) ar.disown(p);
        return MI_OK;
    };
    const int32_t rc = body();
    if (rc != MI_OK) { (void)hipStreamSynchronize(ctx->stream); delete S; return rc; }   // the arena has freed the rows
    *out = S;
    return MI_OK;
}

int32_t mi_phase1_from_srs(mi_ctx *ctx, const mi_srs_desc *srs, uint64_t n_domain, uint32_t flags, mi_phase1 **out) {
    if (!ctx) return MI_EINVAL;
    if (!out) MI_FAIL(ctx, MI_EINVAL, "phase1: out is null");
    *out = nullptr;
    if (flags & ~MI_KEYFILE_NO_SUBGROUP_CHECK) MI_FAIL(ctx, MI_EINVAL, "phase1: unknown flag");
    u32 log_n = 0;
    MI_TRY(check_domain(ctx, n_domain, &log_n));
    MI_TRY(mi_phase2_srs_host_check(ctx, srs, n_domain));
    mi_phase1 *S = new (std::nothrow) mi_phase1();
    if (!S) return MI_ENOMEM;
    S->log_n = log_n; S->N = n_domain;
    Arena ar;
    NewRows nr;
    int32_t rc = upload_rows(ctx, ar, srs, n_domain, flags, nr);
    if (rc == MI_OK) rc = fetch_watch(ctx, nr.t1, nr.al, nr.be, S->watch);
    if (rc != MI_OK) { (void)hipStreamSynchronize(ctx->stream); delete S; return rc; }
    S->tau_g1 = nr.t1; S->alpha_tau_g1 = nr.al; S->beta_tau_g1 = nr.be; S->tau_g2 = nr.t2; S->beta_g2 = nr.b2;
    for (void *p : {(void *)nr.t1, (void *)nr.al, (void *)nr.be, (void *)nr.t2}) ar.disown(p);
    *out = S;
    return MI_OK;
}

int32_t mi_phase1_set_transcript_id(mi_ctx *ctx, mi_phase1 *S, const uint8_t id[32]) {
    if (!ctx) return MI_EINVAL;
    if (!S || !id) MI_FAIL(ctx, MI_EINVAL, "phase1: the state or the transcript id is null");
    if (S->n_records) MI_FAIL(ctx, MI_EINVAL, "phase1: the transcript id is set before the first record only; the state holds " + std::to_string(S->n_records));
    std::memcpy(S->chain, id, 32);
    return MI_OK;
}

int32_t mi_phase1_contribute(mi_ctx *ctx, mi_phase1 *S, const mi_fr *tau, const mi_fr *alpha, const mi_fr *beta) {
    if (!ctx) return MI_EINVAL;
    Fr d[3];
    MI_TRY(read_factors(ctx, S, tau, alpha, beta, d));
    return contribute(ctx, S, d, nullptr);
}

int32_t mi_phase1_contribute_proved(mi_ctx *ctx, mi_phase1 *S, const mi_fr *tau, const mi_fr *alpha, const mi_fr *beta, const mi_fr *nonce, mi_phase1_record *out) {
    if (!ctx) return MI_EINVAL;
    Fr d[3], k[3];
    MI_TRY(read_factors(ctx, S, tau, alpha, beta, d));
    if (!out) MI_FAIL(ctx, MI_EINVAL, "phase1: the record's out is null");
    for (int x = 0; x < 3; x++) {
        if (nonce) {
            k[x] = fr_of(nonce[x]);
            if (k[x].is_zero()) MI_FAIL(ctx, MI_EINVAL, "phase1: nonce[" + std::to_string(x) + "] is 0");
            if (!fe_is_reduced(k[x])) MI_FAIL(ctx, MI_EINVAL, "phase1: nonce[" + std::to_string(x) + "] is not below r");
        } else MI_TRY(mi_draw_nonce(ctx, "phase1: the operating system gave no randomness for the nonces (getrandom)", "phase1: a drawn nonce is 0", k[x]));
    }
    G1Aff before[3];
    MI_TRY(contribute(ctx, S, d, before));
    Phase1Record rec;
    phase1_record_make(S->chain, S->n_records, before, S->watch, d, k, &rec);
    std::memcpy(out, &rec, sizeof(rec));
    std::memcpy(S->chain, rec.hash, 32);
    S->n_records++;
    return MI_OK;
}

int32_t mi_phase1_check(mi_ctx *ctx, const mi_phase1 *S, const uint8_t *seed, uint32_t *failed) {
    if (!ctx) return MI_EINVAL;
    if (!S || !failed) MI_FAIL(ctx, MI_EINVAL, "phase1 check: the state or failed is null");
    const mi_srs_desc d = rows_desc(S->tau_g1, S->alpha_tau_g1, S->beta_tau_g1, S->tau_g2, S->beta_g2, S->N);
    mi_srs_check_stats stats;
    return mi_srs_check_rows_dev(ctx, "phase1 check", &d, S->N, seed, stats, failed);
}

int32_t mi_phase1_verify_adopt(mi_ctx *ctx, mi_phase1 *S, const mi_srs_desc *claim, const mi_phase1_record *rec, size_t m, const uint8_t *seed, uint32_t *failed,
                               uint64_t *first_bad_record) {
    if (!ctx) return MI_EINVAL;
    if (!S) MI_FAIL(ctx, MI_EINVAL, "phase1 verify: the state is null");
    if (!m) MI_FAIL(ctx, MI_EINVAL, "phase1 verify: m is 0: claimed rows come with the records of their contributions");
    if (!claim || !rec || !failed) MI_FAIL(ctx, MI_EINVAL, "phase1 verify: claim, rec or failed is null");
    MI_TRY(mi_phase2_srs_host_check(ctx, claim, S->N));
    const u64 N = S->N;
    Arena ar;
    NewRows nr;
    uint32_t mask = 0;
    auto body = [&]() -> int32_t {
        MI_TRY(upload_rows(ctx, ar, claim, N, 0, nr));
        const mi_srs_desc d = rows_desc(nr.t1, nr.al, nr.be, nr.t2, nr.b2, N);
        mi_srs_check_stats stats;
        return mi_srs_check_rows_dev(ctx, "phase1 verify", &d, N, seed, stats, &mask);
    };
    const int32_t rc = body();
    if (rc != MI_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    // the chain, on the host: from where this state stands
    const uint64_t fb = phase1_records_first_bad(S->watch, S->chain, S->n_records, (const Phase1Record *)rec, m);
    if (fb != m) mask |= MI_PHASE1_BAD_RECORD;
    const G1Aff claimed[3] = {g1_of(claim->tau_g1[1]), g1_of(claim->alpha_tau_g1[0]), g1_of(claim->beta_tau_g1[0])};
    const mi_g1_affine *last = &rec[m - 1].tau1;   // tau1, alpha1, beta1 lie one after the other
    if (std::memcmp(claimed, last, sizeof(claimed)) != 0) mask |= MI_PHASE1_BAD_LINK;
    *failed = mask;
    if (first_bad_record) *first_bad_record = fb;
    if (!mask) {   // the state takes the claimed rows as they stand on the device; nothing below can fail
        free_rows(S);
        S->tau_g1 = nr.t1; S->alpha_tau_g1 = nr.al; S->beta_tau_g1 = nr.be; S->tau_g2 = nr.t2; S->beta_g2 = nr.b2;
        for (void *p : {(void *)nr.t1, (void *)nr.al, (void *)nr.be, (void *)nr.t2}) ar.disown(p);
        for (int x = 0; x < 3; x++) S->watch[x] = claimed[x];
        std::memcpy(S->chain, rec[m - 1].hash, 32);
        S->n_records += m;
    }
    return MI_OK;
}

int32_t mi_phase1_get_info(mi_ctx *ctx, const mi_phase1 *S, mi_phase1_info *out) {
    if (!ctx) return MI_EINVAL;
    if (!S || !out) MI_FAIL(ctx, MI_EINVAL, "phase1: the state or out is null");
    *out = mi_phase1_info{};
    out->log_n = S->log_n; out->n_records = S->n_records;
    std::memcpy(out->chain, S->chain, 32);
    std::memcpy(&out->tau1, S->watch, sizeof(S->watch));   // tau1, alpha1, beta1 lie one after the other
    return MI_OK;
}

int32_t mi_phase1_export(mi_ctx *ctx, const mi_phase1 *S, mi_g1_affine *tau_g1, mi_g1_affine *alpha_tau_g1, mi_g1_affine *beta_tau_g1, mi_g2_affine *tau_g2,
                         mi_g2_affine *beta_g2, uint64_t cap_tau_g1, uint64_t cap_alpha_tau_g1, uint64_t cap_beta_tau_g1, uint64_t cap_tau_g2, uint64_t n[4]) {
    if (!ctx) return MI_EINVAL;
    if (!S || !n) MI_FAIL(ctx, MI_EINVAL, "phase1: the state or n is null");
    const struct { const char *name; void *dst; const void *src; u64 cap, cnt, bytes; } rows[4] = {
        {"tau_g1", tau_g1, S->tau_g1, cap_tau_g1, 2 * S->N, 64}, {"alpha_tau_g1", alpha_tau_g1, S->alpha_tau_g1, cap_alpha_tau_g1, S->N, 64},
        {"beta_tau_g1", beta_tau_g1, S->beta_tau_g1, cap_beta_tau_g1, S->N, 64}, {"tau_g2", tau_g2, S->tau_g2, cap_tau_g2, S->N, 128}};
    for (int i = 0; i < 4; i++) n[i] = rows[i].cnt;
    for (const auto &r : rows)
        if (r.dst && r.cap < r.cnt) MI_FAIL(ctx, MI_EINVAL, std::string("phase1: ") + r.name + " holds " + std::to_string(r.cnt) + " points, the array given has room for " + std::to_string(r.cap));
    for (const auto &r : rows)
        if (r.dst) MI_CHECK_HIP(ctx, hipMemcpyAsync(r.dst, r.src, r.cnt * r.bytes, hipMemcpyDeviceToHost, ctx->stream));
    MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (beta_g2) std::memcpy(beta_g2, &S->beta_g2, sizeof(G2Aff));
    return MI_OK;
}

int32_t mi_phase1_free(mi_ctx *ctx, mi_phase1 *S) {
    if (!ctx || !S) return MI_EINVAL;
    (void)hipStreamSynchronize(ctx->stream);
    free_rows(S);
    delete S;
    return MI_OK;
}

int32_t mi_phase2_init_from_phase1(mi_ctx *ctx, const mi_r1cs_desc *r1cs, const mi_phase1 *p1, const mi_fr *sigma, uint32_t flags, mi_phase2 **out) {
    if (!ctx) return MI_EINVAL;
    if (!out) MI_FAIL(ctx, MI_EINVAL, "phase2: out is null");
    *out = nullptr;
    if (!p1) MI_FAIL(ctx, MI_EINVAL, "phase2: the phase-1 state is null");
    const mi_srs_desc d = rows_desc(p1->tau_g1, p1->alpha_tau_g1, p1->beta_tau_g1, p1->tau_g2, p1->beta_g2, p1->N);
    return mi_phase2_init_rows(ctx, r1cs, &d, true, sigma, flags, out);   // a circuit above the state's N is refused as a short row is
}

int32_t mi_debug_scale_powers_dev(mi_ctx *ctx, int32_t g2, const void *pts_host, size_t n, const mi_fr *t, const mi_fr *c, uint64_t k0, void *out_host) {
    if (!ctx) return MI_EINVAL;
    if (!t || !c || ((!pts_host || !out_host) && n)) MI_FAIL(ctx, MI_EINVAL, "scale powers: a null argument");
    if (n > MAX_DEBUG_POINTS || k0 > ~(uint64_t)0 - n) MI_FAIL(ctx, MI_EINVAL, "scale powers: n or k0 out of range");
    const Fr tt = fr_of(*t), cc = fr_of(*c);
    if (!fe_is_reduced(tt) || !fe_is_reduced(cc)) MI_FAIL(ctx, MI_EINVAL, "scale powers: t or c is not below r");
    ctx->phase1_stats = mi_phase1_stats{};
    if (!n) return MI_OK;
    const Plan pl = plan_of(ctx);
    mi_phase1_stats &stats = ctx->phase1_stats;
    stats.window = pl.window; stats.chunk = pl.chunk;
    const double t0 = now_ms();
    auto body = [&]() -> int32_t {
        Arena ar;
        StreamLaps laps;
        MI_TRY(laps.init(ctx));
        void *pts = nullptr;
        const size_t bytes = n * (g2 ? sizeof(G2Aff) : sizeof(G1Aff));
        MI_TRY(ar.alloc(ctx, &pts, bytes));
        MI_CHECK_HIP(ctx, hipMemcpyAsync(pts, pts_host, bytes, hipMemcpyHostToDevice, ctx->stream));
        if (g2) {
            Workspace<Fp2> ws;
            MI_TRY(ws.reserve(ctx, ar, pl, n));
            MI_TRY(scale_row<Fp2>(ctx, laps, pl, ws, (const G2Aff *)pts, (G2Aff *)pts, n, tt, cc, k0, stats.scalar_mul_ms[0], stats.affine_ms[0]));
        } else {
            Workspace<Fp> ws;
            MI_TRY(ws.reserve(ctx, ar, pl, n));
            MI_TRY(scale_row<Fp>(ctx, laps, pl, ws, (const G1Aff *)pts, (G1Aff *)pts, n, tt, cc, k0, stats.scalar_mul_ms[0], stats.affine_ms[0]));
        }
        MI_CHECK_HIP(ctx, hipMemcpyAsync(out_host, pts, bytes, hipMemcpyDeviceToHost, ctx->stream));
        MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        stats.peak_bytes = ar.peak;
        return MI_OK;
    };
    const int32_t rc = body();
    if (rc != MI_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    stats.total_ms = (float)(now_ms() - t0);
    return MI_OK;
}

}  // extern "C"

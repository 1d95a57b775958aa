// Phase-2 key generation from a powers-of-tau SRS (include/mi355x_groth16_phase2.h): Setup's arithmetic "in the exponent".
// Replaces gnark's mpcsetup.InitPhase2 / Contribute / ExtractKeys for the key the reference makes with groth16.Setup (mt.go:448).
//
//   1  the SRS rows go up and are checked point by point: on the curve and not at infinity (point_check.cuh's POINT_RULE_SRS_ROW through
//      k_points_check_g1 / _g2), the G2 points in the r-torsion (keyfile.hip's endomorphism test)
//   2  Z_i = [tau^(i + N)]1 - [tau^i]1, stored bit-reversed
//   3  the Lagrange bases [L_i]1, [alpha L_i]1, [beta L_i]1, [L_i]2: the inverse NTT over points of point_ntt.cuh, a launch per stage, a
//      lane per butterfly, then batch_affine.cuh's conversion in place over the SRS row (bit-reversed order)
//   4  the three matrices sorted by column by setup.hip's MatrixSorter, then the sums of points of sparse_points.cuh:
//      [A_j]1, [B_j]1, [B_j]2 and [t_j]1 = one accumulator over (A, [beta L]), (B, [alpha L]), (C, [L])
//   5  masks from the points at infinity, Setup's wire selection (key_handover.h), the gathers for vk.K and the Pedersen bases
// The state keeps the plain affine arrays and, per commitment, the point [-sigma]2; contribute multiplies Z, K, BasisExpSigma, that
// point and the two delta points by scalars; seal copies
// the arrays into an ordinary key and the streams are written from the state's arrays directly, both through key_handover.h.
#include "prove_internal.h"
#include "r1cs_internal.h"
#include "keyfile_internal.h"
#include "keyfile_ops.cuh"
#include "phase2_internal.h"
#include "key_handover.h"
#include "batch_affine.cuh"
#include "point_ntt.cuh"
#include "sparse_points.cuh"
#include "point_check.cuh"
#include "stream_clock.h"
#include <algorithm>
#include <cstring>
#include <vector>

namespace {

// ---------------------------------------------------------------------------------------------------- kernels
// Z_i = tau_g1[i + N] - tau_g1[i] into slot bitrev(i)
__global__ void __launch_bounds__(256) k_phase2_z(G1X *Z, const G1Aff *tau, u32 log_n) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >> log_n) return;
    G1X acc = G1X::from_affine(tau[i + ((u64)1 << log_n)]);
    xyzz_madd(acc, tau[i], true);
    Z[bitrev_u32((u32)i, log_n)] = acc;
}
// tw[m] = w^(-m), m < half
__global__ void __launch_bounds__(256) k_phase2_twiddles(Fr *tw, u64 half, Fr w_inv) {
    const u64 m = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (m < half) tw[m] = fe_pow_u64(w_inv, m);
}
template <class F>
MI_D void lane_from_affine(XYZZ<F> *out, const Affine<F> *in, u64 n) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = XYZZ<F>::from_affine(in[i]);
}
__global__ void __launch_bounds__(256) k_phase2_from_affine_g1(G1X *out, const G1Aff *in, u64 n) { lane_from_affine(out, in, n); }
__global__ void __launch_bounds__(256) k_phase2_from_affine_g2(G2X *out, const G2Aff *in, u64 n) { lane_from_affine(out, in, n); }
// one stage of the point NTT: a lane per butterfly
__global__ void __launch_bounds__(64) k_phase2_ntt_stage_g1(G1X *a, u32 log_n, u32 s, const Fr *tw, Fr scale) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < ((u64)1 << log_n) / 2) point_ntt_stage_lane(a, log_n, s, t, tw, scale);
}
__global__ void __launch_bounds__(64) k_phase2_ntt_stage_g2(G2X *a, u32 log_n, u32 s, const Fr *tw, Fr scale) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < ((u64)1 << log_n) / 2) point_ntt_stage_lane(a, log_n, s, t, tw, scale);
}
// every point of an array times one scalar (contribute, BasisExpSigma)
template <class F>
MI_D void lane_scale(XYZZ<F> *out, const Affine<F> *in, u64 n, const Fr &s) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = xyzz_scale(XYZZ<F>::from_affine(in[i]), s);
}
__global__ void __launch_bounds__(64) k_phase2_scale_g1(G1X *out, const G1Aff *in, u64 n, Fr s) { lane_scale(out, in, n, s); }
__global__ void __launch_bounds__(64) k_phase2_scale_g2(G2X *out, const G2Aff *in, u64 n, Fr s) { lane_scale(out, in, n, s); }

// the sums of points: the three passes of sparse_points.cuh under plain names
__global__ void __launch_bounds__(64) k_phase2_sum_short_g1(G1X *out, u64 nb_wires, PointSources<Fp, 1> src) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < nb_wires) out[j] = sparse_points_short(src, (u32)j);
}
__global__ void __launch_bounds__(64) k_phase2_sum_short_g1x3(G1X *out, u64 nb_wires, PointSources<Fp, 3> src) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < nb_wires) out[j] = sparse_points_short(src, (u32)j);
}
__global__ void __launch_bounds__(64) k_phase2_sum_short_g2(G2X *out, u64 nb_wires, PointSources<Fp2, 1> src) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < nb_wires) out[j] = sparse_points_short(src, (u32)j);
}
__global__ void __launch_bounds__(64) k_phase2_sum_pieces_g1(G1X *partial, PointSource<Fp> ps) { sparse_points_pieces(partial, ps); }
__global__ void __launch_bounds__(64) k_phase2_sum_pieces_g2(G2X *partial, PointSource<Fp2> ps) { sparse_points_pieces(partial, ps); }
__global__ void __launch_bounds__(64) k_phase2_sum_combine_g1(G1X *out, PointSource<Fp> ps, const G1X *partial) { sparse_points_combine(out, ps, partial); }
__global__ void __launch_bounds__(64) k_phase2_sum_combine_g2(G2X *out, PointSource<Fp2> ps, const G2X *partial) { sparse_points_combine(out, ps, partial); }

// masks and the wire selection's flags from the per-wire points (setup.hip's k_elementwise, from points): keep_k = private wire, the
// committed and commitment wires are cleared afterwards
__global__ void __launch_bounds__(256) k_phase2_masks(const G1Aff *A, const G1Aff *B, uint8_t *inf_a, uint8_t *inf_b, u32 *keep_a, u32 *keep_b, u32 *keep_k,
                                                      u64 nb_wires, u32 nb_public) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nb_wires) return;
    const bool za = A[j].is_inf(), zb = B[j].is_inf();
    inf_a[j] = za; inf_b[j] = zb;
    keep_a[j] = !za; keep_b[j] = !zb; keep_k[j] = j >= nb_public;
}
__global__ void __launch_bounds__(256) k_phase2_gather_g1(G1Aff *dst, const G1Aff *src, const u32 *idx, u64 n) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[idx[i]];
}

// ---------------------------------------------------------------------------------------------------- host side
template <class F> struct Curve;
template <> struct Curve<Fp> {
    static void from_affine(hipStream_t st, G1X *o, const G1Aff *i, u64 n) { hipLaunchKernelGGL(k_phase2_from_affine_g1, dim3(mi_blocks_of(n, 256)), dim3(256), 0, st, o, i, n); }
    static void stage(hipStream_t st, G1X *a, u32 log_n, u32 s, const Fr *tw, const Fr &sc) { hipLaunchKernelGGL(k_phase2_ntt_stage_g1, dim3(mi_blocks_of(((u64)1 << log_n) / 2, 64)), dim3(64), 0, st, a, log_n, s, tw, sc); }
    static void scale(hipStream_t st, G1X *o, const G1Aff *i, u64 n, const Fr &s) { hipLaunchKernelGGL(k_phase2_scale_g1, dim3(mi_blocks_of(n, 64)), dim3(64), 0, st, o, i, n, s); }
    static void pieces(hipStream_t st, unsigned grid, G1X *partial, const PointSource<Fp> &ps) { hipLaunchKernelGGL(k_phase2_sum_pieces_g1, dim3(grid), dim3(64), 0, st, partial, ps); }
    static void combine(hipStream_t st, unsigned grid, G1X *out, const PointSource<Fp> &ps, const G1X *partial) { hipLaunchKernelGGL(k_phase2_sum_combine_g1, dim3(grid), dim3(64), 0, st, out, ps, partial); }
};
template <> struct Curve<Fp2> {
    static void from_affine(hipStream_t st, G2X *o, const G2Aff *i, u64 n) { hipLaunchKernelGGL(k_phase2_from_affine_g2, dim3(mi_blocks_of(n, 256)), dim3(256), 0, st, o, i, n); }
    static void stage(hipStream_t st, G2X *a, u32 log_n, u32 s, const Fr *tw, const Fr &sc) { hipLaunchKernelGGL(k_phase2_ntt_stage_g2, dim3(mi_blocks_of(((u64)1 << log_n) / 2, 64)), dim3(64), 0, st, a, log_n, s, tw, sc); }
    static void scale(hipStream_t st, G2X *o, const G2Aff *i, u64 n, const Fr &s) { hipLaunchKernelGGL(k_phase2_scale_g2, dim3(mi_blocks_of(n, 64)), dim3(64), 0, st, o, i, n, s); }
    static void pieces(hipStream_t st, unsigned grid, G2X *partial, const PointSource<Fp2> &ps) { hipLaunchKernelGGL(k_phase2_sum_pieces_g2, dim3(grid), dim3(64), 0, st, partial, ps); }
    static void combine(hipStream_t st, unsigned grid, G2X *out, const PointSource<Fp2> &ps, const G2X *partial) { hipLaunchKernelGGL(k_phase2_sum_combine_g2, dim3(grid), dim3(64), 0, st, out, ps, partial); }
};
void short_pass(hipStream_t st, G1X *out, u64 nw, const PointSources<Fp, 1> &s) { hipLaunchKernelGGL(k_phase2_sum_short_g1, dim3(mi_blocks_of(nw, 64)), dim3(64), 0, st, out, nw, s); }
void short_pass(hipStream_t st, G1X *out, u64 nw, const PointSources<Fp, 3> &s) { hipLaunchKernelGGL(k_phase2_sum_short_g1x3, dim3(mi_blocks_of(nw, 64)), dim3(64), 0, st, out, nw, s); }
void short_pass(hipStream_t st, G2X *out, u64 nw, const PointSources<Fp2, 1> &s) { hipLaunchKernelGGL(k_phase2_sum_short_g2, dim3(mi_blocks_of(nw, 64)), dim3(64), 0, st, out, nw, s); }

// every point of an affine array times s, in place
template <class F>
int32_t scale_array(mi_ctx *ctx, Affine<F> *pts, u64 n, const Fr &s) {
    if (!n) return MI_OK;
    Arena ar;
    XYZZ<F> *x = nullptr;
    F *prefix = nullptr;
    MI_TRY(ar.alloc(ctx, &x, (size_t)n));
    MI_TRY(ar.alloc(ctx, &prefix, (size_t)n));
    Curve<F>::scale(ctx->stream, x, pts, n, s);
    MI_TRY(mi_xyzz_to_affine_enqueue<F>(ctx, x, pts, prefix, (size_t)n));
    MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MI_OK;
}
// the inverse point NTT of one SRS row, in place: row[bitrev(i)] <- [L_i] (affine)
template <class F>
int32_t lagrange_row(mi_ctx *ctx, Arena &ar, StreamLaps &laps, float &ntt_ms, Affine<F> *row, u32 log_n, const Fr *tw, F *prefix) {
    const u64 N = (u64)1 << log_n;
    XYZZ<F> *x = nullptr;
    MI_TRY(ar.alloc(ctx, &x, (size_t)N));
    Curve<F>::from_affine(ctx->stream, x, row, N);
    const Fr n_inv = fe_inv(fe_from_u32<FrParams>((u32)N));
    for (u32 s = 0; s < log_n; s++) Curve<F>::stage(ctx->stream, x, log_n, s, tw, s == 0 ? n_inv : Fr::one());
    MI_CHECK_HIP(ctx, hipGetLastError());
    MI_TRY(laps.lap(ctx, ntt_ms));
    MI_TRY(mi_xyzz_to_affine_enqueue<F>(ctx, x, row, prefix, (size_t)N));
    MI_TRY(laps.lap(ctx, ctx->phase2_stats.affine_ms));
    ar.release(x);
    return MI_OK;
}

// one matrix on the device, sorted by column
struct SortedMatrix { u32 *off = nullptr; uint2 *sorted = nullptr; u32 nnz = 0; };
// where the plan of one matrix's long columns goes: sized for that matrix
struct LongPlan { uint2 *pieces = nullptr; SparseLong *long_cols = nullptr; };

// pair m of a sum: a matrix, the basis its rows multiply, and the pair's two counters (ctr[2 m], ctr[2 m + 1])
template <class F>
PointSource<F> source_of(const SortedMatrix &mat, const LongPlan &lp, const Affine<F> *basis, const Fr *coeffs, u32 log_n, u32 *ctr, int m) {
    return PointSource<F>{mat.off, SortedEntries{mat.sorted}, PointTerm<F>{basis, coeffs, log_n}, ctr + 2 * m, lp.pieces, lp.long_cols};
}
// out[j] = the sum over the NS pairs of column j; long_columns / chunks (may be null) += the plan's counts
template <class F, int NS>
int32_t sum_points(mi_ctx *ctx, XYZZ<F> *out, u64 nw, const PointSources<F, NS> &src, u32 *ctr_base, XYZZ<F> *partial, u64 *long_columns, u64 *chunks) {
    hipStream_t st = ctx->stream;
    MI_CHECK_HIP(ctx, hipMemsetAsync(ctr_base, 0, 32, st));
    short_pass(st, out, nw, src);
    const unsigned grid = (unsigned)ctx->cu_count * 8;   // single-wave workgroups, grid-stride over the pieces
    for (int m = 0; m < NS; m++) {   // pair by pair: the partials are one array, and two pairs can hold the same column
        Curve<F>::pieces(st, grid, partial, src.s[m]);
        Curve<F>::combine(st, grid, out, src.s[m], partial);
    }
    MI_CHECK_HIP(ctx, hipGetLastError());
    u32 ctr_h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    MI_CHECK_HIP(ctx, hipMemcpyAsync(ctr_h, ctr_base, 32, hipMemcpyDeviceToHost, st));
    MI_CHECK_HIP(ctx, hipStreamSynchronize(st));
    for (int m = 0; m < NS; m++) {
        if (chunks) *chunks += ctr_h[2 * m];
        if (long_columns) *long_columns += ctr_h[2 * m + 1];
    }
    return MI_OK;
}

void free_state(mi_phase2 *s) {
    for (void *p : {s->g1_a, s->g1_b, s->g2_b, s->g1_k, s->g1_z, s->vk_k}) if (p) (void)hipFree(p);
    for (auto &pd : s->ped) { if (pd.basis) (void)hipFree(pd.basis); if (pd.bes) (void)hipFree(pd.bes); }
    delete s;
}

int32_t init_run(mi_ctx *ctx, const mi_r1cs_desc *d, const mi_srs_desc *srs, bool on_device, const R1csShape &sh, const std::vector<Fr> &sigma, uint32_t flags, mi_phase2 *S) {
    hipStream_t st = ctx->stream;
    mi_phase2_stats &stats = ctx->phase2_stats;
    const u64 N = sh.N, nw = sh.nb_wires;
    const u32 log_n = sh.log_n;
    Arena ar;
    StreamLaps laps;
    MI_TRY(laps.init(ctx));
    // ---- 1: the SRS goes up and is checked
    G1Aff *T1 = nullptr, *Al = nullptr, *Be = nullptr;
    G2Aff *T2 = nullptr, *b2 = nullptr;
    MI_TRY(ar.alloc(ctx, &T1, (size_t)(2 * N)));
    MI_TRY(ar.alloc(ctx, &Al, (size_t)N));
    MI_TRY(ar.alloc(ctx, &Be, (size_t)N));
    MI_TRY(ar.alloc(ctx, &T2, (size_t)N));
    MI_TRY(ar.alloc(ctx, &b2, (size_t)1));
    const hipMemcpyKind up = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;   // the rows are transformed in place: copies either way
    MI_CHECK_HIP(ctx, hipMemcpyAsync(T1, srs->tau_g1, 2 * N * 64, up, st));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(Al, srs->alpha_tau_g1, N * 64, up, st));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(Be, srs->beta_tau_g1, N * 64, up, st));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(T2, srs->tau_g2, N * 128, up, st));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(b2, &srs->beta_g2, 128, hipMemcpyHostToDevice, st));
    // the points the SRS hands over as they are
    MI_CHECK_HIP(ctx, hipMemcpyAsync(&S->alpha1, Al, 64, hipMemcpyDeviceToHost, st));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(&S->beta1, Be, 64, hipMemcpyDeviceToHost, st));
    MI_TRY(laps.lap(ctx, stats.upload_ms));
    {
        const Phase2Row rows[5] = {{"tau_g1", false, T1, 2 * N}, {"alpha_tau_g1", false, Al, N}, {"beta_tau_g1", false, Be, N}, {"tau_g2", true, T2, N}, {"beta_g2", true, b2, 1}};
        MI_TRY(mi_phase2_check_points(ctx, ar, rows, 5, flags));
        ar.release(b2);
    }
    MI_TRY(laps.lap(ctx, stats.check_ms));
    // one scratch for every batched conversion: a field element per point (Fp2-sized, the longest array)
    Fp2 *prefix = nullptr;
    MI_TRY(ar.alloc(ctx, &prefix, (size_t)std::max(N, nw)));
    // ---- 2: Z
    {
        G1X *zx = nullptr;
        MI_TRY(ar.alloc(ctx, &zx, (size_t)N));
        MI_TRY(ar.alloc(ctx, (G1Aff **)&S->g1_z, (size_t)N));
        hipLaunchKernelGGL(k_phase2_z, dim3(mi_blocks_of(N, 256)), dim3(256), 0, st, zx, (const G1Aff *)T1, log_n);
        MI_CHECK_HIP(ctx, hipGetLastError());
        MI_TRY(laps.lap(ctx, stats.z_ms));
        MI_TRY(mi_xyzz_to_affine_enqueue<Fp>(ctx, zx, (G1Aff *)S->g1_z, (Fp *)prefix, (size_t)N));
        MI_TRY(laps.lap(ctx, stats.affine_ms));
        ar.release(zx);
    }
    // ---- 3: the Lagrange bases, in place over the rows (T1's upper half is done with)
    {
        Fr *tw = nullptr;
        MI_TRY(ar.alloc(ctx, &tw, (size_t)std::max<u64>(N / 2, 1)));
        if (N / 2) hipLaunchKernelGGL(k_phase2_twiddles, dim3(mi_blocks_of(N / 2, 256)), dim3(256), 0, st, tw, N / 2, fe_inv(fr_domain_generator(log_n)));
        MI_CHECK_HIP(ctx, hipGetLastError());
        MI_TRY(lagrange_row<Fp>(ctx, ar, laps, stats.point_ntt_g1_ms, T1, log_n, tw, (Fp *)prefix));
        MI_TRY(lagrange_row<Fp>(ctx, ar, laps, stats.point_ntt_g1_ms, Al, log_n, tw, (Fp *)prefix));
        MI_TRY(lagrange_row<Fp>(ctx, ar, laps, stats.point_ntt_g1_ms, Be, log_n, tw, (Fp *)prefix));
        MI_TRY(lagrange_row<Fp2>(ctx, ar, laps, stats.point_ntt_g2_ms, T2, log_n, tw, prefix));
        ar.release(tw);
    }
    // ---- 4: the matrices by column (setup.hip's sort), then the sums of points
    const u32 max_nnz = std::max(sh.nnz[0], std::max(sh.nnz[1], sh.nnz[2]));
    Fr *coeffs = nullptr;
    SortedMatrix mat[3];
    {
        MatrixSorter ms{d, &sh};
        MI_TRY(ar.alloc(ctx, &coeffs, (size_t)d->n_coeffs));
        if (d->n_coeffs) MI_CHECK_HIP(ctx, hipMemcpyAsync(coeffs, d->coeffs, d->n_coeffs * 32, hipMemcpyHostToDevice, st));
        MI_TRY(ar.alloc(ctx, &ms.row_ptr, (size_t)sh.nc + 1));
        MI_TRY(ar.alloc(ctx, &ms.col, (size_t)max_nnz));
        MI_TRY(ar.alloc(ctx, &ms.cf, (size_t)max_nnz));
        MI_TRY(ar.alloc(ctx, &ms.cnt, (size_t)nw));
        MI_TRY(ar.alloc(ctx, &ms.rank, (size_t)max_nnz));
        for (int k = 0; k < 3; k++) {
            mat[k].nnz = sh.nnz[k];
            MI_TRY(ar.alloc(ctx, &mat[k].off, (size_t)nw + 1));
            MI_TRY(ar.alloc(ctx, &mat[k].sorted, (size_t)sh.nnz[k]));
            MI_TRY(ms.upload(ctx, st, k));
            MI_TRY(laps.lap(ctx, stats.upload_ms));
            MI_TRY(ms.sort(ctx, st, k, mat[k].off, mat[k].sorted));
            MI_CHECK_HIP(ctx, hipGetLastError());
            MI_TRY(laps.lap(ctx, stats.sparse_g1_ms));   // the host arrays of this matrix are not read after this point
        }
        for (void *p : {(void *)ms.row_ptr, (void *)ms.col, (void *)ms.cf, (void *)ms.cnt, (void *)ms.rank}) ar.release(p);
    }
    // a long column has more than SPARSE_SHORT entries and at most len / SPARSE_SHORT pieces
    LongPlan lp[3];
    u32 *ctr = nullptr;
    MI_TRY(ar.alloc(ctx, &ctr, (size_t)8));
    for (int k = 0; k < 3; k++) {
        const size_t cap_long = (size_t)sh.nnz[k] / SPARSE_SHORT + 1;
        MI_TRY(ar.alloc(ctx, &lp[k].pieces, cap_long));
        MI_TRY(ar.alloc(ctx, &lp[k].long_cols, cap_long));
    }
    const size_t cap_partial = (size_t)max_nnz / SPARSE_SHORT + 1;
    G1Aff *pA = nullptr, *pB1 = nullptr, *pT = nullptr;   // per wire, affine
    G2Aff *pB2 = nullptr;
    {
        G1X *x1 = nullptr, *part1 = nullptr;
        MI_TRY(ar.alloc(ctx, &x1, (size_t)nw));
        MI_TRY(ar.alloc(ctx, &part1, cap_partial));
        MI_TRY(ar.alloc(ctx, &pA, (size_t)nw));
        MI_TRY(ar.alloc(ctx, &pB1, (size_t)nw));
        MI_TRY(ar.alloc(ctx, &pT, (size_t)nw));
        // A over [L]1; B over [L]1; t over (A, [beta L]1), (B, [alpha L]1), (C, [L]1) -- whose plan gives the stats their counts
        const PointSources<Fp, 1> sa{{source_of<Fp>(mat[0], lp[0], T1, coeffs, log_n, ctr, 0)}};
        const PointSources<Fp, 1> sb{{source_of<Fp>(mat[1], lp[1], T1, coeffs, log_n, ctr, 0)}};
        const PointSources<Fp, 3> stt{{source_of<Fp>(mat[0], lp[0], Be, coeffs, log_n, ctr, 0), source_of<Fp>(mat[1], lp[1], Al, coeffs, log_n, ctr, 1),
                                       source_of<Fp>(mat[2], lp[2], T1, coeffs, log_n, ctr, 2)}};
        MI_TRY((sum_points<Fp, 1>(ctx, x1, nw, sa, ctr, part1, nullptr, nullptr)));
        MI_TRY(laps.lap(ctx, stats.sparse_g1_ms));
        MI_TRY(mi_xyzz_to_affine_enqueue<Fp>(ctx, x1, pA, (Fp *)prefix, (size_t)nw));
        MI_TRY(laps.lap(ctx, stats.affine_ms));
        MI_TRY((sum_points<Fp, 1>(ctx, x1, nw, sb, ctr, part1, nullptr, nullptr)));
        MI_TRY(laps.lap(ctx, stats.sparse_g1_ms));
        MI_TRY(mi_xyzz_to_affine_enqueue<Fp>(ctx, x1, pB1, (Fp *)prefix, (size_t)nw));
        MI_TRY(laps.lap(ctx, stats.affine_ms));
        MI_TRY((sum_points<Fp, 3>(ctx, x1, nw, stt, ctr, part1, &stats.long_columns, &stats.chunks)));
        MI_TRY(laps.lap(ctx, stats.sparse_g1_ms));
        MI_TRY(mi_xyzz_to_affine_enqueue<Fp>(ctx, x1, pT, (Fp *)prefix, (size_t)nw));
        MI_TRY(laps.lap(ctx, stats.affine_ms));
        ar.release(x1); ar.release(part1);
    }
    {
        G2X *x2 = nullptr, *part2 = nullptr;
        MI_TRY(ar.alloc(ctx, &x2, (size_t)nw));
        MI_TRY(ar.alloc(ctx, &part2, (size_t)sh.nnz[1] / SPARSE_SHORT + 1));
        MI_TRY(ar.alloc(ctx, &pB2, (size_t)nw));
        const PointSources<Fp2, 1> sb2{{source_of<Fp2>(mat[1], lp[1], T2, coeffs, log_n, ctr, 0)}};
        MI_TRY((sum_points<Fp2, 1>(ctx, x2, nw, sb2, ctr, part2, nullptr, nullptr)));
        MI_TRY(laps.lap(ctx, stats.sparse_g2_ms));
        MI_TRY(mi_xyzz_to_affine_enqueue<Fp2>(ctx, x2, pB2, prefix, (size_t)nw));
        MI_TRY(laps.lap(ctx, stats.affine_ms));
        ar.release(x2); ar.release(part2);
    }
    for (int k = 0; k < 3; k++) { ar.release(mat[k].off); ar.release(mat[k].sorted); ar.release(lp[k].pieces); ar.release(lp[k].long_cols); }
    for (void *p : {(void *)T1, (void *)Al, (void *)Be, (void *)T2, (void *)coeffs, (void *)ctr, (void *)prefix}) ar.release(p);
    // ---- 5: masks, compaction, gathers
    uint8_t *inf_a = nullptr, *inf_b = nullptr;
    WireSelection sel; sel.nb_wires = nw;
    MI_TRY(ar.alloc(ctx, &inf_a, (size_t)nw));
    MI_TRY(ar.alloc(ctx, &inf_b, (size_t)nw));
    MI_TRY(ar.alloc(ctx, &sel.slot_a, (size_t)nw + 1));
    MI_TRY(ar.alloc(ctx, &sel.slot_b, (size_t)nw + 1));
    MI_TRY(ar.alloc(ctx, &sel.slot_k, (size_t)nw + 1));
    hipLaunchKernelGGL(k_phase2_masks, dim3(mi_blocks_of(nw, 256)), dim3(256), 0, st, (const G1Aff *)pA, (const G1Aff *)pB1, inf_a, inf_b, sel.slot_a, sel.slot_b, sel.slot_k, nw, sh.nb_public);
    MI_CHECK_HIP(ctx, hipGetLastError());
    MI_TRY(sel.scan(ctx, ar, sh.removed));
    S->inf_a.resize(nw); S->inf_b.resize(nw);
    MI_TRY(sel.fetch(ctx, inf_a, inf_b, S->inf_a.data(), S->inf_b.data()));
    S->n_a = sel.n_a; S->n_b = sel.n_b; S->n_k = sel.n_k; S->n_vk = sh.vk_wires.size();
    MI_TRY(ar.alloc(ctx, (G1Aff **)&S->g1_a, (size_t)S->n_a));
    MI_TRY(ar.alloc(ctx, (G1Aff **)&S->g1_b, (size_t)S->n_b));
    MI_TRY(ar.alloc(ctx, (G2Aff **)&S->g2_b, (size_t)S->n_b));
    MI_TRY(ar.alloc(ctx, (G1Aff **)&S->g1_k, (size_t)S->n_k));
    MI_TRY(ar.alloc(ctx, (G1Aff **)&S->vk_k, (size_t)S->n_vk));
    MI_TRY(sel.compact(ctx, S->g1_a, pA, sel.slot_a, sizeof(G1Aff)));
    MI_TRY(sel.compact(ctx, S->g1_b, pB1, sel.slot_b, sizeof(G1Aff)));
    MI_TRY(sel.compact(ctx, S->g2_b, pB2, sel.slot_b, sizeof(G2Aff)));
    MI_TRY(sel.compact(ctx, S->g1_k, pT, sel.slot_k, sizeof(G1Aff)));
    MI_CHECK_HIP(ctx, hipGetLastError());
    auto gather = [&](void **dst, const u32 *wires, size_t n) -> int32_t {
        u32 *idx = nullptr;
        MI_TRY(ar.alloc(ctx, &idx, n));
        if (n) MI_CHECK_HIP(ctx, hipMemcpyAsync(idx, wires, n * 4, hipMemcpyHostToDevice, st));
        MI_CHECK_HIP(ctx, hipStreamSynchronize(st));   // wires may be the caller's
        if (n) hipLaunchKernelGGL(k_phase2_gather_g1, dim3(mi_blocks_of(n, 256)), dim3(256), 0, st, (G1Aff *)*dst, (const G1Aff *)pT, (const u32 *)idx, (u64)n);
        MI_CHECK_HIP(ctx, hipGetLastError());
        return MI_OK;
    };
    MI_TRY(gather(&S->vk_k, sh.vk_wires.data(), sh.vk_wires.size()));
    S->ped.resize(sh.n_commitments);
    for (u32 k = 0; k < sh.n_commitments; k++) {
        mi_phase2::Ped &pd = S->ped[k];
        pd.n = d->n_committed[k]; pd.sigma = sigma[k];
        MI_TRY(ar.alloc(ctx, (G1Aff **)&pd.basis, (size_t)pd.n));
        MI_TRY(ar.alloc(ctx, (G1Aff **)&pd.bes, (size_t)pd.n));
        MI_TRY(gather(&pd.basis, d->committed[k], (size_t)pd.n));
        MI_CHECK_HIP(ctx, hipMemcpyAsync(pd.bes, pd.basis, pd.n * 64, hipMemcpyDeviceToDevice, st));
        MI_TRY(scale_array<Fp>(ctx, (G1Aff *)pd.bes, pd.n, pd.sigma));
    }
    if (sh.n_commitments) {   // [-sigma_k]2 as mi_pedersen_vk_make makes it
        std::vector<mi_fr> sg(sh.n_commitments);
        std::vector<mi_pedersen_vk> pvk(sh.n_commitments);
        for (u32 k = 0; k < sh.n_commitments; k++) std::memcpy(&sg[k], &sigma[k], 32);
        MI_TRY(mi_pedersen_vk_make(ctx, sg.data(), sh.n_commitments, pvk.data()));
        for (u32 k = 0; k < sh.n_commitments; k++) std::memcpy(&S->ped[k].g_sigma_neg, &pvk[k].g_sigma_neg, sizeof(G2Aff));
    }
    MI_TRY(laps.lap(ctx, stats.affine_ms));
    // beta_g2 as it is, and the generators where gamma = delta = 1
    std::memcpy(&S->beta2, &srs->beta_g2, 128);
    S->delta1 = g1_generator();
    S->gamma2 = S->delta2 = g2_generator();
    stats.peak_bytes = ar.peak;
    // the state takes its arrays
    for (void *p : {S->g1_a, S->g1_b, S->g2_b, S->g1_k, S->g1_z, S->vk_k}) ar.disown(p);
    for (auto &pd : S->ped) { ar.disown(pd.basis); ar.disown(pd.bes); }
    return MI_OK;
}

// the state's own arrays as a key's (seal hands copies of them over, the streams read them where they are)
KeyArrays key_arrays_of(const mi_phase2 *S) {
    KeyArrays ka(S->log_n, S->nb_public, S->nb_wires, S->inf_a.data(), S->inf_b.data(), S->removed.data(), S->removed.size());
    ka.arr[KEY_G1_A] = S->g1_a; ka.arr[KEY_G1_B] = S->g1_b; ka.arr[KEY_G1_K] = S->g1_k; ka.arr[KEY_G1_Z] = S->g1_z; ka.arr[KEY_G2_B] = S->g2_b;
    ka.n[KEY_G1_A] = S->n_a; ka.n[KEY_G1_B] = ka.n[KEY_G2_B] = S->n_b; ka.n[KEY_G1_K] = S->n_k; ka.n[KEY_G1_Z] = S->N;
    ka.small1[0] = S->alpha1; ka.small1[1] = S->beta1; ka.small1[2] = S->delta1; ka.small2[0] = S->beta2; ka.small2[1] = S->delta2; ka.small2[2] = S->gamma2;
    return ka;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------- shared with phase2_check.hip
int32_t mi_phase2_srs_host_check(mi_ctx *ctx, const mi_srs_desc *srs, u64 N) {
    if (!srs) MI_FAIL(ctx, MI_EINVAL, "phase2: srs is null");
    const struct { const char *name; const void *p; u64 n, need; } rows[4] = {
        {"tau_g1", srs->tau_g1, srs->n_tau_g1, 2 * N}, {"alpha_tau_g1", srs->alpha_tau_g1, srs->n_alpha_tau_g1, N},
        {"beta_tau_g1", srs->beta_tau_g1, srs->n_beta_tau_g1, N}, {"tau_g2", srs->tau_g2, srs->n_tau_g2, N}};
    for (const auto &r : rows) {
        if (!r.p) MI_FAIL(ctx, MI_EINVAL, std::string("phase2: srs.") + r.name + " is null");
        if (r.n < r.need) MI_FAIL(ctx, MI_EINVAL, std::string("phase2: srs.n_") + r.name + " is " + std::to_string(r.n) + ", the circuit needs " + std::to_string(r.need) + " points");
    }
    return MI_OK;
}
int32_t mi_phase2_scale_sigma(mi_ctx *ctx, mi_phase2 *S, const Fr *sf) {
    for (u32 k = 0; k < S->n_commitments; k++) {
        MI_TRY(scale_array<Fp>(ctx, (G1Aff *)S->ped[k].bes, S->ped[k].n, sf[k]));
        S->ped[k].sigma = S->ped[k].sigma * sf[k];
    }
    if (!S->n_commitments) return MI_OK;
    // the points [-sigma_k]2: one array of n_commitments points, one factor each -- a launch per point of the kernel delta2 goes through
    Arena ar;
    G2Aff *g = nullptr;
    std::vector<G2Aff> h(S->n_commitments);
    for (u32 k = 0; k < S->n_commitments; k++) h[k] = S->ped[k].g_sigma_neg;
    MI_TRY(ar.alloc(ctx, &g, (size_t)S->n_commitments));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(g, h.data(), h.size() * sizeof(G2Aff), hipMemcpyHostToDevice, ctx->stream));
    for (u32 k = 0; k < S->n_commitments; k++) MI_TRY(scale_array<Fp2>(ctx, g + k, 1, sf[k]));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(h.data(), g, h.size() * sizeof(G2Aff), hipMemcpyDeviceToHost, ctx->stream));
    MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (u32 k = 0; k < S->n_commitments; k++) S->ped[k].g_sigma_neg = h[k];
    return MI_OK;
}
void mi_phase2_pedersen_vk_of(const mi_phase2 *S, mi_pedersen_vk *out) {
    const G2Aff gen = g2_generator();
    for (u32 k = 0; k < S->n_commitments; k++) {
        std::memcpy(&out[k].g, &gen, sizeof(gen));
        std::memcpy(&out[k].g_sigma_neg, &S->ped[k].g_sigma_neg, sizeof(gen));
    }
}
int32_t mi_phase2_check_points(mi_ctx *ctx, Arena &ar, const Phase2Row *rows, int n_rows, uint32_t flags) {
    if (n_rows > 8) return MI_EINVAL;
    BadSlots bad;   // word 2 i: row i's curve check; 2 i + 1: its r-torsion check
    MI_TRY(bad.init(ctx, 16, &ar));
    for (int i = 0; i < n_rows; i++) MI_TRY(mi_points_check_enqueue(ctx, rows[i].g2, rows[i].pts, rows[i].n, POINT_RULE_SRS_ROW, bad.dev + 2 * i));
    MI_TRY(bad.fetch(ctx));
    for (int i = 0; i < n_rows; i++)
        if (bad.bad(2 * i))
            MI_FAIL(ctx, MI_EINVAL, std::string("phase2: srs.") + rows[i].name + "[" + std::to_string(bad.host[2 * i]) + "] is at infinity or not on its curve");
    if (!(flags & MI_KEYFILE_NO_SUBGROUP_CHECK)) {   // of points of the twist only: the curve checks have passed
        bool any = false;
        for (int i = 0; i < n_rows; i++)
            if (rows[i].g2) { MI_TRY(mi_keyfile_subgroup_enqueue(ctx, rows[i].pts, (size_t)rows[i].n, false, bad.dev + 2 * i + 1)); any = true; }
        if (any) MI_TRY(bad.fetch(ctx));
        for (int i = 0; i < n_rows; i++)
            if (bad.bad(2 * i + 1))
                MI_FAIL(ctx, MI_EINVAL, std::string("phase2: srs.") + rows[i].name + "[" + std::to_string(bad.host[2 * i + 1]) + "] is not in the r-torsion");
    }
    return MI_OK;
}

extern "C" {

int32_t mi_phase2_get_stats(mi_ctx *ctx, mi_phase2_stats *out) {
    if (!ctx || !out) return MI_EINVAL;
    *out = ctx->phase2_stats;
    return MI_OK;
}

int32_t mi_phase2_init(mi_ctx *ctx, const mi_r1cs_desc *r1cs, const mi_srs_desc *srs, const mi_fr *sigma, uint32_t flags, mi_phase2 **out) {
    return mi_phase2_init_rows(ctx, r1cs, srs, false, sigma, flags, out);
}

}  // extern "C"

int32_t mi_phase2_init_rows(mi_ctx *ctx, const mi_r1cs_desc *r1cs, const mi_srs_desc *srs, bool on_device, const mi_fr *sigma, uint32_t flags, mi_phase2 **out) {
    if (!ctx) return MI_EINVAL;
    if (!out) MI_FAIL(ctx, MI_EINVAL, "phase2: out is null");
    *out = nullptr;
    if (!r1cs) MI_FAIL(ctx, MI_EINVAL, "phase2: r1cs is null");
    if (flags & ~MI_KEYFILE_NO_SUBGROUP_CHECK) MI_FAIL(ctx, MI_EINVAL, "phase2: unknown flag");
    R1csShape sh;
    MI_TRY(mi_r1cs_validate(ctx, "phase2", r1cs, sh));
    MI_TRY(mi_phase2_srs_host_check(ctx, srs, sh.N));
    if (sh.n_commitments && !sigma) MI_FAIL(ctx, MI_EINVAL, "phase2: sigma is null");
    std::vector<Fr> sg(sh.n_commitments);
    for (u32 k = 0; k < sh.n_commitments; k++) {
        sg[k] = fr_of(sigma[k]);
        if (sg[k].is_zero()) MI_FAIL(ctx, MI_EINVAL, "phase2: sigma[" + std::to_string(k) + "] is 0");
    }
    const double t0 = now_ms();
    ctx->phase2_stats = mi_phase2_stats{};
    ctx->phase2_stats.entries = (u64)sh.nnz[0] + sh.nnz[1] + sh.nnz[2];
    mi_phase2 *S = new (std::nothrow) mi_phase2();
    if (!S) return MI_ENOMEM;
    S->log_n = sh.log_n; S->N = sh.N; S->nb_public = sh.nb_public; S->nb_wires = sh.nb_wires; S->n_commitments = sh.n_commitments;
    S->removed = sh.removed;
    const int32_t rc = init_run(ctx, r1cs, srs, on_device, sh, sg, flags, S);
    if (rc != MI_OK) {   // the arena has freed everything, the state's arrays included (they are disowned last)
        (void)hipStreamSynchronize(ctx->stream);
        delete S;
        return rc;
    }
    ctx->phase2_stats.total_ms = (float)(now_ms() - t0);
    *out = S;
    return MI_OK;
}

extern "C" {

int32_t mi_phase2_contribute(mi_ctx *ctx, mi_phase2 *S, const mi_fr *delta, const mi_fr *sigma_factor) {
    if (!ctx) return MI_EINVAL;
    if (!S) MI_FAIL(ctx, MI_EINVAL, "phase2: the state is null");
    if (!delta) MI_FAIL(ctx, MI_EINVAL, "phase2: delta is null");
    const Fr d = fr_of(*delta);
    if (d.is_zero()) MI_FAIL(ctx, MI_EINVAL, "phase2: delta is 0");
    std::vector<Fr> sf(S->n_commitments, Fr::one());
    for (u32 k = 0; k < S->n_commitments && sigma_factor; k++) {
        sf[k] = fr_of(sigma_factor[k]);
        if (sf[k].is_zero()) MI_FAIL(ctx, MI_EINVAL, "phase2: sigma_factor[" + std::to_string(k) + "] is 0");
    }
    const Fr d_inv = fe_inv(d);
    MI_TRY(scale_array<Fp>(ctx, (G1Aff *)S->g1_z, S->N, d_inv));
    MI_TRY(scale_array<Fp>(ctx, (G1Aff *)S->g1_k, S->n_k, d_inv));
    if (sigma_factor) MI_TRY(mi_phase2_scale_sigma(ctx, S, sf.data()));
    // the two delta points: one-point arrays through the same kernel
    Arena ar;
    G1Aff *d1 = nullptr;
    G2Aff *d2 = nullptr;
    MI_TRY(ar.alloc(ctx, &d1, (size_t)1));
    MI_TRY(ar.alloc(ctx, &d2, (size_t)1));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(d1, &S->delta1, 64, hipMemcpyHostToDevice, ctx->stream));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(d2, &S->delta2, 128, hipMemcpyHostToDevice, ctx->stream));
    MI_TRY(scale_array<Fp>(ctx, d1, 1, d));
    MI_TRY(scale_array<Fp2>(ctx, d2, 1, d));
    G1Aff n1;
    G2Aff n2;
    MI_CHECK_HIP(ctx, hipMemcpyAsync(&n1, d1, 64, hipMemcpyDeviceToHost, ctx->stream));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(&n2, d2, 128, hipMemcpyDeviceToHost, ctx->stream));
    MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    S->delta1 = n1; S->delta2 = n2;
    return MI_OK;
}

int32_t mi_phase2_seal(mi_ctx *ctx, const mi_phase2 *S, mi_pk **pk_out, mi_pedersen_pk **ped_out, mi_vk_out *vk_out) {
    if (!ctx) return MI_EINVAL;
    if (!pk_out) MI_FAIL(ctx, MI_EINVAL, "phase2: pk_out is null");
    *pk_out = nullptr;
    if (!S) MI_FAIL(ctx, MI_EINVAL, "phase2: the state is null");
    if (!vk_out) MI_FAIL(ctx, MI_EINVAL, "phase2: vk_out is null");
    if (S->n_commitments && !ped_out) MI_FAIL(ctx, MI_EINVAL, "phase2: ped_out is null");
    if (!vk_out->k || vk_out->k_cap < S->n_vk) MI_FAIL(ctx, MI_EINVAL, "phase2: vk_out.k / k_cap: room for nb_public + n_commitments points is needed");
    for (u32 k = 0; k < S->n_commitments; k++) ped_out[k] = nullptr;
    hipStream_t st = ctx->stream;
    KeyHandover hand(ctx, pk_out, ped_out);
    auto body = [&]() -> int32_t {
        Arena ar;
        auto copy = [&](void **dst, const void *src, size_t bytes) -> int32_t {
            MI_TRY(ar.alloc(ctx, dst, bytes));
            if (bytes) MI_CHECK_HIP(ctx, hipMemcpyAsync(*dst, src, bytes, hipMemcpyDeviceToDevice, st));
            return MI_OK;
        };
        MI_CHECK_HIP(ctx, hipMemcpyAsync(vk_out->k, S->vk_k, S->n_vk * 64, hipMemcpyDeviceToHost, st));
        for (u32 k = 0; k < S->n_commitments; k++) {
            void *basis = nullptr, *bes = nullptr;
            MI_TRY(copy(&basis, S->ped[k].basis, S->ped[k].n * 64));
            MI_TRY(copy(&bes, S->ped[k].bes, S->ped[k].n * 64));
            MI_CHECK_HIP(ctx, hipStreamSynchronize(st));
            MI_TRY(hand.adopt_pedersen(&basis, &bes, (size_t)S->ped[k].n, &ar));
        }
        KeyArrays ka = key_arrays_of(S);   // the key takes copies
        for (int i = 0; i < KEY_ARRAYS; i++) {
            const void *src = ka.arr[i];
            MI_TRY(copy(&ka.arr[i], src, ka.n[i] * (i == KEY_G2_B ? 128 : 64)));
        }
        MI_CHECK_HIP(ctx, hipStreamSynchronize(st));
        return hand.adopt_key(ka, &ar);
    };
    const int32_t rc = body();
    if (rc != MI_OK) { (void)hipStreamSynchronize(st); return rc; }
    hand.dismiss();
    std::memcpy(&vk_out->alpha1, &S->alpha1, 64);
    std::memcpy(&vk_out->beta2, &S->beta2, 128); std::memcpy(&vk_out->gamma2, &S->gamma2, 128); std::memcpy(&vk_out->delta2, &S->delta2, 128);
    vk_out->n_k = S->n_vk;
    return MI_OK;
}

int32_t mi_phase2_to_streams(mi_ctx *ctx, const mi_phase2 *S, uint32_t encoding, uint8_t *out_host, size_t cap, size_t *len, uint8_t *vk_out_host,
                             size_t vk_cap, size_t *vk_len) {
    if (!ctx) return MI_EINVAL;
    if (!S) MI_FAIL(ctx, MI_EINVAL, "phase2: the state is null");
    const KeyArrays ka = key_arrays_of(S);
    const mi_pk_desc d = ka.desc();
    std::vector<mi_pedersen_arrays> pa(S->n_commitments);
    std::vector<mi_pedersen_vk> pvk(S->n_commitments);
    for (u32 k = 0; k < S->n_commitments; k++) pa[k] = mi_pedersen_arrays{(const mi_g1_affine *)S->ped[k].basis, (const mi_g1_affine *)S->ped[k].bes, S->ped[k].n};
    mi_phase2_pedersen_vk_of(S, pvk.data());
    std::vector<mi_g1_affine> k_host(S->n_vk);
    const KeyStreams ks{encoding, out_host, cap, len, true, vk_out_host, vk_cap, vk_len};
    MI_TRY(ks.check(ctx, "phase2", d, pa.data(), S->n_commitments, S->n_vk));
    if (S->n_vk) MI_CHECK_HIP(ctx, hipMemcpyAsync(k_host.data(), S->vk_k, S->n_vk * 64, hipMemcpyDeviceToHost, ctx->stream));
    MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    MI_TRY(ks.write_vk_points(ctx, ka, k_host.data(), S->n_vk, pvk.data(), S->n_commitments));
    return mi_pk_write_dev(ctx, &d, pa.data(), S->n_commitments, encoding, out_host, cap, len);
}

int32_t mi_phase2_get_array(mi_ctx *ctx, const mi_phase2 *S, uint32_t which, void *out_host, uint64_t cap, uint64_t *n) {
    if (!ctx) return MI_EINVAL;
    if (!S || !n) MI_FAIL(ctx, MI_EINVAL, "phase2: the state or n is null");
    const void *src = nullptr;
    u64 cnt = 0, bytes = 64;
    switch (which) {
    case MI_PHASE2_G1_A: src = S->g1_a; cnt = S->n_a; break;
    case MI_PHASE2_G1_B: src = S->g1_b; cnt = S->n_b; break;
    case MI_PHASE2_G2_B: src = S->g2_b; cnt = S->n_b; bytes = 128; break;
    case MI_PHASE2_G1_K: src = S->g1_k; cnt = S->n_k; break;
    case MI_PHASE2_G1_Z: src = S->g1_z; cnt = S->N; break;
    case MI_PHASE2_VK_K: src = S->vk_k; cnt = S->n_vk; break;
    default: {
        const u32 k = (which - MI_PHASE2_BASIS) / 2;
        if (k >= S->n_commitments) MI_FAIL(ctx, MI_EINVAL, "phase2: which names no array of this state");
        src = (which - MI_PHASE2_BASIS) & 1 ? S->ped[k].bes : S->ped[k].basis; cnt = S->ped[k].n;
    }
    }
    *n = cnt;
    if (!out_host) return MI_OK;
    if (cap < cnt) MI_FAIL(ctx, MI_EINVAL, "phase2: the array holds " + std::to_string(cnt) + " points, out_host has room for " + std::to_string(cap));
    if (cnt) MI_CHECK_HIP(ctx, hipMemcpyAsync(out_host, src, cnt * bytes, hipMemcpyDeviceToHost, ctx->stream));
    MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MI_OK;
}

int32_t mi_phase2_get_pedersen_vk(mi_ctx *ctx, const mi_phase2 *S, mi_pedersen_vk *out) {
    if (!ctx) return MI_EINVAL;
    if (!S) MI_FAIL(ctx, MI_EINVAL, "phase2: the state is null");
    if (!out && S->n_commitments) MI_FAIL(ctx, MI_EINVAL, "phase2: out is null");
    mi_phase2_pedersen_vk_of(S, out);
    return MI_OK;
}

int32_t mi_phase2_free(mi_ctx *ctx, mi_phase2 *S) {
    if (!ctx || !S) return MI_EINVAL;
    (void)hipStreamSynchronize(ctx->stream);
    free_state(S);
    return MI_OK;
}

}  // extern "C"

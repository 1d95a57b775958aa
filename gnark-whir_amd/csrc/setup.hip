// groth16.Setup on the device (include/mi355x_groth16_setup.h): compiled R1CS + trapdoor -> device-resident proving key.
// Replaces the gnark call at mt.go:448 of the reference that the reference pays on every run.
//
//   1  L_i(tau) = lam w^i / (tau - w^i), lam = (tau^N - 1) / N, i < n_constraints          k_lagrange: strided runs of 64 rows per
//      thread, Montgomery's trick along the run, one Fermat inversion per run
//   2  the transposed sparse product M_j = sum_i M[i][j] L_i for M = A, B, C.  The matrices arrive by row, the sums are by column,
//      and there is no 256-bit atomic add.  Per matrix:
//        count    32-bit histogram of the column indices; every entry keeps the rank the atomic gave it inside its column
//        scan     exclusive prefix sum -> first slot of every column (scan_u32.cuh, the MSM's scan)
//        scatter  (row, coeff) of every entry to slot + rank (a counting sort by column; the order inside a column is whatever the
//                 atomics gave: field addition is exact and commutative, so every order gives the same bits)
//        sum      the split sum of sparse_fr.cuh (short columns by one lane, long ones cut into pieces, a wave per piece, a combine
//                 pass), planned here on the device because a column's length exists only after the histogram: k_col_sum_short
//                 sums the short columns and cuts the long ones, its counts stay in device memory (ctr) for the two wave passes
//      The count adds up a wave's entries of one column first (wave_claim): a hot column costs one atomic per wave instead of 64 on
//      one address.
//   3  element-wise: t_j = beta A_j + alpha B_j + C_j, t_j / delta, t_j / gamma, the zero tests; prefix sums compact the A_j / B_j / K_j
//      that own a key point into dense arrays; the Z exponents directly in the stored bit-reversed order
//   4  points: mi_batch_scalar_mul_g1/g2_dev (csrc/fixed_base.hip), then the arrays go to the key through key_handover.h (the adopt
//      path of mi_pk_load_range / mi_pedersen_pk_adopt).  Every exponent array is freed as soon as its points exist.
// Only the R1CS goes up; the infinity masks, the counts and the verifying key come down.
#include "prove_internal.h"
#include "r1cs_internal.h"
#include "key_handover.h"
#include "fp12.cuh"
#include "scan_u32.cuh"
#include "sparse_fr.cuh"
#include <algorithm>
#include <cstring>
#include <vector>

namespace {

constexpr u32 LAG_RUN = 64;    // rows per thread of k_lagrange: one inversion per run

// cnt[key] += 1 for every active lane; returns the value this lane's increment saw.  Lanes of one wave that share a key are served by
// ONE atomic: each round takes the first active lane's key, its lanes count themselves with a ballot, the lowest adds the count.
MI_D u32 wave_claim(u32 *cnt, u32 key) {
    const u32 lane = __lane_id();
    u32 res = 0;
    for (;;) {
        const u32 k0 = (u32)__builtin_amdgcn_readfirstlane((int)key);
        if (key == k0) {
            const u64 m = __ballot(1);
            const u32 rank = (u32)__popcll(m & (((u64)1 << lane) - 1));
            u32 base = 0;
            if (rank == 0) base = atomicAdd(&cnt[k0], (u32)__popcll(m));
            base = (u32)__builtin_amdgcn_readfirstlane((int)base);
            res = base + rank;
            break;
        }
    }
    return res;
}

// ---------------------------------------------------------------------------------------------------- 1: the Lagrange basis at tau
// thread t owns the rows t, t + T, t + 2T, ... (< nc): coalesced, and the run's w^i follow from one power and repeated steps of w^T
__global__ void __launch_bounds__(64) k_lagrange(Fr *L, u64 nc, u32 T, Fr w, Fr wT, Fr wTinv, Fr tau, Fr lam) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T || t >= nc) return;
    Fr x = fe_pow_u64(w, t), p = Fr::one();
    u32 cnt = 0;
    for (u64 i = t; i < nc && cnt < LAG_RUN; i += T, cnt++) {   // L[i] <- product of the run's earlier denominators
        st_fr(L + i, p);
        p = p * (tau - x);
        x = x * wT;
    }
    Fr inv = fe_inv(p);   // tau is not on the domain (refused on the host): no denominator is zero
    for (u32 k = cnt; k-- > 0;) {
        const u64 i = t + (u64)k * T;
        x = x * wTinv;
        const Fr dinv = inv * ld_fr(L + i);
        inv = inv * (tau - x);
        st_fr(L + i, (lam * x) * dinv);
    }
}

// ---------------------------------------------------------------------------------------------------- 2: the transposed sparse product
// rank[e] = how many entries of e's column were counted before it (any order: the atomics decide); cnt ends as the histogram
__global__ void __launch_bounds__(256) k_col_count(const u32 *col, u32 nnz, u32 *cnt, u32 *rank) {
    const u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < nnz) rank[e] = wave_claim(cnt, col[e]);
}
// four consecutive entries per thread: one binary search of the row starts, then a walk
__global__ void __launch_bounds__(256) k_col_scatter(const u32 *row_ptr, u32 n_rows, const u32 *col, const u32 *coeff, u32 nnz, const u32 *off,
                                                     const u32 *rank, uint2 *sorted) {
    const u64 e0 = ((u64)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (e0 >= nnz) return;
    u32 lo = 0, hi = n_rows;   // row_ptr[lo] <= e0 < row_ptr[hi]
    while (hi - lo > 1) {
        const u32 mid = lo + (hi - lo) / 2;
        if (row_ptr[mid] <= e0) lo = mid; else hi = mid;
    }
    u32 row = lo;
    for (u32 k = 0; k < 4; k++) {
        const u64 e = e0 + k;
        if (e >= nnz) break;
        while (row_ptr[row + 1] <= e) row++;   // empty rows in between
        const u32 key = col[e];
        const u32 pos = off[key] + rank[e];
        sorted[pos] = make_uint2(row, coeff[e]);
    }
}
// the term of an entry (row, coefficient) of a sorted column: coeffs[coefficient] * L[row]
struct ColTerm {
    const Fr *L, *coeffs;
    MI_D void operator()(Fr &acc, const uint2 en) const { acc = acc + ld_fr(coeffs + en.y) * ld_fr(L + en.x); }
};
// a short column is summed here; a long one claims its pieces: ctr[0] = pieces, ctr[1] = long columns
__global__ void __launch_bounds__(256) k_col_sum_short(Fr *out, u64 nb_wires, const u32 *off, const uint2 *sorted, ColTerm term, u32 *ctr, uint2 *pieces,
                                                       SparseLong *long_cols) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nb_wires) return;
    const u32 lo = off[j], len = off[j + 1] - lo;
    if (len <= SPARSE_SHORT) { st_fr(out + j, sparse_sum_short(sorted, lo, len, term)); return; }
    const u32 np = sparse_cut(lo, len, nullptr), first = atomicAdd(&ctr[0], np);
    long_cols[atomicAdd(&ctr[1], 1u)] = SparseLong{(u32)j, first, np, 0};
    sparse_cut(lo, len, pieces + first);
}
__global__ void __launch_bounds__(256) k_col_sum_pieces(Fr *partial, const u32 *ctr, const uint2 *pieces, const uint2 *sorted, ColTerm term) {
    sparse_sum_pieces(partial, pieces, ctr[0], sorted, term);
}
__global__ void __launch_bounds__(256) k_col_sum_combine(Fr *out, const u32 *ctr, const SparseLong *long_cols, const Fr *partial) {
    sparse_combine(out, long_cols, ctr[1], partial, false);
}

// ---------------------------------------------------------------------------------------------------- 3: element-wise
// keep_* = 1 where the wire owns a point of pk.G1.A / pk.G1.B (+ pk.G2.B) / pk.G1.K (private; the committed and commitment wires are
// cleared afterwards); WireSelection::scan turns all three into the compaction's slots
__global__ void __launch_bounds__(256) k_elementwise(const Fr *A, const Fr *B, const Fr *C, Fr *Kd, Fr *Kg, uint8_t *inf_a, uint8_t *inf_b,
                                                     u32 *keep_a, u32 *keep_b, u32 *keep_k, u64 nb_wires, u32 nb_public, Fr alpha, Fr beta,
                                                     Fr delta_inv, Fr gamma_inv) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nb_wires) return;
    const Fr a = ld_fr(A + j), b = ld_fr(B + j), c = ld_fr(C + j);
    const Fr t = beta * a + alpha * b + c;
    st_fr(Kd + j, t * delta_inv);
    st_fr(Kg + j, t * gamma_inv);
    const bool za = a.is_zero(), zb = b.is_zero();
    inf_a[j] = za; inf_b[j] = zb;
    keep_a[j] = !za; keep_b[j] = !zb; keep_k[j] = j >= nb_public;
}
__global__ void __launch_bounds__(256) k_gather_scale(Fr *dst, const Fr *src, const u32 *idx, u64 n, Fr factor) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) st_fr(dst + i, ld_fr(src + idx[i]) * factor);
}
struct TauPowers { Fr p[MI_SETUP_MAX_LOG_N + 1]; };   // tau^(2^k)
// slot s of the stored order holds tau^bitrev(s) (tau^N - 1) / delta
__global__ void __launch_bounds__(256) k_z_exps(Fr *Z, u32 log_n, Fr zt, TauPowers tp) {
    const u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >> log_n) return;
    const u32 i = log_n ? __brev((u32)s) >> (32 - log_n) : 0;
    Fr acc = zt;
    for (u32 k = 0; k < log_n; k++)
        if ((i >> k) & 1) acc = acc * tp.p[k];
    st_fr(Z + s, acc);
}

// ---------------------------------------------------------------------------------------------------- host side
// what the host derives from the inputs before any device work: the R1CS's shape (r1cs_internal.h, shared with the resident handle
// of r1cs.hip) and the trapdoor's part
struct Plan : R1csShape {
    Fr tau, alpha, beta, delta_inv, gamma_inv, lam, zt, w;
    TauPowers tp;
};

int32_t make_plan(mi_ctx *ctx, const mi_r1cs_desc *d, const mi_trapdoor *td, Plan &pl) {
    if (!d) MI_FAIL(ctx, MI_EINVAL, "setup: r1cs is null");
    if (!td) MI_FAIL(ctx, MI_EINVAL, "setup: trapdoor is null");
    MI_TRY(mi_r1cs_validate(ctx, "setup", d, pl));
    const u32 log_n = pl.log_n;
    // the trapdoor
    const Fr delta = fr_of(td->delta), gamma = fr_of(td->gamma);
    pl.tau = fr_of(td->tau); pl.alpha = fr_of(td->alpha); pl.beta = fr_of(td->beta);
    if (delta.is_zero()) MI_FAIL(ctx, MI_EINVAL, "setup: trapdoor.delta is 0");
    if (gamma.is_zero()) MI_FAIL(ctx, MI_EINVAL, "setup: trapdoor.gamma is 0");
    for (u32 k = 0; k < d->n_commitments; k++)
        if (fr_of(td->sigma[k]).is_zero()) MI_FAIL(ctx, MI_EINVAL, "setup: trapdoor.sigma[" + std::to_string(k) + "] is 0");
    Fr tn = pl.tau;
    for (u32 k = 0; k <= log_n; k++) { pl.tp.p[k] = tn; if (k < log_n) tn = fe_sqr(tn); }
    if (tn == Fr::one()) MI_FAIL(ctx, MI_EINVAL, "setup: trapdoor.tau lies on the domain (tau^N = 1)");
    pl.delta_inv = fe_inv(delta); pl.gamma_inv = fe_inv(gamma);
    const Fr zn = tn - Fr::one();
    pl.lam = zn * fe_inv(fe_from_u32<FrParams>((u32)pl.N));
    pl.zt = zn * pl.delta_inv;
    pl.w = fr_domain_generator(log_n);
    return MI_OK;
}

struct Timer {   // HIP events on the context's stream, one per phase boundary
    enum { UP0, UP1, LAG, SUM, ELEM, POINTS, DONE, COUNT };
    hipEvent_t ev[COUNT]{};
    bool have[COUNT]{};
    ~Timer() { for (auto e : ev) if (e) (void)hipEventDestroy(e); }
    int32_t init(mi_ctx *ctx) { for (auto &e : ev) MI_CHECK_HIP(ctx, hipEventCreate(&e)); return MI_OK; }
    int32_t mark(mi_ctx *ctx, int k) { MI_CHECK_HIP(ctx, hipEventRecord(ev[k], ctx->stream)); have[k] = true; return MI_OK; }
    float span(int a, int b) { float ms = 0; if (have[a] && have[b] && hipEventElapsedTime(&ms, ev[a], ev[b]) != hipSuccess) { (void)hipGetLastError(); ms = 0; } return ms; }
};

// the Fr half on the device: everything both entry points share
struct FrHalf {
    Fr *A = nullptr, *B = nullptr, *C = nullptr, *Kd = nullptr, *Kg = nullptr;
    uint8_t *inf_a = nullptr, *inf_b = nullptr;
    WireSelection sel;   // the compaction slots
    float sort_ms = 0, sum_ms = 0;
    u64 long_columns = 0, chunks = 0;
};

int32_t run_fr_half(mi_ctx *ctx, const mi_r1cs_desc *d, const Plan &pl, Arena &ar, Timer &tm, FrHalf &f) {
    const u64 nw = pl.nb_wires;
    hipStream_t st = ctx->stream;
    const u32 max_nnz = std::max(pl.nnz[0], std::max(pl.nnz[1], pl.nnz[2]));
    // ---- upload
    MI_TRY(tm.mark(ctx, Timer::UP0));
    Fr *coeffs = nullptr, *L = nullptr;
    MatrixSorter ms{d, &pl};
    MI_TRY(ar.alloc(ctx, &coeffs, (size_t)d->n_coeffs));
    if (d->n_coeffs) MI_CHECK_HIP(ctx, hipMemcpyAsync(coeffs, d->coeffs, d->n_coeffs * 32, hipMemcpyHostToDevice, st));
    MI_TRY(ar.alloc(ctx, &ms.row_ptr, (size_t)pl.nc + 1));
    MI_TRY(ar.alloc(ctx, &ms.col, (size_t)max_nnz));
    MI_TRY(ar.alloc(ctx, &ms.cf, (size_t)max_nnz));
    MI_TRY(tm.mark(ctx, Timer::UP1));
    // ---- 1: Lagrange
    MI_TRY(ar.alloc(ctx, &L, (size_t)pl.nc));
    if (pl.nc) {
        u64 T = (pl.nc + LAG_RUN - 1) / LAG_RUN;
        T = (T + 63) / 64 * 64;
        Fr wT = Fr::one(), b = pl.w;
        for (u64 e = T; e; e >>= 1) { if (e & 1) wT = wT * b; b = fe_sqr(b); }
        hipLaunchKernelGGL(k_lagrange, dim3((unsigned)(T / 64)), dim3(64), 0, st, L, pl.nc, (u32)T, pl.w, wT, fe_inv(wT), pl.tau, pl.lam);
        MI_CHECK_HIP(ctx, hipGetLastError());
    }
    MI_TRY(tm.mark(ctx, Timer::LAG));
    // ---- 2: the three transposed products, one after the other over the same scratch
    u32 *off = nullptr, *ctr = nullptr;
    uint2 *sorted = nullptr, *pieces = nullptr;
    SparseLong *long_cols = nullptr;
    Fr *partial = nullptr;
    const size_t cap_long = (size_t)max_nnz / SPARSE_SHORT + 1;   // a long column has more than SPARSE_SHORT entries and at most len / SPARSE_SHORT pieces
    MI_TRY(ar.alloc(ctx, &ms.cnt, (size_t)nw));
    MI_TRY(ar.alloc(ctx, &off, (size_t)nw + 1));
    MI_TRY(ar.alloc(ctx, &ms.rank, (size_t)max_nnz));
    MI_TRY(ar.alloc(ctx, &sorted, (size_t)max_nnz));
    MI_TRY(ar.alloc(ctx, &pieces, cap_long));
    MI_TRY(ar.alloc(ctx, &long_cols, cap_long));
    MI_TRY(ar.alloc(ctx, &partial, cap_long));
    MI_TRY(ar.alloc(ctx, &ctr, (size_t)8));
    MI_TRY(ar.alloc(ctx, &f.A, (size_t)nw));
    MI_TRY(ar.alloc(ctx, &f.B, (size_t)nw));
    MI_TRY(ar.alloc(ctx, &f.C, (size_t)nw));
    MI_CHECK_HIP(ctx, hipMemsetAsync(ctr, 0, 32, st));
    Fr *outs[3] = {f.A, f.B, f.C};
    // per matrix: e[0] upload e[1] sort e[2] sum e[3]
    struct Events { hipEvent_t e[4]{}; ~Events() { for (auto x : e) if (x) (void)hipEventDestroy(x); } } evs;
    for (auto &x : evs.e) MI_CHECK_HIP(ctx, hipEventCreate(&x));
    hipEvent_t e0 = evs.e[0], e1 = evs.e[1], e2 = evs.e[2], e3 = evs.e[3];
    const unsigned wave_grid = (unsigned)ctx->cu_count * 8;   // blocks of 4 waves for the grid-stride passes
    for (int k = 0; k < 3; k++) {
        MI_CHECK_HIP(ctx, hipEventRecord(e0, st));
        MI_TRY(ms.upload(ctx, st, k));
        MI_CHECK_HIP(ctx, hipEventRecord(e1, st));
        MI_TRY(ms.sort(ctx, st, k, off, sorted));
        MI_CHECK_HIP(ctx, hipEventRecord(e2, st));
        MI_CHECK_HIP(ctx, hipMemsetAsync(ctr, 0, 8, st));
        const ColTerm term{L, coeffs};
        hipLaunchKernelGGL(k_col_sum_short, dim3(mi_blocks_of(nw, 256)), dim3(256), 0, st, outs[k], nw, (const u32 *)off, (const uint2 *)sorted, term, ctr, pieces, long_cols);
        hipLaunchKernelGGL(k_col_sum_pieces, dim3(wave_grid), dim3(256), 0, st, partial, (const u32 *)ctr, (const uint2 *)pieces, (const uint2 *)sorted, term);
        hipLaunchKernelGGL(k_col_sum_combine, dim3(wave_grid), dim3(256), 0, st, outs[k], (const u32 *)ctr, (const SparseLong *)long_cols, (const Fr *)partial);
        MI_CHECK_HIP(ctx, hipGetLastError());
        u32 ctr_h[2] = {0, 0};
        MI_CHECK_HIP(ctx, hipMemcpyAsync(ctr_h, ctr, 8, hipMemcpyDeviceToHost, st));
        MI_CHECK_HIP(ctx, hipEventRecord(e3, st));
        MI_CHECK_HIP(ctx, hipStreamSynchronize(st));   // the host arrays of this matrix are not read after this point
        float ms = 0;
        if (hipEventElapsedTime(&ms, e1, e2) == hipSuccess) f.sort_ms += ms;
        if (hipEventElapsedTime(&ms, e2, e3) == hipSuccess) f.sum_ms += ms;
        if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) ctx->setup_stats.upload_ms += ms;
        f.chunks += ctr_h[0]; f.long_columns += ctr_h[1];
    }
    MI_TRY(tm.mark(ctx, Timer::SUM));
    for (void *p : {(void *)ms.row_ptr, (void *)ms.col, (void *)ms.cf, (void *)ms.cnt, (void *)off, (void *)ms.rank, (void *)sorted, (void *)pieces, (void *)long_cols, (void *)partial, (void *)L, (void *)coeffs, (void *)ctr})
        ar.release(p);
    // ---- 3: element-wise and the compaction slots
    MI_TRY(ar.alloc(ctx, &f.Kd, (size_t)nw));
    MI_TRY(ar.alloc(ctx, &f.Kg, (size_t)nw));
    MI_TRY(ar.alloc(ctx, &f.inf_a, (size_t)nw));
    MI_TRY(ar.alloc(ctx, &f.inf_b, (size_t)nw));
    f.sel.nb_wires = nw;
    MI_TRY(ar.alloc(ctx, &f.sel.slot_a, (size_t)nw + 1));
    MI_TRY(ar.alloc(ctx, &f.sel.slot_b, (size_t)nw + 1));
    MI_TRY(ar.alloc(ctx, &f.sel.slot_k, (size_t)nw + 1));
    hipLaunchKernelGGL(k_elementwise, dim3(mi_blocks_of(nw, 256)), dim3(256), 0, st, (const Fr *)f.A, (const Fr *)f.B, (const Fr *)f.C, f.Kd, f.Kg, f.inf_a, f.inf_b,
                       f.sel.slot_a, f.sel.slot_b, f.sel.slot_k, nw, pl.nb_public, pl.alpha, pl.beta, pl.delta_inv, pl.gamma_inv);
    MI_CHECK_HIP(ctx, hipGetLastError());
    MI_TRY(f.sel.scan(ctx, ar, pl.removed));
    MI_TRY(tm.mark(ctx, Timer::ELEM));
    return MI_OK;
}

int32_t z_exps_dev(mi_ctx *ctx, const Plan &pl, Fr *Z) {
    hipLaunchKernelGGL(k_z_exps, dim3(mi_blocks_of(pl.N, 256)), dim3(256), 0, ctx->stream, Z, pl.log_n, pl.zt, pl.tp);
    MI_CHECK_HIP(ctx, hipGetLastError());
    return MI_OK;
}

void fill_stats(mi_ctx *ctx, const Plan &pl, Timer &tm, const FrHalf &f, double total_ms) {
    mi_setup_stats &s = ctx->setup_stats;
    s.upload_ms += tm.span(Timer::UP0, Timer::UP1);
    s.lagrange_ms = tm.span(Timer::UP1, Timer::LAG);
    s.sparse_sort_ms = f.sort_ms; s.sparse_sum_ms = f.sum_ms; s.sparse_ms = f.sort_ms + f.sum_ms;
    s.elementwise_ms = tm.span(Timer::SUM, Timer::ELEM);
    s.points_ms = tm.span(Timer::ELEM, Timer::POINTS);
    s.handover_ms = tm.span(Timer::POINTS, Timer::DONE);
    s.total_ms = (float)total_ms;
    s.entries = (u64)pl.nnz[0] + pl.nnz[1] + pl.nnz[2];
    s.long_columns = f.long_columns; s.chunks = f.chunks;
}

}  // namespace

// r1cs_internal.h: one matrix up, then its counting sort by column; for phase2.hip too
int32_t MatrixSorter::upload(mi_ctx *ctx, hipStream_t st, int k) {
    const mi_r1cs_matrix *mats[3] = {&d->A, &d->B, &d->C};
    const u32 nnz = sh->nnz[k];
    MI_CHECK_HIP(ctx, hipMemcpyAsync(row_ptr, sh->row_ptr[k].data(), (sh->nc + 1) * 4, hipMemcpyHostToDevice, st));
    if (nnz) {
        MI_CHECK_HIP(ctx, hipMemcpyAsync(col, mats[k]->col, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
        MI_CHECK_HIP(ctx, hipMemcpyAsync(cf, mats[k]->coeff, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
    }
    return MI_OK;
}
int32_t MatrixSorter::sort(mi_ctx *ctx, hipStream_t st, int k, uint32_t *off, uint2 *sorted) {
    const u32 nnz = sh->nnz[k];
    const u64 nb_wires = sh->nb_wires;
    MI_CHECK_HIP(ctx, hipMemsetAsync(cnt, 0, nb_wires * 4, st));
    if (nnz) hipLaunchKernelGGL(k_col_count, dim3(mi_blocks_of(nnz, 256)), dim3(256), 0, st, (const u32 *)col, nnz, cnt, rank);
    MI_TRY(exclusive_scan(ctx, st, cnt, nb_wires, off, ctx->ws[WS_SCAN]));   // off[nb_wires] = the number of entries
    if (nnz) hipLaunchKernelGGL(k_col_scatter, dim3(mi_blocks_of(((u64)nnz + 3) / 4, 256)), dim3(256), 0, st, (const u32 *)row_ptr, (u32)sh->nc, (const u32 *)col,
                                (const u32 *)cf, nnz, (const u32 *)off, (const u32 *)rank, sorted);
    return MI_OK;
}

extern "C" {

int32_t mi_groth16_setup_get_stats(mi_ctx *ctx, mi_setup_stats *out) {
    if (!ctx || !out) return MI_EINVAL;
    *out = ctx->setup_stats;
    return MI_OK;
}

int32_t mi_groth16_setup_exponents(mi_ctx *ctx, const mi_r1cs_desc *r1cs, const mi_trapdoor *trapdoor, mi_setup_exponents *out) {
    if (!ctx) return MI_EINVAL;
    if (!out) MI_FAIL(ctx, MI_EINVAL, "setup: out is null");
    Plan pl;
    MI_TRY(make_plan(ctx, r1cs, trapdoor, pl));
    const double t0 = now_ms();
    ctx->setup_stats = mi_setup_stats{};
    Arena ar;
    Timer tm;
    FrHalf f;
    MI_TRY(tm.init(ctx));
    MI_TRY(run_fr_half(ctx, r1cs, pl, ar, tm, f));
    hipStream_t st = ctx->stream;
    const u64 nw = pl.nb_wires;
    const std::pair<void *, const void *> fetch[] = {{out->a, f.A}, {out->b, f.B}, {out->c, f.C}, {out->k, f.Kd}, {out->k_gamma, f.Kg}};
    for (const auto &p : fetch)
        if (p.first) MI_CHECK_HIP(ctx, hipMemcpyAsync(p.first, p.second, nw * 32, hipMemcpyDeviceToHost, st));
    if (out->infinity_a) MI_CHECK_HIP(ctx, hipMemcpyAsync(out->infinity_a, f.inf_a, nw, hipMemcpyDeviceToHost, st));
    if (out->infinity_b) MI_CHECK_HIP(ctx, hipMemcpyAsync(out->infinity_b, f.inf_b, nw, hipMemcpyDeviceToHost, st));
    if (out->z) {
        Fr *Z = nullptr;
        MI_TRY(ar.alloc(ctx, &Z, (size_t)pl.N));
        MI_TRY(z_exps_dev(ctx, pl, Z));
        MI_CHECK_HIP(ctx, hipMemcpyAsync(out->z, Z, pl.N * 32, hipMemcpyDeviceToHost, st));
    }
    MI_TRY(tm.mark(ctx, Timer::DONE));
    MI_CHECK_HIP(ctx, hipStreamSynchronize(st));
    fill_stats(ctx, pl, tm, f, now_ms() - t0);
    return MI_OK;
}

// groth16.Setup behind the three entry points.  ks (mi_groth16_setup_to_stream[s]; null for mi_groth16_setup): the key's stream is written
// from the plain arrays, right before the key takes them.  pk_out null (with ks only): no key is built and ped_out is not written.
static int32_t setup_run(mi_ctx *ctx, const mi_r1cs_desc *r1cs, const mi_trapdoor *trapdoor, const KeyStreams *ks, mi_pk **pk_out, mi_pedersen_pk **ped_out,
                         mi_vk_out *vk_out) {
    if (!ctx) return MI_EINVAL;
    if (!pk_out && !ks) MI_FAIL(ctx, MI_EINVAL, "setup: pk_out is null");
    if (pk_out) *pk_out = nullptr;
    if (!vk_out) MI_FAIL(ctx, MI_EINVAL, "setup: vk_out is null");
    const bool build = pk_out != nullptr;
    Plan pl;
    MI_TRY(make_plan(ctx, r1cs, trapdoor, pl));
    if (pl.n_commitments && !ped_out && build) MI_FAIL(ctx, MI_EINVAL, "setup: ped_out is null");
    if (!vk_out->k || vk_out->k_cap < pl.vk_wires.size()) MI_FAIL(ctx, MI_EINVAL, "setup: vk_out.k / k_cap: room for nb_public + n_commitments points is needed");
    for (u32 k = 0; k < pl.n_commitments && build; k++) ped_out[k] = nullptr;
    std::vector<mi_pedersen_arrays> ped_arrays;   // the plain Pedersen arrays, for the stream
    const double t0 = now_ms();
    ctx->setup_stats = mi_setup_stats{};
    const G1Aff g1 = g1_generator();
    const G2Aff g2 = g2_generator();
    hipStream_t st = ctx->stream;
    const u64 nw = pl.nb_wires;
    KeyHandover hand(ctx, pk_out, ped_out);
    auto body = [&]() -> int32_t {
        Arena ar;
        Timer tm;
        FrHalf f;
        MI_TRY(tm.init(ctx));
        MI_TRY(run_fr_half(ctx, r1cs, pl, ar, tm, f));
        // masks and counts to the host
        std::vector<uint8_t> ia(nw), ib(nw);
        WireSelection &sel = f.sel;
        MI_TRY(sel.fetch(ctx, f.inf_a, f.inf_b, ia.data(), ib.data()));
        ar.release(f.inf_a); ar.release(f.inf_b);
        KeyArrays ka(pl.log_n, pl.nb_public, nw, ia.data(), ib.data(), pl.removed.data(), pl.removed.size());
        ka.n[KEY_G1_A] = sel.n_a; ka.n[KEY_G1_B] = ka.n[KEY_G2_B] = sel.n_b; ka.n[KEY_G1_K] = sel.n_k; ka.n[KEY_G1_Z] = pl.N;
        if (ks) {   // the counts are known: a buffer that cannot hold the stream is refused before the points are computed
            std::vector<mi_pedersen_arrays> pc(pl.n_commitments);
            for (u32 k = 0; k < pl.n_commitments; k++) pc[k] = mi_pedersen_arrays{nullptr, nullptr, r1cs->n_committed[k]};
            MI_TRY(ks->check(ctx, "setup", ka.desc(), pc.data(), pl.n_commitments, pl.vk_wires.size()));
        }
        // dense scalar arrays; each per-wire array goes as soon as it has been read
        Fr *sa = nullptr, *sb = nullptr, *sk = nullptr;
        auto compact = [&](Fr **dst, Fr *src, u32 *slot, u32 n) -> int32_t {
            MI_TRY(ar.alloc(ctx, dst, (size_t)n));
            MI_TRY(sel.compact(ctx, *dst, src, slot, sizeof(Fr)));
            MI_CHECK_HIP(ctx, hipGetLastError());
            MI_CHECK_HIP(ctx, hipStreamSynchronize(st));
            ar.release(src); ar.release(slot);
            return MI_OK;
        };
        MI_TRY(compact(&sa, f.A, sel.slot_a, sel.n_a));
        MI_TRY(compact(&sb, f.B, sel.slot_b, sel.n_b));
        ar.release(f.C);
        MI_TRY(compact(&sk, f.Kd, sel.slot_k, sel.n_k));
        // a batch of points from device scalars into a fresh array
        auto mul_g1 = [&](void **dst, const Fr *sc, size_t n) -> int32_t {
            MI_TRY(ar.alloc(ctx, dst, n * 64));
            return mi_batch_scalar_mul_g1_dev(ctx, (const mi_g1_affine *)&g1, (const mi_fr *)sc, n, (mi_g1_affine *)*dst);
        };
        auto gather = [&](Fr **dst, const u32 *wires, size_t n, const Fr &factor) -> int32_t {
            u32 *idx = nullptr;
            MI_TRY(ar.alloc(ctx, &idx, n));
            MI_TRY(ar.alloc(ctx, dst, n));
            if (n) {
                MI_CHECK_HIP(ctx, hipMemcpyAsync(idx, wires, n * 4, hipMemcpyHostToDevice, st));
                hipLaunchKernelGGL(k_gather_scale, dim3(mi_blocks_of(n, 256)), dim3(256), 0, st, *dst, (const Fr *)f.Kg, (const u32 *)idx, (u64)n, factor);
                MI_CHECK_HIP(ctx, hipGetLastError());
            }
            MI_CHECK_HIP(ctx, hipStreamSynchronize(st));
            ar.release(idx);
            return MI_OK;
        };
        // ---- 4: points.  vk.G1.K and the Pedersen bases first: they read t / gamma, which can go afterwards
        {
            Fr *sv = nullptr;
            void *pv = nullptr;
            const size_t n = pl.vk_wires.size();
            MI_TRY(gather(&sv, pl.vk_wires.data(), n, Fr::one()));
            MI_TRY(mul_g1(&pv, sv, n));
            MI_CHECK_HIP(ctx, hipMemcpyAsync(vk_out->k, pv, n * 64, hipMemcpyDeviceToHost, st));
            MI_CHECK_HIP(ctx, hipStreamSynchronize(st));
            vk_out->n_k = n;
            ar.release(sv); ar.release(pv);
        }
        for (u32 k = 0; k < pl.n_commitments; k++) {
            Fr *s0 = nullptr, *s1 = nullptr;
            void *basis = nullptr, *bes = nullptr;
            const size_t n = (size_t)r1cs->n_committed[k];
            MI_TRY(gather(&s0, r1cs->committed[k], n, Fr::one()));
            MI_TRY(gather(&s1, r1cs->committed[k], n, fr_of(trapdoor->sigma[k])));
            MI_TRY(mul_g1(&basis, s0, n));
            MI_TRY(mul_g1(&bes, s1, n));
            MI_CHECK_HIP(ctx, hipStreamSynchronize(st));
            ar.release(s0); ar.release(s1);
            ped_arrays.push_back(mi_pedersen_arrays{(const mi_g1_affine *)basis, (const mi_g1_affine *)bes, n});
            if (!build) continue;   // write only: the arrays stay the arena's
            MI_TRY(hand.adopt_pedersen(&basis, &bes, n, &ar));
        }
        ar.release(f.Kg);
        // alpha, beta, delta on G1; beta, delta, gamma on G2
        {
            const Fr sc[4] = {pl.alpha, pl.beta, fr_of(trapdoor->delta), fr_of(trapdoor->gamma)};
            Fr *ds = nullptr;
            void *p1 = nullptr, *p2 = nullptr;
            MI_TRY(ar.alloc(ctx, &ds, (size_t)4));
            MI_CHECK_HIP(ctx, hipMemcpyAsync(ds, sc, sizeof(sc), hipMemcpyHostToDevice, st));
            MI_TRY(mul_g1(&p1, ds, 3));
            MI_TRY(ar.alloc(ctx, &p2, (size_t)3 * 128));
            MI_TRY(mi_batch_scalar_mul_g2_dev(ctx, (const mi_g2_affine *)&g2, (const mi_fr *)(ds + 1), 3, (mi_g2_affine *)p2));
            MI_CHECK_HIP(ctx, hipMemcpyAsync(ka.small1, p1, sizeof(ka.small1), hipMemcpyDeviceToHost, st));
            MI_CHECK_HIP(ctx, hipMemcpyAsync(ka.small2, p2, sizeof(ka.small2), hipMemcpyDeviceToHost, st));
            MI_CHECK_HIP(ctx, hipStreamSynchronize(st));
            ar.release(ds); ar.release(p1); ar.release(p2);
        }
        std::memcpy(&vk_out->alpha1, &ka.small1[0], 64);
        std::memcpy(&vk_out->beta2, &ka.small2[0], 128); std::memcpy(&vk_out->delta2, &ka.small2[1], 128); std::memcpy(&vk_out->gamma2, &ka.small2[2], 128);
        // the verifying key's stream: everything it holds is on the host here
        if (ks && ks->with_vk) MI_TRY(ks->write_vk(ctx, ka, vk_out->k, vk_out->n_k, trapdoor->sigma, pl.n_commitments));
        // the five arrays of the key
        MI_TRY(mul_g1(&ka.arr[KEY_G1_A], sa, sel.n_a));
        MI_CHECK_HIP(ctx, hipStreamSynchronize(st));
        ar.release(sa);
        MI_TRY(mul_g1(&ka.arr[KEY_G1_B], sb, sel.n_b));
        MI_TRY(ar.alloc(ctx, &ka.arr[KEY_G2_B], (size_t)sel.n_b * 128));
        MI_TRY(mi_batch_scalar_mul_g2_dev(ctx, (const mi_g2_affine *)&g2, (const mi_fr *)sb, sel.n_b, (mi_g2_affine *)ka.arr[KEY_G2_B]));
        MI_CHECK_HIP(ctx, hipStreamSynchronize(st));
        ar.release(sb);
        MI_TRY(mul_g1(&ka.arr[KEY_G1_K], sk, sel.n_k));
        MI_CHECK_HIP(ctx, hipStreamSynchronize(st));
        ar.release(sk);
        {
            Fr *Z = nullptr;
            MI_TRY(ar.alloc(ctx, &Z, (size_t)pl.N));
            MI_TRY(z_exps_dev(ctx, pl, Z));
            MI_TRY(mul_g1(&ka.arr[KEY_G1_Z], Z, pl.N));
            MI_CHECK_HIP(ctx, hipStreamSynchronize(st));
            ar.release(Z);
        }
        MI_TRY(tm.mark(ctx, Timer::POINTS));
        // ---- the key takes the arrays
        if (ks) {
            const mi_pk_desc d = ka.desc();
            MI_TRY(mi_pk_write_dev(ctx, &d, ped_arrays.data(), pl.n_commitments, ks->encoding, ks->out, ks->cap, ks->len));
        }
        if (build) MI_TRY(hand.adopt_key(ka, &ar));
        MI_TRY(tm.mark(ctx, Timer::DONE));
        MI_CHECK_HIP(ctx, hipStreamSynchronize(st));
        fill_stats(ctx, pl, tm, f, now_ms() - t0);
        return MI_OK;
    };
    const int32_t rc = body();
    if (rc == MI_OK) hand.dismiss();
    else (void)hipStreamSynchronize(st);
    return rc;
}
int32_t mi_groth16_setup(mi_ctx *ctx, const mi_r1cs_desc *r1cs, const mi_trapdoor *trapdoor, mi_pk **pk_out, mi_pedersen_pk **ped_out, mi_vk_out *vk_out) {
    return setup_run(ctx, r1cs, trapdoor, nullptr, pk_out, ped_out, vk_out);
}
int32_t mi_groth16_setup_to_stream(mi_ctx *ctx, const mi_r1cs_desc *r1cs, const mi_trapdoor *trapdoor, uint32_t encoding, uint8_t *out_host, size_t cap,
                                   size_t *len, mi_pk **pk_out, mi_pedersen_pk **ped_out, mi_vk_out *vk_out) {
    const KeyStreams ks{encoding, out_host, cap, len};
    return setup_run(ctx, r1cs, trapdoor, &ks, pk_out, ped_out, vk_out);
}
int32_t mi_groth16_setup_to_streams(mi_ctx *ctx, const mi_r1cs_desc *r1cs, const mi_trapdoor *trapdoor, uint32_t encoding, uint8_t *out_host, size_t cap,
                                    size_t *len, uint8_t *vk_out_host, size_t vk_cap, size_t *vk_len, mi_pk **pk_out, mi_pedersen_pk **ped_out,
                                    mi_vk_out *vk_out) {
    const KeyStreams ks{encoding, out_host, cap, len, true, vk_out_host, vk_cap, vk_len};
    return setup_run(ctx, r1cs, trapdoor, &ks, pk_out, ped_out, vk_out);
}

}  // extern "C"

// Sparse sums of curve points (include/mi355x_groth16_phase2.h): [M_j] = sum_i M[i][j] [L_i], Setup's transposed sparse product "in the
// exponent".  The entries are setup.hip's, sorted by column by setup.hip's sort; the split of skewed columns is sparse_fr.cuh's
// (SPARSE_SHORT, SPARSE_CHUNK, sparse_cut, SparseLong) with a point accumulator:
//   short   a lane per column sums the lists of at most SPARSE_SHORT entries and cuts the longer ones        sparse_points_short
//   pieces  a wave per piece, its lanes striding over it and meeting in a butterfly of XYZZ additions         sparse_points_pieces
//   combine a wave per long list adds its partials INTO the column's sum                                      sparse_points_combine
// A column's sum can be fed from several (matrix, basis) pairs -- [t_j] takes (A, [beta L]), (B, [alpha L]), (C, [L]) -- into ONE
// accumulator: the short pass walks all of them, the long lists of each pair are cut, summed and combined pair by pair.
// An entry contributes coeff * P_row (sparse_point_term): coefficient 1 and r - 1 are a mixed addition or subtraction, c or r - c below
// 2^32 goes through xyzz_mul_u32, everything else through double-and-add over the coefficient's true bit length.
// Group addition is exact and commutative and an affine point has one encoding: every order gives the same bytes.  Sums pass through
// infinity, doubling and cancellation (c and r - c on one wire in one row): only the complete operations of curve.cuh are used.
// The term and the short sum are MI_HD (tests/cpp/phase2_host.cpp runs them on the host); the wave passes are device code.
#pragma once
#include "point_ntt.cuh"

// acc += coeff * p; p affine ((0, 0) = infinity), coeff in Montgomery form
template <class F>
MI_HD void sparse_point_term(XYZZ<F> &acc, const Affine<F> &p, const Fr &coeff_mont) {
    if (p.is_inf()) return;
    const ScalarPath sp = scalar_path(coeff_mont);
    switch (sp.kind) {
    case ScalarPath::ZERO: return;
    case ScalarPath::ONE: xyzz_madd(acc, p, false); return;
    case ScalarPath::MINUS_ONE: xyzz_madd(acc, p, true); return;
    case ScalarPath::SMALL: xyzz_add(acc, xyzz_mul_u32(XYZZ<F>::from_affine(p), sp.c.l[0])); return;
    case ScalarPath::SMALL_NEG: xyzz_add(acc, xyzz_neg(xyzz_mul_u32(XYZZ<F>::from_affine(p), sp.c.l[0]))); return;
    default: xyzz_add(acc, xyzz_mul_bits(XYZZ<F>::from_affine(p), sp.c.l)); return;
    }
}
// the term of an entry (row, coefficient index) of a sorted column: coeffs[coefficient] * basis[bitrev(row)] (point_ntt.cuh leaves the
// Lagrange basis in bit-reversed order)
template <class F>
struct PointTerm {
    const Affine<F> *basis;
    const Fr *coeffs;
    u32 log_n;
    MI_HD void operator()(XYZZ<F> &acc, u32 row, u32 coeff) const { sparse_point_term(acc, basis[bitrev_u32(row, log_n)], coeffs[coeff]); }
};
// one lane: acc += the entries [lo, lo + len) of a sorted column, entry e = (row[e], coeff[e])
template <class F, class Entries>
MI_HD void sparse_points_run(XYZZ<F> &acc, const Entries &entries, u32 lo, u32 len, const PointTerm<F> &term) {
    for (u32 e = lo; e < lo + len; e++) term(acc, entries.row(e), entries.coeff(e));
}

#if defined(__HIPCC__)
#include "sparse_fr.cuh"

struct SortedEntries {   // setup.hip's sorted array: (row, coefficient index)
    const uint2 *p;
    MI_D u32 row(u32 e) const { return p[e].x; }
    MI_D u32 coeff(u32 e) const { return p[e].y; }
};
// the sum of v over the 64 lanes of a wave, in every lane (all lanes active)
template <class F>
MI_D XYZZ<F> wave_sum_points(XYZZ<F> v) {
    constexpr int W = sizeof(XYZZ<F>) / 4;
#pragma unroll 1
    for (int o = 32; o >= 1; o >>= 1) {
        XYZZ<F> t;
        const u32 *src = reinterpret_cast<const u32 *>(&v);
        u32 *dst = reinterpret_cast<u32 *>(&t);
#pragma unroll
        for (int i = 0; i < W; i++) dst[i] = (u32)__shfl_xor((int)src[i], o);
        xyzz_add(v, t);
    }
    return v;
}
// one (matrix, basis) pair of a sum: the matrix's sorted entries and column starts, the term, and where the plan of its long columns
// goes (ctr[0] = pieces, ctr[1] = long columns, both zero before the short pass)
template <class F>
struct PointSource {
    const u32 *off;
    SortedEntries sorted;
    PointTerm<F> term;
    u32 *ctr;
    uint2 *pieces;
    SparseLong *long_cols;
};
template <class F, int NS>
struct PointSources { PointSource<F> s[NS]; };
// column j (one lane): the short lists of every pair are summed here, the long ones claim their pieces
template <class F, int NS>
MI_D XYZZ<F> sparse_points_short(const PointSources<F, NS> &src, u32 j) {
    XYZZ<F> acc = XYZZ<F>::inf();
#pragma unroll 1
    for (int m = 0; m < NS; m++) {
        const PointSource<F> &ps = src.s[m];
        const u32 lo = ps.off[j], len = ps.off[j + 1] - lo;
        if (len <= SPARSE_SHORT) { sparse_points_run(acc, ps.sorted, lo, len, ps.term); continue; }
        const u32 np = sparse_cut(lo, len, nullptr), first = atomicAdd(&ps.ctr[0], np);
        ps.long_cols[atomicAdd(&ps.ctr[1], 1u)] = SparseLong{j, first, np, 0};
        sparse_cut(lo, len, ps.pieces + first);
    }
    return acc;
}
// a wave per piece (grid-stride over whole waves): partial[piece] = the sum of its entries
template <class F>
MI_D void sparse_points_pieces(XYZZ<F> *partial, const PointSource<F> &ps) {
    const u32 lane = threadIdx.x & 63, wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    const u32 n_pieces = ps.ctr[0];
    for (u32 it = wave; it < n_pieces; it += n_waves) {
        const uint2 pc = ps.pieces[it];
        XYZZ<F> acc = XYZZ<F>::inf();
        for (u32 k = lane; k < pc.y; k += 64) ps.term(acc, ps.sorted.row(pc.x + k), ps.sorted.coeff(pc.x + k));
        acc = wave_sum_points(acc);
        if (lane == 0) partial[it] = acc;
    }
}
// a wave per long list (grid-stride): out[the list's column] += the sum of its partials
template <class F>
MI_D void sparse_points_combine(XYZZ<F> *out, const PointSource<F> &ps, const XYZZ<F> *partial) {
    const u32 lane = threadIdx.x & 63, wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    const u32 n_long = ps.ctr[1];
    for (u32 it = wave; it < n_long; it += n_waves) {
        const SparseLong ll = ps.long_cols[it];
        XYZZ<F> acc = XYZZ<F>::inf();
        for (u32 k = lane; k < ll.n_pieces; k += 64) xyzz_add(acc, partial[ll.first_piece + k]);
        acc = wave_sum_points(acc);
        if (lane == 0) {
            XYZZ<F> o = out[ll.index];
            xyzz_add(o, acc);
            out[ll.index] = o;
        }
    }
}
#endif

// The inverse NTT over curve points (include/mi355x_groth16_phase2.h): [L_i] = (1 / N) sum_k w^(-i k) [tau^k], the Lagrange basis "in the
// exponent", for G1 (F = Fp) and G2 (F = Fp2).  What one lane does, MI_HD so that the host build of the tests (tests/cpp/phase2_host.cpp)
// runs the same text; the __global__ wrappers are phase2.hip's.
//
//   radix 2, decimation in frequency, in place over N XYZZ points: natural order in, BIT-REVERSED order out (the readers index by
//   bit-reversed row: sparse_points.cuh).  Stage s = 0 .. log_n - 1 pairs i0 = blk * 2 h + j with i1 = i0 + h, h = N >> (s + 1):
//       a[i0] <- k_top (a[i0] + a[i1])          a[i1] <- k_bot (a[i0] - a[i1])
//   with k_bot = w^(-j 2^s) and k_top = 1, but for stage 0, which carries the 1 / N: k_top = 1 / N, k_bot = w^(-j) / N (N / 2 extra
//   scalar multiplications instead of the N of a scaling pass).  A factor of 1 costs nothing and one of r - 1 a negation: the last stage
//   (h = 1: every twiddle is 1) and lane j = 0 of every stage multiply nothing.
//   The scalar multiplication is double-and-add over the scalar's true bit length, in plain integers.
//   The operands are the SRS's: sums can be infinity, the two inputs of a butterfly can be equal or opposite.  Only the complete
//   operations of curve.cuh are used (xyzz_add: infinity, doubling and cancellation all handled).
#pragma once
#include "curve.cuh"

// bits of a plain 8 x u32 integer (0 for 0)
MI_HD int u256_bit_length(const u32 k[8]) {
    for (int i = 7; i >= 0; i--)
        if (k[i]) {
            int b = 31;
            while (!((k[i] >> b) & 1)) b--;
            return 32 * i + b + 1;
        }
    return 0;
}
MI_HD bool u256_fits_u32(const u32 k[8]) { return (k[1] | k[2] | k[3] | k[4] | k[5] | k[6] | k[7]) == 0; }
// k * p for a plain integer k, over k's own bit length
template <class F>
MI_HD XYZZ<F> xyzz_mul_bits(const XYZZ<F> &p, const u32 k[8]) {
    const int n = u256_bit_length(k);
    if (n == 0) return XYZZ<F>::inf();
    XYZZ<F> acc = p;
    for (int i = n - 2; i >= 0; i--) {
        acc = xyzz_dbl(acc);
        if ((k[i >> 5] >> (i & 31)) & 1) xyzz_add(acc, p);
    }
    return acc;
}
// How a scalar (Montgomery Fr) multiplies a point: by nothing (1), by a negation (r - 1), by xyzz_mul_u32 on c or r - c below 2^32, or
// by the full double-and-add.  One classification for the transform's twiddles and the sparse sums' coefficients.
struct ScalarPath {
    enum Kind { ZERO, ONE, MINUS_ONE, SMALL, SMALL_NEG, FULL } kind;
    Fr c;   // the plain integer that multiplies: the scalar (SMALL, FULL) or r minus it (SMALL_NEG)
};
MI_HD ScalarPath scalar_path(const Fr &s_mont) {
    ScalarPath sp;
    sp.c = fe_from_mont(s_mont);
    Fr neg;
    fe_sub_raw(neg, Fr::modulus(), sp.c);   // r - c as a plain integer (c < r)
    const bool c32 = u256_fits_u32(sp.c.l), n32 = u256_fits_u32(neg.l);
    if (sp.c.is_zero()) sp.kind = ScalarPath::ZERO;
    else if (c32 && sp.c.l[0] == 1) sp.kind = ScalarPath::ONE;
    else if (n32 && neg.l[0] == 1) sp.kind = ScalarPath::MINUS_ONE;
    else if (c32) sp.kind = ScalarPath::SMALL;
    else if (n32) { sp.kind = ScalarPath::SMALL_NEG; sp.c = neg; }
    else sp.kind = ScalarPath::FULL;
    return sp;
}
// s * p
template <class F>
MI_HD XYZZ<F> xyzz_scale(const XYZZ<F> &p, const Fr &s_mont) {
    const ScalarPath sp = scalar_path(s_mont);
    switch (sp.kind) {
    case ScalarPath::ZERO: return XYZZ<F>::inf();
    case ScalarPath::ONE: return p;
    case ScalarPath::MINUS_ONE: return xyzz_neg(p);
    case ScalarPath::SMALL: return xyzz_mul_u32(p, sp.c.l[0]);
    case ScalarPath::SMALL_NEG: return xyzz_neg(xyzz_mul_u32(p, sp.c.l[0]));
    default: return xyzz_mul_bits(p, sp.c.l);
    }
}

// bit reversal of i over log_n bits
MI_HD u32 bitrev_u32(u32 i, u32 log_n) {
    u32 r = 0;
    for (u32 k = 0; k < log_n; k++) r |= ((i >> k) & 1u) << (log_n - 1 - k);
    return r;
}

// one butterfly, in place: *pa <- k_top (a + b), *pb <- k_bot (a - b).  The difference is parked in *pb while the sum is multiplied and
// fetched again afterwards: two points and the temporaries of one operation are live at a time, not three (G2: 64 words a point).
template <class F>
MI_HD void point_butterfly(XYZZ<F> *pa, XYZZ<F> *pb, const Fr &k_top, const Fr &k_bot) {
    XYZZ<F> a = *pa, b = *pb;
    XYZZ<F> u = a;
    xyzz_add(u, b);             // a + b
    b = xyzz_neg(b);
    xyzz_add(a, b);             // a - b
    *pb = a;
    *pa = xyzz_scale(u, k_top);
    const XYZZ<F> d = *pb;
    *pb = xyzz_scale(d, k_bot);
}
// butterfly t (< N / 2) of stage s over a[0 .. N); tw[m] = w^(-m) (Montgomery), m < N / 2; scale = 1 / N in stage 0, 1 afterwards
template <class F>
MI_HD void point_ntt_stage_lane(XYZZ<F> *a, u32 log_n, u32 s, u64 t, const Fr *tw, const Fr &scale) {
    const u64 h = ((u64)1 << log_n) >> (s + 1);
    const u64 blk = t / h, j = t % h;
    const u64 i0 = blk * 2 * h + j;
    point_butterfly(a + i0, a + i0 + h, scale, tw[j << s] * scale);
}

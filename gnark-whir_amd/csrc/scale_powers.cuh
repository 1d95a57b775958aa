// out[i] = [c t^(k0 + i)] P[i]: the scalar multiplication of a phase-1 contribution (include/mi355x_groth16_phase1.h), every lane its own
// dense scalar, for G1 (F = Fp) and G2 (F = Fp2).  What one lane does, MI_HD so that the host build of the tests
// (tests/cpp/phase1_host.cpp) runs the same text; the __global__ wrappers and the chunk driver are phase1.hip's.
//
// xyzz_mul_bits (point_ntt.cuh) branches on every bit of the scalar: 64 lanes with 64 different scalars pay a doubling AND an addition
// at every bit.  Here every lane runs the same sequence:
//   scalar   s = c t^(k0 + i) is made in the lane (fe_pow_u64), taken out of Montgomery form: a plain integer below r < 2^254
//   recode   D = ceil(255 / W) signed digits d_j with s = sum_j d_j 2^(W j), d_j in [-(2^(W-1) - 1), 2^(W-1)].  Digit j is stored as
//            e_j = d_j + 2^(W-1) - 1 in [0, 2^W): the carry chain of the recoding is then ONE 256-bit addition of the constant
//            B = sum_j (2^(W-1) - 1) 2^(W j), E = s + B, and e_j is window j of E.  B < 2^(W D - 1) and s < 2^254 <= 2^(W D - 1), so E fits
//            W D bits for EVERY s below 2^254: bit 254 is the room the last carry takes.
//   digits   E sits in eight registers, moved up so that window D - 1 ends at bit 255; a digit is the top W bits, then the eight words
//            shift left by W: constant indices only, nothing goes to scratch memory
//   table    T[m] = (m + 1) P, m < 2^(W-1), XYZZ, in a workspace of the call, lane-interleaved: entry m of lane l is tab[m * lanes + l],
//            so the lanes of a wave that read one entry index read neighbouring points
//   ladder   acc = infinity; per digit from the top: W doublings, then acc += +/- T[|d| - 1], skipped under a predicate when d = 0.
//            Only the complete operations of curve.cuh: leading zero digits double infinity, 2^W acc can meet a table entry (xyzz_add
//            doubles or cancels), a point at infinity has a table of infinities and comes out as infinity.
#pragma once
#include "curve.cuh"

template <int W> struct ScalePowers {
    static_assert(W >= 2 && W <= 5, "window widths 2..5");
    static constexpr int digits = (255 + W - 1) / W;
    static constexpr int entries = 1 << (W - 1);
    static constexpr u32 offset = (1u << (W - 1)) - 1;     // e_j = d_j + offset
    static constexpr int lift = 256 - W * digits;          // window D - 1 ends at bit 255 after a shift by this (0 or 1)
    // word i of B
    static constexpr u32 bias_word(int i) {
        u64 acc = 0;   // the windows that touch bits [32 i, 32 i + 32)
        for (int j = 0; j < digits; j++) {
            const int lo = W * j - 32 * i;
            if (lo > -W && lo < 32) acc |= lo >= 0 ? ((u64)offset << lo) : ((u64)offset >> -lo);
        }
        return (u32)acc;
    }
};

// the scalar of lane i: c t^k as a plain integer
MI_HD void scale_powers_scalar(const Fr &t, const Fr &c, u64 k, u32 out[8]) {
    const Fr s = fe_from_mont(fe_pow_u64(t, k) * c);
#pragma unroll
    for (int i = 0; i < 8; i++) out[i] = s.l[i];
}
// e <- (s + B) << lift, s a plain integer below 2^254
template <int W>
MI_HD void scale_powers_recode(const u32 s[8], u32 e[8]) {
    typedef ScalePowers<W> SP;
    constexpr u32 b[8] = {SP::bias_word(0), SP::bias_word(1), SP::bias_word(2), SP::bias_word(3), SP::bias_word(4), SP::bias_word(5), SP::bias_word(6), SP::bias_word(7)};
    u64 carry = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        carry += (u64)s[i] + b[i];
        e[i] = (u32)carry;
        carry >>= 32;
    }
    if constexpr (SP::lift != 0) {
#pragma unroll
        for (int i = 7; i > 0; i--) e[i] = (e[i] << SP::lift) | (e[i - 1] >> (32 - SP::lift));
        e[0] <<= SP::lift;
    }
}
// the top digit of e, which then moves up by one window
template <int W>
MI_HD int scale_powers_next_digit(u32 e[8]) {
    const int d = (int)(e[7] >> (32 - W)) - (int)ScalePowers<W>::offset;
#pragma unroll
    for (int i = 7; i > 0; i--) e[i] = (e[i] << W) | (e[i - 1] >> (32 - W));
    e[0] <<= W;
    return d;
}
// the table of one lane: tab[m * stride] = (m + 1) p
template <class F, int W>
MI_HD void scale_powers_table_lane(XYZZ<F> *tab, u64 stride, const Affine<F> &p) {
    const XYZZ<F> base = XYZZ<F>::from_affine(p);
    XYZZ<F> acc = base;
    tab[0] = acc;
    for (int m = 1; m < ScalePowers<W>::entries; m++) {
        xyzz_add(acc, base);   // m = 1 meets acc = base: the complete addition doubles
        tab[(u64)m * stride] = acc;
    }
}
// [s] p from that table, s a plain integer below 2^254
template <class F, int W>
MI_HD XYZZ<F> scale_powers_ladder_lane(const XYZZ<F> *tab, u64 stride, const u32 s[8]) {
    u32 e[8];
    scale_powers_recode<W>(s, e);
    XYZZ<F> acc = XYZZ<F>::inf();
    for (int j = 0; j < ScalePowers<W>::digits; j++) {
        for (int i = 0; i < W; i++) acc = xyzz_dbl(acc);
        const int d = scale_powers_next_digit<W>(e);
        if (d != 0) {   // a predicate over the same instructions in every lane
            const u32 mag = (u32)(d < 0 ? -d : d);
            XYZZ<F> q = tab[(u64)(mag - 1) * stride];
            if (d < 0) q = xyzz_neg(q);
            xyzz_add(acc, q);
        }
    }
    return acc;
}

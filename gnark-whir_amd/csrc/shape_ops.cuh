// Test records of the field arithmetic on OPERAND SHAPES the compiler can see through: literal factors, limbs that are provably zero, one
// value in two operand positions, a result written over one of its inputs, chains that start at a literal.  The per-primitive tests
// (mi_field_op_dev, lazy_ops.cuh, limb29_ops.cuh) feed the inline-asm bodies values loaded from memory only; a wrong asm constraint shows
// on operands the register allocator knows something about (the "+v" accumulator of mont_cols.inc and fr_from_u128), and
// the portable host bodies cannot show it at all.  The same dispatch runs on the host (tests/emu/emu.cpp, overflow traps on) and on the
// device (mi_debug_field_shape_dev, one record per lane).  Nothing in the product calls this file.
//
// The shape is a TEMPLATE parameter: one kernel per shape, so every body is compiled the way its real call site is -- the literals stay
// literals, nothing sits behind a run-time switch or an out-of-line helper that the product does not have either.  No body has a
// data-dependent address or trip count: a wrong product gives wrong words and nothing else.
//
// Record layout (u32 words; the numbers are mirrored in include/mi355x_groth16_debug.h):
//   in  [SH_IN_WORDS]:  x | y | u | v, eight limbs each (raw Montgomery residues below the modulus).  The curve shapes read them as
//                       points: G1 a = (x, y), b = (u, v); G2 one point x.a0 | x.a1 | y.a0 | y.a1; SHT_G1_INF_ADD an XYZZ point X | Y | ZZ | ZZZ;
//                       SHT_G1X29_CHAIN two points in the packed R' form of curve29.cuh.  The 29-bit shapes read nine limbs a at in[0..8]
//                       and nine limbs b at in[9..17].
//   out [SH_OUT_WORDS]: up to four results of eight limbs at out[8 k]; the 29-bit shapes leave three results of nine limbs at out[9 k].
//                       Words a shape does not write are zero.
// Shape numbers: a generic shape g over Fr is g, over Fp it is SHG_END + g; a typed shape t is 2 SHG_END + t.
#pragma once
#include "curve29.cuh"
#include "fp12.cuh"

#define SH_IN_WORDS 32
#define SH_OUT_WORDS 32
enum {   // generic over the field: results o0 | o1 | o2 | o3
    // A: a literal factor, on either side
    SHG_MUL_ONE = 0,      // x one() | one() x | x zero() | zero() x
    SHG_MUL_R2,           // x r2() | fe_to_mont(x) | r2() x
    SHG_MUL_UNIT,         // x {1, 0, .., 0} | fe_from_mont(x) | {1, 0, .., 0} x
    SHG_MUL_U32,          // x fe_from_u32(2) | x fe_from_u32(3) | x fe_from_u32(9) | fe_from_u32(3) fe_from_u32(9)
    SHG_MUL_PM1,          // x (p - 1) | (p - 1) x | (p - 1)(p - 1), p - 1 a literal
    // B: limbs that are provably zero.  k(.) keeps the named words of a loaded value and writes literal zeros elsewhere:
    //    k(x) y | y k(x) | k(x) k(y) | fe_to_mont(k(x))
    SHG_ZERO_LO1,         // word 0
    SHG_ZERO_LO2,         // words 0, 1
    SHG_ZERO_LO4,         // words 0..3: fr_from_u128 (pairing_ops.cuh), and the same over Fp
    SHG_ZERO_HI4,         // words 4..7
    SHG_ZERO_MID1,        // word 3
    SHG_U128_CHAIN,       // k_locate_points with several commitments: pw = fe_to_mont(lo4(x)); three times { o_k = fe_from_mont(pw); pw = pw y }; o3 = pw
    // C: one value in two places, results over inputs
    SHG_SQR,              // x x | fe_sqr(x)
    SHG_INPLACE,          // x = x y | y = x y | x = x x three times, all in place
    SHG_MUL2_SAME,        // fe_mul2_add(x, y, y, x) | (x, x, x, x) | (x, y, x, y)
    SHG_MUL2_LIT,         // fe_mul2_add(x, y, zero(), v) | fe_mul2_add(x, y, u, one()) | x y
    SHG_MUL_SUB_SAME,     // fe_mul_sub(x, y, x, y) | fe_mul_sub(x, x, y, y)
    SHG_LAZY_LIT,         // fe_mul_lazy(x, one()) | fe_mul_lazy(x, p - 1) | fe_mul_lazy(x, r2()), raw
    // D: chains that start at a literal
    SHG_POW5,             // fe_pow(x, 5)
    SHG_INV,              // fe_inv(x)
    SHG_LAGRANGE,         // k_lagrange's run (setup.hip) of three rows at tau = x, nodes y, u, v: 1 / (x - y) | 1 / (x - u) | 1 / (x - v) | what is left of the inverse (one)
    // E: the carry-chain asm with literal operands
    SHG_ADD_LIT,          // x + zero() | x + one() | (p - 1) + x | fe_dbl(x)
    SHG_SUB_LIT,          // zero() - x | x - x | fe_neg(zero()) | fe_neg_raw(zero())
    SHG_LAZY_ADD_LIT,     // fe_add_nored(x, zero()) | fe_sub_plus2p(x, x) | fe_condsub_2p(2p) | fe_canon(2p), 2p a literal
    SHG_LAZY_X,           // fe_condsub_2p(x) | fe_canon(x) | fe_condsub_2p(x + x) | fe_canon(x + x + x), the sums by fe_add_nored
    // B again, ONE product per kernel (the register allocator is freest where nothing else is live: fr_from_u128 at the head of
    // k_locate_points): SHG_ZERO_ALONE + 4 f + s, f = 0..4 the forms lo1, lo2, lo4, hi4, mid1 in the order above,
    // s = 0: k(x) y, 1: y k(x), 2: k(x) k(y), 3: fe_to_mont(k(x)); the result at o0
    SHG_ZERO_ALONE,
    SHG_END = SHG_ZERO_ALONE + 20
};
enum {   // one type each
    // D: curve chains that start at a literal (affine results, (0, 0) = infinity)
    SHT_G1_MADD = 0,      // G1X::from_affine(a), xyzz_madd(b): a + b at out[0..15]
    SHT_G2_MADD,          // G2X::from_affine(a), xyzz_madd(a) twice (the doubling branch, then a general step): 3 a at out[0..31]
    SHT_G1_INF_ADD,       // G1X::inf(), xyzz_add(q) twice, q the XYZZ point of the record: 2 q at out[0..15]
    SHT_G2_INF_ADD,       // G2X::inf(), xyzz_add(from_affine(a)) twice: 2 a at out[0..31]
    SHT_G1_DBL_INF,       // xyzz_dbl(G1X::inf()) at out[0..15] (infinity), then xyzz_madd(a) at out[16..31]
    SHT_G2_DBL_INF,       // xyzz_dbl(G2X::inf()), xyzz_madd(a): a at out[0..31]
    SHT_G1X29_CHAIN,      // g1x29_inf(), g1x29_madd(a), g1x29_madd(b), back through g1x29_to_std: a + b at out[0..15]
    // F: Fp2, X = x + y u, Y = u + v u: results o0 o1 | o2 o3
    SHT_FP2_HALF_ZERO,    // X (u + 0 u) | X (0 + v u)
    SHT_FP2_MUL_ONE,      // X Fp2::one() | Fp2::one() X
    SHT_FP2_XI,           // fp2_mul_xi(X) | fp2_mul_xi(Fp2::one())
    SHT_FP2_REAL,         // fe_sqr(x + 0 u) | fe_inv(x + 0 u)
    SHT_FP2_SQR,          // X X | fe_sqr(X)
    SHT_FP2_MUL_SUB,      // fe_mul_sub(X, Y, X, X) | fe_mul_sub(X, Y, X, Y)
    // G: nine 29-bit limbs over Fp, a = in[0..8], b = in[9..17]; k(a) keeps limbs 0..3 and writes literal zeros above
    SHT_F29_ONE,          // f29_mul(a, one) | f29_mul(one, a) | f29_sqr(one)
    SHT_F29_ZERO_UPPER,   // f29_mul(k(a), b) | f29_mul(b, k(a)) | f29_sqr(k(a))
    SHT_F29_TWICE,        // f29_mul(a, a) | f29_sqr(a) | f29_mul(k(a), k(a))
    // H: Fp12.  f has the coefficients (x, y), (u, v), (y, x), (v, u), (x, u), (y, v); a result z is folded to four words o_j = z_j + z_(j + 4) + z_(j + 8)
    SHT_FP12_MUL_ONE,     // fp12_mul(f, one)
    SHT_FP12_LINE_FIRST,  // f = one, then fp12_mul_by_line(f, (x, y), (u, v), (y, u)): the Miller loop's first step
    SHT_FP12_SQR_ONE,     // fp12_sqr(one) folded to o0 o1 (o_j = sum of z_(j + 2 i)) | fp12_cyclo_sqr(one) folded to o2 o3
    SHT_END
};
#define SH_FR(g) (g)
#define SH_FP(g) (SHG_END + (g))
#define SH_TYPED(t) (2 * SHG_END + (t))
#define SH_OP_END (2 * SHG_END + SHT_END)

template <class P>
MI_HD Fe<P> sh_get(const u32 *w) { Fe<P> x;
#pragma unroll
    for (int i = 0; i < 8; i++) x.l[i] = w[i];
    return x; }
template <class P>
MI_HD void sh_put(u32 *w, const Fe<P> &x) {
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = x.l[i];
}
MI_HD void sh_put2(u32 *w, const Fp2 &x) { sh_put(w, x.a0); sh_put(w + 8, x.a1); }
// the words [lo, hi) of x, literal zeros elsewhere
template <class P, int LO, int HI>
MI_HD Fe<P> sh_keep(const Fe<P> &x) { Fe<P> z = Fe<P>::zero();
#pragma unroll
    for (int i = LO; i < HI; i++) z.l[i] = x.l[i];
    return z; }
template <class P>
MI_HD Fe<P> sh_unit() { Fe<P> z = Fe<P>::zero(); z.l[0] = 1; return z; }
template <class P>
MI_HD Fe<P> sh_pm1() { Fe<P> z = Fe<P>::modulus(); z.l[0] -= 1; return z; }   // the low limb of both moduli is odd
template <class P>
MI_HD Fe<P> sh_2p() { Fe<P> z;
#pragma unroll
    for (int i = 0; i < 8; i++) z.l[i] = P::p2[i];
    return z; }

template <class P, int LO, int HI>
MI_HD void sh_zero_limbs(const Fe<P> &x, const Fe<P> &y, u32 *out) {
    const Fe<P> kx = sh_keep<P, LO, HI>(x), ky = sh_keep<P, LO, HI>(y);
    sh_put(out, kx * y); sh_put(out + 8, y * kx); sh_put(out + 16, kx * ky); sh_put(out + 24, fe_to_mont(kx));
}

template <class P, int G>
MI_HD void shape_generic(const u32 *in, u32 *out) {
    typedef Fe<P> F;
    F x = sh_get<P>(in), y = sh_get<P>(in + 8);
    const F u = sh_get<P>(in + 16), v = sh_get<P>(in + 24);
    if constexpr (G == SHG_MUL_ONE) {
        sh_put(out, x * F::one()); sh_put(out + 8, F::one() * x); sh_put(out + 16, x * F::zero()); sh_put(out + 24, F::zero() * x);
    } else if constexpr (G == SHG_MUL_R2) {
        sh_put(out, x * F::r2()); sh_put(out + 8, fe_to_mont(x)); sh_put(out + 16, F::r2() * x);
    } else if constexpr (G == SHG_MUL_UNIT) {
        sh_put(out, x * sh_unit<P>()); sh_put(out + 8, fe_from_mont(x)); sh_put(out + 16, sh_unit<P>() * x);
    } else if constexpr (G == SHG_MUL_U32) {
        sh_put(out, x * fe_from_u32<P>(2)); sh_put(out + 8, x * fe_from_u32<P>(3)); sh_put(out + 16, x * fe_from_u32<P>(9));
        sh_put(out + 24, fe_from_u32<P>(3) * fe_from_u32<P>(9));
    } else if constexpr (G == SHG_MUL_PM1) {
        sh_put(out, x * sh_pm1<P>()); sh_put(out + 8, sh_pm1<P>() * x); sh_put(out + 16, sh_pm1<P>() * sh_pm1<P>());
    } else if constexpr (G == SHG_ZERO_LO1) {
        sh_zero_limbs<P, 0, 1>(x, y, out);
    } else if constexpr (G == SHG_ZERO_LO2) {
        sh_zero_limbs<P, 0, 2>(x, y, out);
    } else if constexpr (G == SHG_ZERO_LO4) {
        sh_zero_limbs<P, 0, 4>(x, y, out);
    } else if constexpr (G == SHG_ZERO_HI4) {
        sh_zero_limbs<P, 4, 8>(x, y, out);
    } else if constexpr (G == SHG_ZERO_MID1) {
        sh_zero_limbs<P, 3, 4>(x, y, out);
    } else if constexpr (G == SHG_U128_CHAIN) {
        F pw = fe_to_mont(sh_keep<P, 0, 4>(x));
        for (int k = 0; k < 3; k++) {
            sh_put(out + 8 * k, fe_from_mont(pw));
            pw = pw * y;
        }
        sh_put(out + 24, pw);
    } else if constexpr (G == SHG_SQR) {
        sh_put(out, x * x); sh_put(out + 8, fe_sqr(x));
    } else if constexpr (G == SHG_INPLACE) {
        F a = x, b = y, c = x;
        a = a * b; sh_put(out, a);
        b = x * b; sh_put(out + 8, b);
        c = c * c; c = c * c; c = c * c; sh_put(out + 16, c);
    } else if constexpr (G == SHG_MUL2_SAME) {
        sh_put(out, fe_mul2_add(x, y, y, x)); sh_put(out + 8, fe_mul2_add(x, x, x, x)); sh_put(out + 16, fe_mul2_add(x, y, x, y));
    } else if constexpr (G == SHG_MUL2_LIT) {
        sh_put(out, fe_mul2_add(x, y, F::zero(), v)); sh_put(out + 8, fe_mul2_add(x, y, u, F::one())); sh_put(out + 16, x * y);
    } else if constexpr (G == SHG_MUL_SUB_SAME) {
        sh_put(out, fe_mul_sub(x, y, x, y)); sh_put(out + 8, fe_mul_sub(x, x, y, y));
    } else if constexpr (G == SHG_LAZY_LIT) {
        sh_put(out, fe_mul_lazy(x, F::one())); sh_put(out + 8, fe_mul_lazy(x, sh_pm1<P>())); sh_put(out + 16, fe_mul_lazy(x, F::r2()));
    } else if constexpr (G == SHG_POW5) {
        const u32 e[8] = {5, 0, 0, 0, 0, 0, 0, 0};
        sh_put(out, fe_pow(x, e));
    } else if constexpr (G == SHG_INV) {
        sh_put(out, fe_inv(x));
    } else if constexpr (G == SHG_LAGRANGE) {
        const F d0 = x - y, d1 = x - u, d2 = x - v;
        F p = F::one();
        const F l0 = p; p = p * d0;
        const F l1 = p; p = p * d1;
        const F l2 = p; p = p * d2;
        F inv = fe_inv(p);
        sh_put(out + 16, inv * l2); inv = inv * d2;
        sh_put(out + 8, inv * l1); inv = inv * d1;
        sh_put(out, inv * l0); inv = inv * d0;
        sh_put(out + 24, inv);
    } else if constexpr (G == SHG_ADD_LIT) {
        sh_put(out, x + F::zero()); sh_put(out + 8, x + F::one()); sh_put(out + 16, sh_pm1<P>() + x); sh_put(out + 24, fe_dbl(x));
    } else if constexpr (G == SHG_SUB_LIT) {
        sh_put(out, F::zero() - x); sh_put(out + 8, x - x); sh_put(out + 16, fe_neg(F::zero())); sh_put(out + 24, fe_neg_raw(F::zero()));
    } else if constexpr (G == SHG_LAZY_ADD_LIT) {
        sh_put(out, fe_add_nored(x, F::zero())); sh_put(out + 8, fe_sub_plus2p(x, x)); sh_put(out + 16, fe_condsub_2p(sh_2p<P>()));
        sh_put(out + 24, fe_canon(sh_2p<P>()));
    } else if constexpr (G == SHG_LAZY_X) {
        sh_put(out, fe_condsub_2p(x)); sh_put(out + 8, fe_canon(x)); sh_put(out + 16, fe_condsub_2p(fe_add_nored(x, x)));
        sh_put(out + 24, fe_canon(fe_add_nored(fe_add_nored(x, x), x)));
    } else if constexpr (G >= SHG_ZERO_ALONE && G < SHG_ZERO_ALONE + 20) {
        constexpr int f = (G - SHG_ZERO_ALONE) / 4, s = (G - SHG_ZERO_ALONE) % 4;
        constexpr int LO = f == 3 ? 4 : f == 4 ? 3 : 0, HI = f == 0 ? 1 : f == 1 ? 2 : f == 2 ? 4 : f == 3 ? 8 : 4;
        const F kx = sh_keep<P, LO, HI>(x);
        if constexpr (s == 0) sh_put(out, kx * y);
        else if constexpr (s == 1) sh_put(out, y * kx);
        else if constexpr (s == 2) sh_put(out, kx * sh_keep<P, LO, HI>(y));
        else sh_put(out, fe_to_mont(kx));
    } else {
        static_assert(G >= 0 && G < SHG_END, "unknown generic shape");
    }
    (void)y; (void)u; (void)v;
}

MI_HD F29 sh_get29(const u32 *w) { F29 x;
#pragma unroll
    for (int i = 0; i < 9; i++) x.l[i] = w[i];
    return x; }
MI_HD void sh_put29(u32 *w, const F29 &x) {
#pragma unroll
    for (int i = 0; i < 9; i++) w[i] = x.l[i];
}
MI_HD F29 sh_keep29(const F29 &a) { F29 z = f29_zero();
#pragma unroll
    for (int i = 0; i < 4; i++) z.l[i] = a.l[i];
    return z; }
template <int K>   // z folded to K Fp words: o_j = sum of z_(j + K i)
MI_HD void sh_fold12(u32 *out, const Fp12 &z) {
    const Fp c[12] = {z.c0.b0.a0, z.c0.b0.a1, z.c0.b1.a0, z.c0.b1.a1, z.c0.b2.a0, z.c0.b2.a1, z.c1.b0.a0, z.c1.b0.a1, z.c1.b1.a0, z.c1.b1.a1, z.c1.b2.a0, z.c1.b2.a1};
#pragma unroll
    for (int j = 0; j < K; j++) {
        Fp s = c[j];
#pragma unroll
        for (int i = j + K; i < 12; i += K) s = s + c[i];
        sh_put(out + 8 * j, s);
    }
}

template <int T>
MI_HD void shape_typed(const u32 *in, u32 *out) {
    typedef FpParams Q;
    const Fp x = sh_get<Q>(in), y = sh_get<Q>(in + 8), u = sh_get<Q>(in + 16), v = sh_get<Q>(in + 24);
    const Fp2 X{x, y}, Y{u, v};
    if constexpr (T == SHT_G1_MADD) {
        G1X acc = G1X::from_affine(G1Aff{x, y});
        xyzz_madd(acc, G1Aff{u, v}, false);
        const G1Aff r = xyzz_to_affine(acc);
        sh_put(out, r.x); sh_put(out + 8, r.y);
    } else if constexpr (T == SHT_G2_MADD) {
        const G2Aff a{X, Y};
        G2X acc = G2X::from_affine(a);
        xyzz_madd(acc, a, false);
        xyzz_madd(acc, a, false);
        const G2Aff r = xyzz_to_affine(acc);
        sh_put2(out, r.x); sh_put2(out + 16, r.y);
    } else if constexpr (T == SHT_G1_INF_ADD) {
        const G1X q{x, y, u, v};
        G1X acc = G1X::inf();
        xyzz_add(acc, q);
        xyzz_add(acc, q);
        const G1Aff r = xyzz_to_affine(acc);
        sh_put(out, r.x); sh_put(out + 8, r.y);
    } else if constexpr (T == SHT_G2_INF_ADD) {
        const G2X q = G2X::from_affine(G2Aff{X, Y});
        G2X acc = G2X::inf();
        xyzz_add(acc, q);
        xyzz_add(acc, q);
        const G2Aff r = xyzz_to_affine(acc);
        sh_put2(out, r.x); sh_put2(out + 16, r.y);
    } else if constexpr (T == SHT_G1_DBL_INF) {
        G1X acc = xyzz_dbl(G1X::inf());
        const G1Aff r0 = xyzz_to_affine(acc);
        sh_put(out, r0.x); sh_put(out + 8, r0.y);
        xyzz_madd(acc, G1Aff{x, y}, false);
        const G1Aff r = xyzz_to_affine(acc);
        sh_put(out + 16, r.x); sh_put(out + 24, r.y);
    } else if constexpr (T == SHT_G2_DBL_INF) {
        G2X acc = xyzz_dbl(G2X::inf());
        xyzz_madd(acc, G2Aff{X, Y}, false);
        const G2Aff r = xyzz_to_affine(acc);
        sh_put2(out, r.x); sh_put2(out + 16, r.y);
    } else if constexpr (T == SHT_G1X29_CHAIN) {
        G1X29 acc = g1x29_inf();
        g1x29_madd(acc, in, false);
        g1x29_madd(acc, in + 16, false);
        const G1Aff r = xyzz_to_affine(g1x29_to_std(acc));
        sh_put(out, r.x); sh_put(out + 8, r.y);
    } else if constexpr (T == SHT_FP2_HALF_ZERO) {
        sh_put2(out, X * Fp2{u, Fp::zero()}); sh_put2(out + 16, X * Fp2{Fp::zero(), v});
    } else if constexpr (T == SHT_FP2_MUL_ONE) {
        sh_put2(out, X * Fp2::one()); sh_put2(out + 16, Fp2::one() * X);
    } else if constexpr (T == SHT_FP2_XI) {
        sh_put2(out, fp2_mul_xi(X)); sh_put2(out + 16, fp2_mul_xi(Fp2::one()));
    } else if constexpr (T == SHT_FP2_REAL) {
        const Fp2 r{x, Fp::zero()};
        sh_put2(out, fe_sqr(r)); sh_put2(out + 16, fe_inv(r));
    } else if constexpr (T == SHT_FP2_SQR) {
        sh_put2(out, X * X); sh_put2(out + 16, fe_sqr(X));
    } else if constexpr (T == SHT_FP2_MUL_SUB) {
        sh_put2(out, fe_mul_sub(X, Y, X, X)); sh_put2(out + 16, fe_mul_sub(X, Y, X, Y));
    } else if constexpr (T == SHT_F29_ONE) {
        const F29 a = sh_get29(in), one = f29_const<Q>(P29<Q>::one);
        sh_put29(out, f29_mul<Q>(a, one)); sh_put29(out + 9, f29_mul<Q>(one, a)); sh_put29(out + 18, f29_sqr<Q>(one));
    } else if constexpr (T == SHT_F29_ZERO_UPPER) {
        const F29 b = sh_get29(in + 9), k = sh_keep29(sh_get29(in));
        sh_put29(out, f29_mul<Q>(k, b)); sh_put29(out + 9, f29_mul<Q>(b, k)); sh_put29(out + 18, f29_sqr<Q>(k));
    } else if constexpr (T == SHT_F29_TWICE) {
        const F29 a = sh_get29(in), k = sh_keep29(a);
        sh_put29(out, f29_mul<Q>(a, a)); sh_put29(out + 9, f29_sqr<Q>(a)); sh_put29(out + 18, f29_mul<Q>(k, k));
    } else if constexpr (T == SHT_FP12_MUL_ONE) {
        const Fp12 f{Fp6{Fp2{x, y}, Fp2{u, v}, Fp2{y, x}}, Fp6{Fp2{v, u}, Fp2{x, u}, Fp2{y, v}}}, one = Fp12::one();
        Fp12 z;
        fp12_mul(&z, &f, &one);
        sh_fold12<4>(out, z);
    } else if constexpr (T == SHT_FP12_LINE_FIRST) {
        Fp12 f = Fp12::one();
        const Fp2 l0{x, y}, l3{u, v}, l4{y, u};
        fp12_mul_by_line(&f, &f, &l0, &l3, &l4);
        sh_fold12<4>(out, f);
    } else if constexpr (T == SHT_FP12_SQR_ONE) {
        const Fp12 one = Fp12::one();
        Fp12 z;
        fp12_sqr(&z, &one);
        sh_fold12<2>(out, z);
        fp12_cyclo_sqr(&z, &one);
        sh_fold12<2>(out + 16, z);
    } else {
        static_assert(T >= 0 && T < SHT_END, "unknown typed shape");
    }
    (void)X; (void)Y;
}

// one record: in and out are the caller's own SH_IN_WORDS / SH_OUT_WORDS words (registers on the device), out zeroed
template <int SHAPE>
MI_HD void shape_op(const u32 *in, u32 *out) {
    static_assert(SHAPE >= 0 && SHAPE < SH_OP_END, "unknown shape");
    if constexpr (SHAPE < SHG_END) shape_generic<FrParams, SHAPE>(in, out);
    else if constexpr (SHAPE < 2 * SHG_END) shape_generic<FpParams, SHAPE - SHG_END>(in, out);
    else shape_typed<SHAPE - 2 * SHG_END>(in, out);
}

// BN254 extension tower for the pairing (groth16.Verify, mt.go:497 of the reference): gnark-crypto's fptower shape
//     Fp2 = Fp[u]/(u^2 + 1)   (field.cuh)      Fp6 = Fp2[v]/(v^3 - xi), xi = 9 + u      Fp12 = Fp6[w]/(w^2 - v)
// on top of the 8 x 32-bit Montgomery Fp / Fp2 of field.cuh.  An Fp12 value is 12 x Fp = 384 bytes in the order
//     C0.B0.A0, C0.B0.A1, C0.B1.A0, C0.B1.A1, C0.B2.A0, C0.B2.A1, C1.B0.A0, ... C1.B2.A1
// (the memory layout of the structs below, and of gnark-crypto's E12).  Everything is MI_HD: the host build of the tests (tests/emu/
// emu_pairing.cpp, -DMI_CHECK_NOWRAP) runs the same bodies.
//
// The Fp6 / Fp12 products, the Frobenius maps and the cyclotomic squaring are out-of-line device functions over pointers (MI_OOL; the
// precedent is fp_mul_call of field.cuh): a final exponentiation is ~130 Fp12 products of 54 Fp products each -- inlined, no kernel
// would fit the instruction cache or finish compiling.  The price: an Fp12 value that has its address taken lives in scratch memory, not
// in its 96 VGPRs (profiles/verify_kernel_resources.txt).  Coefficients are only ever indexed by name, never by a runtime index.
// Outputs may alias inputs: every function reads its operands before it writes.
#pragma once
#include "curve.cuh"
#include "fp12_consts.inc"   // generated: tools/gen_fp12_consts.py

// the generators gnark-crypto's bn254 package fixes: g1 = (1, 2), g2 as in EIP-197
MI_HD G1Aff g1_generator() { return G1Aff{Fp::one(), fe_from_u32<FpParams>(2)}; }
MI_HD G2Aff g2_generator() { return G2Aff{fp12c_g2gen_x(), fp12c_g2gen_y()}; }

#if defined(__HIP_DEVICE_COMPILE__)
#define MI_OOL __host__ __device__ __attribute__((noinline))   // (__host__: the host functions of a .hip file are parsed in the device pass too)
#else
#define MI_OOL MI_HD
#endif

// ---------------------------------------------------------------- Fp2 helpers the tower needs
MI_HD Fp2 fp2_conj(const Fp2 &x) { return Fp2{x.a0, fe_neg(x.a1)}; }
MI_HD Fp2 fp2_mul_fp(const Fp2 &x, const Fp &k) { return Fp2{fp_mul_call(x.a0, k), fp_mul_call(x.a1, k)}; }
// x (9 + u) = (9 x0 - x1) + (9 x1 + x0) u
MI_HD Fp2 fp2_mul_xi(const Fp2 &x) {
    const Fp2 n = fe_dbl(fe_dbl(fe_dbl(x))) + x;
    return Fp2{n.a0 - x.a1, n.a1 + x.a0};
}
MI_HD Fp2 fp2_triple(const Fp2 &x) { return fe_dbl(x) + x; }

// ---------------------------------------------------------------- Fp6
struct Fp6 {
    Fp2 b0, b1, b2;
    static MI_HD Fp6 zero() { return Fp6{Fp2::zero(), Fp2::zero(), Fp2::zero()}; }
    static MI_HD Fp6 one() { return Fp6{Fp2::one(), Fp2::zero(), Fp2::zero()}; }
    MI_HD bool is_zero() const { return b0.is_zero() && b1.is_zero() && b2.is_zero(); }
    MI_HD bool operator==(const Fp6 &o) const { return b0 == o.b0 && b1 == o.b1 && b2 == o.b2; }
};
MI_HD Fp6 operator+(const Fp6 &x, const Fp6 &y) { return Fp6{x.b0 + y.b0, x.b1 + y.b1, x.b2 + y.b2}; }
MI_HD Fp6 operator-(const Fp6 &x, const Fp6 &y) { return Fp6{x.b0 - y.b0, x.b1 - y.b1, x.b2 - y.b2}; }
MI_HD Fp6 fe_neg(const Fp6 &x) { return Fp6{fe_neg(x.b0), fe_neg(x.b1), fe_neg(x.b2)}; }
MI_HD Fp6 fe_dbl(const Fp6 &x) { return x + x; }
// x v: (b0, b1, b2) -> (xi b2, b0, b1)
MI_HD Fp6 fp6_mul_v(const Fp6 &x) { return Fp6{fp2_mul_xi(x.b2), x.b0, x.b1}; }
// Karatsuba over Fp2: 6 products
MI_OOL void fp6_mul(Fp6 *z, const Fp6 *x, const Fp6 *y) {
    const Fp2 t0 = x->b0 * y->b0, t1 = x->b1 * y->b1, t2 = x->b2 * y->b2;
    const Fp2 c0 = fp2_mul_xi((x->b1 + x->b2) * (y->b1 + y->b2) - t1 - t2) + t0;
    const Fp2 c1 = (x->b0 + x->b1) * (y->b0 + y->b1) - t0 - t1 + fp2_mul_xi(t2);
    const Fp2 c2 = (x->b0 + x->b2) * (y->b0 + y->b2) - t0 - t2 + t1;
    z->b0 = c0; z->b1 = c1; z->b2 = c2;
}
// Chung-Hasan SQR2: 2 products + 3 squarings
MI_OOL void fp6_sqr(Fp6 *z, const Fp6 *x) {
    const Fp2 s0 = fe_sqr(x->b0), s1 = fe_dbl(x->b0 * x->b1), s2 = fe_sqr(x->b0 - x->b1 + x->b2);
    const Fp2 s3 = fe_dbl(x->b1 * x->b2), s4 = fe_sqr(x->b2);
    z->b0 = s0 + fp2_mul_xi(s3);
    z->b1 = s1 + fp2_mul_xi(s4);
    z->b2 = s1 + s2 + s3 - s0 - s4;
}
// x (s0 + s1 v): 5 products
MI_OOL void fp6_mul_by_01(Fp6 *z, const Fp6 *x, const Fp2 *s0, const Fp2 *s1) {
    const Fp2 t0 = x->b0 * *s0, t1 = x->b1 * *s1;
    const Fp2 c0 = t0 + fp2_mul_xi(x->b2 * *s1);
    const Fp2 c1 = (x->b0 + x->b1) * (*s0 + *s1) - t0 - t1;
    const Fp2 c2 = t1 + x->b2 * *s0;
    z->b0 = c0; z->b1 = c1; z->b2 = c2;
}
MI_HD Fp6 fp6_mul_fp2(const Fp6 &x, const Fp2 &k) { return Fp6{x.b0 * k, x.b1 * k, x.b2 * k}; }
// the norm-based inverse (0 -> 0, as fe_inv)
MI_OOL void fp6_inv(Fp6 *z, const Fp6 *x) {
    const Fp2 A = fe_sqr(x->b0) - fp2_mul_xi(x->b1 * x->b2);
    const Fp2 B = fp2_mul_xi(fe_sqr(x->b2)) - x->b0 * x->b1;
    const Fp2 C = fe_sqr(x->b1) - x->b0 * x->b2;
    const Fp2 F = fe_inv(x->b0 * A + fp2_mul_xi(x->b2 * B + x->b1 * C));
    z->b0 = A * F; z->b1 = B * F; z->b2 = C * F;
}

// ---------------------------------------------------------------- Fp12
struct Fp12 {
    Fp6 c0, c1;
    static MI_HD Fp12 one() { return Fp12{Fp6::one(), Fp6::zero()}; }
    MI_HD bool operator==(const Fp12 &o) const { return c0 == o.c0 && c1 == o.c1; }
};
static_assert(sizeof(Fp12) == 384, "12 x Fp, no padding");
MI_HD void fp12_add(Fp12 *z, const Fp12 *x, const Fp12 *y) { z->c0 = x->c0 + y->c0; z->c1 = x->c1 + y->c1; }
MI_HD void fp12_sub(Fp12 *z, const Fp12 *x, const Fp12 *y) { z->c0 = x->c0 - y->c0; z->c1 = x->c1 - y->c1; }
// the p^6-power Frobenius; the inverse of a value of the cyclotomic subgroup
MI_HD void fp12_conj(Fp12 *z, const Fp12 *x) { z->c0 = x->c0; z->c1 = fe_neg(x->c1); }
// Karatsuba over Fp6: 3 products
MI_OOL void fp12_mul(Fp12 *z, const Fp12 *x, const Fp12 *y) {
    Fp6 t0, t1, s, sx = x->c0 + x->c1, sy = y->c0 + y->c1;
    fp6_mul(&t0, &x->c0, &y->c0);
    fp6_mul(&t1, &x->c1, &y->c1);
    fp6_mul(&s, &sx, &sy);
    z->c1 = s - t0 - t1;
    z->c0 = t0 + fp6_mul_v(t1);
}
// complex squaring: 2 products
MI_OOL void fp12_sqr(Fp12 *z, const Fp12 *x) {
    Fp6 ab, t, sa = x->c0 + x->c1, sb = x->c0 + fp6_mul_v(x->c1);
    fp6_mul(&ab, &x->c0, &x->c1);
    fp6_mul(&t, &sa, &sb);
    z->c0 = t - ab - fp6_mul_v(ab);
    z->c1 = ab + ab;
}
MI_OOL void fp12_inv(Fp12 *z, const Fp12 *x) {
    Fp6 a, b, t;
    fp6_sqr(&a, &x->c0);
    fp6_sqr(&b, &x->c1);
    t = a - fp6_mul_v(b);
    fp6_inv(&t, &t);
    fp6_mul(&a, &x->c0, &t);
    fp6_mul(&b, &x->c1, &t);
    z->c0 = a; z->c1 = fe_neg(b);
}
// x (l0 + l3 w + l4 v w): the value of a line of the Miller loop, 13 Fp2 products instead of 18
MI_OOL void fp12_mul_by_line(Fp12 *z, const Fp12 *x, const Fp2 *l0, const Fp2 *l3, const Fp2 *l4) {
    Fp6 t1, t2, s = x->c0 + x->c1;
    const Fp6 t0 = fp6_mul_fp2(x->c0, *l0);
    const Fp2 l03 = *l0 + *l3;
    fp6_mul_by_01(&t1, &x->c1, l3, l4);
    fp6_mul_by_01(&t2, &s, &l03, l4);
    z->c1 = t2 - t0 - t1;
    z->c0 = t0 + fp6_mul_v(t1);
}
// x^(p^k): the coefficient of w^e (e = i + 2 j for C_i.B_j) is conjugated k times and multiplied by xi^(e (p^k - 1) / 6)
MI_OOL void fp12_frob1(Fp12 *z, const Fp12 *x) {
    z->c0.b0 = fp2_conj(x->c0.b0);
    z->c1.b0 = fp2_conj(x->c1.b0) * fp12c_frob1_1();
    z->c0.b1 = fp2_conj(x->c0.b1) * fp12c_frob1_2();
    z->c1.b1 = fp2_conj(x->c1.b1) * fp12c_frob1_3();
    z->c0.b2 = fp2_conj(x->c0.b2) * fp12c_frob1_4();
    z->c1.b2 = fp2_conj(x->c1.b2) * fp12c_frob1_5();
}
MI_OOL void fp12_frob2(Fp12 *z, const Fp12 *x) {   // the p^2 coefficients lie in Fp
    z->c0.b0 = x->c0.b0;
    z->c1.b0 = fp2_mul_fp(x->c1.b0, fp12c_frob2_1().a0);
    z->c0.b1 = fp2_mul_fp(x->c0.b1, fp12c_frob2_2().a0);
    z->c1.b1 = fp2_mul_fp(x->c1.b1, fp12c_frob2_3().a0);
    z->c0.b2 = fp2_mul_fp(x->c0.b2, fp12c_frob2_4().a0);
    z->c1.b2 = fp2_mul_fp(x->c1.b2, fp12c_frob2_5().a0);
}
MI_OOL void fp12_frob3(Fp12 *z, const Fp12 *x) {
    z->c0.b0 = fp2_conj(x->c0.b0);
    z->c1.b0 = fp2_conj(x->c1.b0) * fp12c_frob3_1();
    z->c0.b1 = fp2_conj(x->c0.b1) * fp12c_frob3_2();
    z->c1.b1 = fp2_conj(x->c1.b1) * fp12c_frob3_3();
    z->c0.b2 = fp2_conj(x->c0.b2) * fp12c_frob3_4();
    z->c1.b2 = fp2_conj(x->c1.b2) * fp12c_frob3_5();
}
// Granger-Scott squaring, valid in the cyclotomic subgroup only (x^(p^4 - p^2 + 1) = 1: every value after the easy part of the final
// exponentiation): with (x0 .. x5) = (C0.B0, C0.B1, C0.B2, C1.B0, C1.B1, C1.B2),
//     (3 (x4^2 xi + x0^2) - 2 x0, 3 (x2^2 xi + x3^2) - 2 x1, 3 (x5^2 xi + x1^2) - 2 x2, 6 x1 x5 xi + 2 x3, 6 x0 x4 + 2 x4, 6 x2 x3 + 2 x5)
// -- 9 Fp2 squarings where fp12_sqr takes 12 products.
MI_OOL void fp12_cyclo_sqr(Fp12 *z, const Fp12 *x) {
    const Fp2 x0 = x->c0.b0, x1 = x->c0.b1, x2 = x->c0.b2, x3 = x->c1.b0, x4 = x->c1.b1, x5 = x->c1.b2;
    const Fp2 q0 = fe_sqr(x0), q4 = fe_sqr(x4), m04 = fe_sqr(x0 + x4) - q0 - q4;                     // 2 x0 x4
    const Fp2 q2 = fe_sqr(x2), q3 = fe_sqr(x3), m23 = fe_sqr(x2 + x3) - q2 - q3;                     // 2 x2 x3
    const Fp2 q1 = fe_sqr(x1), q5 = fe_sqr(x5), m15 = fp2_mul_xi(fe_sqr(x1 + x5) - q1 - q5);         // 2 x1 x5 xi
    const Fp2 a = fp2_mul_xi(q4) + q0, b = fp2_mul_xi(q2) + q3, c = fp2_mul_xi(q5) + q1;
    z->c0.b0 = fe_dbl(a - x0) + a;
    z->c0.b1 = fe_dbl(b - x1) + b;
    z->c0.b2 = fe_dbl(c - x2) + c;
    z->c1.b0 = fe_dbl(m15 + x3) + m15;
    z->c1.b1 = fe_dbl(m04 + x4) + m04;
    z->c1.b2 = fe_dbl(m23 + x5) + m23;
}

// The optimal ate pairing of BN254 for groth16.Verify (mt.go:497 of the reference): e: G1 x G2 -> GT in Fp12 (fp12.cuh).
//
// Miller loop.  x0 = 4965661367192848881; T runs over the multiples of Q ON THE TWIST y^2 = x^3 + 3/xi in homogeneous projective
// coordinates (Costello-Lange-Naehrig doubling / mixed addition, no inversion), plain binary over 6 x0 + 2 = 0x19d797039be763ba8, then
// the two correction lines through pi(Q) and -pi^2(Q).  The untwist is (x', y') -> (x' w^2, y' w^3), so a line through twist points,
// evaluated at P = (xP, yP) in G1 and scaled by a factor of Fp2 (which the final exponentiation kills), is the sparse value
//     l0 + l3 w + l4 w^3,      l0 = c0 yP, l3 = c1 xP, l4 = c2            (fp12_mul_by_line)
// Lines are computed as they are needed; nothing is tabulated.  e(infinity, Q) = e(P, infinity) = 1 (the Miller value is 1).  Nothing
// else in the loop depends on the data: the lanes of a wave diverge on the infinity flag alone.
//
// Final exponentiation.  pairing_final_exp raises to EXACTLY
//     d' = s (p^12 - 1) / r,        s = 2 x0 (6 x0^2 + 3 x0 + 1)        (s is coprime to r)
// -- the easy part (p^6 - 1)(p^2 + 1), then Fuentes-Castaneda et al.'s chain for s (p^4 - p^2 + 1) / r with cyclotomic squarings (three
// powers by x0).  This is the exponent gnark-crypto's bn254 FinalExponentiation realises as well.  e(P, Q)^s is as good a pairing as
// e(P, Q): bilinear, non-degenerate, of order r; every check of the verifier compares such values with each other.  The debug entry
// point mi_debug_pairing_dev and the Python reference of the tests (tests/pairing_ref.py: one pow(f, d')) are defined by this d'.
#pragma once
#include "fp12.cuh"

#define MI_BN_X0 0x44e992b44a6909f1ull          // 63 bits
#define MI_BN_ATE_LOW64 0x9d797039be763ba8ull   // 6 x0 + 2 = 2^64 + this

struct G2Proj { Fp2 x, y, z; };
struct MillerLine { Fp2 c0, c1, c2; };   // before the evaluation at P

// T <- 2 T and the tangent at T
MI_OOL void miller_double(G2Proj *t, MillerLine *l) {
    const Fp half = fp12c_half();
    const Fp2 a = fp2_mul_fp(t->x * t->y, half);
    const Fp2 b = fe_sqr(t->y), c = fe_sqr(t->z);
    const Fp2 e = fp12c_twist_b() * fp2_triple(c);
    const Fp2 f = fp2_triple(e);
    const Fp2 g = fp2_mul_fp(b + f, half);
    const Fp2 h = fe_sqr(t->y + t->z) - (b + c);
    const Fp2 j = fe_sqr(t->x);
    const Fp2 e2 = fe_sqr(e);
    t->x = a * (b - f);
    t->y = fe_sqr(g) - fp2_triple(e2);
    t->z = b * h;
    l->c0 = fe_neg(h); l->c1 = fp2_triple(j); l->c2 = e - b;
}
// T <- T + Q (Q affine, not infinity, T != +-Q: true for every step of the loop when Q has order r) and the chord through them
MI_OOL void miller_add(G2Proj *t, const Fp2 *qx, const Fp2 *qy, MillerLine *l) {
    const Fp2 theta = t->y - *qy * t->z, lambda = t->x - *qx * t->z;
    const Fp2 c = fe_sqr(theta), d = fe_sqr(lambda), e = lambda * d, f = t->z * c, g = t->x * d;
    const Fp2 h = e + f - fe_dbl(g);
    t->x = lambda * h;
    t->y = theta * (g - h) - e * t->y;
    t->z = t->z * e;
    l->c0 = lambda; l->c1 = fe_neg(theta); l->c2 = theta * *qx - lambda * *qy;
}
MI_HD void miller_apply(Fp12 *f, const MillerLine *l, const G1Aff *p) {
    const Fp2 l0 = fp2_mul_fp(l->c0, p->y), l3 = fp2_mul_fp(l->c1, p->x);
    fp12_mul_by_line(f, f, &l0, &l3, &l->c2);
}
MI_OOL void pairing_miller_loop(Fp12 *f, const G1Aff *p, const G2Aff *q) {
    *f = Fp12::one();
    if (p->is_inf() || q->is_inf()) return;
    G2Proj t{q->x, q->y, Fp2::one()};
    MillerLine l;
    for (int i = 63; i >= 0; i--) {   // bit 64 is the leading one
        fp12_sqr(f, f);
        miller_double(&t, &l);
        miller_apply(f, &l, p);
        if ((MI_BN_ATE_LOW64 >> i) & 1) {
            miller_add(&t, &q->x, &q->y, &l);
            miller_apply(f, &l, p);
        }
    }
    // pi(Q) = (conj(x) xi^((p-1)/3), conj(y) xi^((p-1)/2)); -pi^2(Q) = (x xi^((p^2-1)/3), -y xi^((p^2-1)/2))
    const Fp2 q1x = fp2_conj(q->x) * fp12c_frob1_2(), q1y = fp2_conj(q->y) * fp12c_frob1_3();
    const Fp2 q2x = fp2_mul_fp(q->x, fp12c_frob2_2().a0), q2y = fe_neg(fp2_mul_fp(q->y, fp12c_frob2_3().a0));
    miller_add(&t, &q1x, &q1y, &l);
    miller_apply(f, &l, p);
    miller_add(&t, &q2x, &q2y, &l);
    miller_apply(f, &l, p);
}
// x^x0 in the cyclotomic subgroup
MI_OOL void pairing_exp_x0(Fp12 *z, const Fp12 *x) {
    const Fp12 base = *x;
    Fp12 acc = base;
    for (int i = 61; i >= 0; i--) {
        fp12_cyclo_sqr(&acc, &acc);
        if ((MI_BN_X0 >> i) & 1) fp12_mul(&acc, &acc, &base);
    }
    *z = acc;
}
// f^((p^6 - 1)(p^2 + 1)): into the cyclotomic subgroup (0 -> 0)
MI_OOL void pairing_easy_part(Fp12 *z, const Fp12 *f) {
    Fp12 t, u;
    fp12_inv(&t, f);
    fp12_conj(&u, f);
    fp12_mul(&t, &u, &t);
    fp12_frob2(&u, &t);
    fp12_mul(z, &u, &t);
}
// f^d', d' as in the header
MI_OOL void pairing_final_exp(Fp12 *z, const Fp12 *f) {
    Fp12 m, t0, t1, t2, t3, t4;
    pairing_easy_part(&m, f);
    pairing_exp_x0(&t0, &m);
    fp12_conj(&t0, &t0);
    fp12_cyclo_sqr(&t0, &t0);             // m^(-2 x0)
    fp12_cyclo_sqr(&t1, &t0);
    fp12_mul(&t1, &t0, &t1);              // m^(-6 x0)
    pairing_exp_x0(&t2, &t1);
    fp12_conj(&t2, &t2);                  // m^(6 x0^2)
    fp12_conj(&t3, &t1);
    fp12_mul(&t1, &t2, &t3);
    fp12_cyclo_sqr(&t3, &t2);
    pairing_exp_x0(&t4, &t3);             // m^(12 x0^3)
    fp12_mul(&t4, &t1, &t4);
    fp12_mul(&t3, &t0, &t4);
    fp12_mul(&t0, &t2, &t4);
    fp12_mul(&t0, &m, &t0);
    fp12_frob1(&t2, &t3);
    fp12_mul(&t0, &t2, &t0);
    fp12_frob2(&t2, &t4);
    fp12_mul(&t0, &t2, &t0);
    fp12_conj(&t2, &m);
    fp12_mul(&t2, &t2, &t3);
    fp12_frob3(&t2, &t2);
    fp12_mul(z, &t2, &t0);
}

// ---------------------------------------------------------------- the checks a verifier makes on points it did not compute
// The eight words of x, read as one 256-bit integer, are below the modulus.  Every comparison in this library is one of words, and the
// arithmetic maps x and x + p (2p < 2^256) to the same result: a caller's value that is not reduced would be a SECOND encoding of the
// same element (and (p, p) a second infinity).  A verifier accepts exactly one encoding, so it asks this of every word it is given.
template <class P>
MI_HD bool fe_is_reduced(const Fe<P> &x) {
    Fe<P> t;
    return fe_sub_raw(t, x, Fe<P>::modulus()) != 0;   // x - p borrows
}
MI_HD bool g1_reduced(const G1Aff &p) { return fe_is_reduced(p.x) && fe_is_reduced(p.y); }
MI_HD bool g2_reduced(const G2Aff &q) { return fe_is_reduced(q.x.a0) && fe_is_reduced(q.x.a1) && fe_is_reduced(q.y.a0) && fe_is_reduced(q.y.a1); }
// host callers only (verify.hip, the host build of the tests).  Coordinates that are not reduced are no point of the curve: decided
// before any arithmetic touches them
MI_HD bool g1_on_curve(const G1Aff &p) {   // infinity counts as a point of the curve
    if (!g1_reduced(p)) return false;
    if (p.is_inf()) return true;
    return fe_sqr(p.y) == fe_sqr(p.x) * p.x + curve_b((const Fp *)0);
}
MI_HD bool g2_on_twist(const G2Aff &q) {   // of REDUCED coordinates (the device runs this one; the host asks g2_reduced first)
    if (q.is_inf()) return true;
    return fe_sqr(q.y) == fe_sqr(q.x) * q.x + fp12c_twist_b();
}
// on the twist AND of order dividing r: [r] Q = infinity by plain double-and-add (the twist's group has a cofactor)
MI_OOL bool g2_in_subgroup(const G2Aff *q) {
    if (!g2_on_twist(*q)) return false;
    u32 r[8];
#pragma unroll
    for (int i = 0; i < 8; i++) r[i] = FrParams::p[i];
    return xyzz_mul_256(G2X::from_affine(*q), r).is_inf();
}

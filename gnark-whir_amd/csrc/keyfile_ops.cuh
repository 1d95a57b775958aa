// The per-point text of the key-file codecs (include/mi355x_groth16_keyfile.h): what one lane of the bulk kernels of keyfile.hip does
// with one point of a proving key's stream, MI_HD so that the host build of the tests (tests/emu/emu_keyfile.cpp, overflow traps on)
// runs the same bodies.
//
//   decode     the decoders of decode_ops.cuh (g1_decode_by / g2_decode_by: one text for proofs and keys, so a string is malformed here
//              exactly where it is malformed there) over another chain for the root: a^((p + 1) / 4) by a FIXED WINDOW of 4 bits --
//              the 63 digits of the constant exponent, 14 products for the table, 4 squarings and at most one product per digit
//              (56 of the lower 62 are not 0): 318 products where the bit-by-bit chain takes 252 + 109.  The exponent is a constant, so the
//              digit is the same in every lane and the table is picked by a switch over NAMED values: nothing is indexed at run time,
//              nothing of the table leaves its registers.
//   raw        a raw point (ProvingKey.WriteRawTo: X | Y, flag 00, or flag 01 and nothing else) with what gnark's decoder asks of it:
//              coordinates below p, the curve's equation.
//   encode     the inverse of both: mi_g1_compress / mi_g2_compress (api.hip) per lane, and the raw form.
//   subgroup   membership of the r-torsion of the twist by the endomorphism psi = twist o Frobenius o untwist:
//                  a = [x0] Q,      a + Q + psi(a) + psi^2(a) == psi^3([2] a)                    x0 = MI_BN_X0, 63 bits
//              -- the test gnark-crypto's bn254 G2Affine.IsInSubGroup makes.  ONE 63-bit double-and-add where g2_in_subgroup
//              (pairing.cuh) takes 254 doublings; psi costs two products by the constants the Miller loop's last two steps use.
//              Coordinates stay XYZZ throughout (psi maps X, Y, ZZ, ZZZ coordinate by coordinate: conjugation is a field automorphism),
//              the equality is tested across denominators, nothing is inverted.
#pragma once
#include "decode_ops.cuh"

// ---------------------------------------------------------------- the root by a fixed window
struct FpWin4 { Fp t1, t2, t3, t4, t5, t6, t7, t8, t9, t10, t11, t12, t13, t14, t15; };
// digit d of (p + 1) / 4 in base 16, d = 0 the least significant; 63 digits, the top one is 12
MI_HD u32 fp_exp_sqrt_digit(int d) { return (fp_exp_sqrt_word(d >> 3) >> (4 * (d & 7))) & 15u; }
#define MI_KEYFILE_ROOT_DIGITS 63
MI_HD Fp fp_win4_pick(const FpWin4 &w, u32 d) {
    switch (d) {
    case 1: return w.t1;
    case 2: return w.t2;
    case 3: return w.t3;
    case 4: return w.t4;
    case 5: return w.t5;
    case 6: return w.t6;
    case 7: return w.t7;
    case 8: return w.t8;
    case 9: return w.t9;
    case 10: return w.t10;
    case 11: return w.t11;
    case 12: return w.t12;
    case 13: return w.t13;
    case 14: return w.t14;
    default: return w.t15;
    }
}
// a^((p + 1) / 4): word for word the value of fp_sqrt_candidate
MI_OOL void fp_sqrt_candidate_win4(Fp *y, const Fp *a) {
    FpWin4 w;
    w.t1 = *a;
    w.t2 = fe_sqr(w.t1); w.t3 = w.t2 * w.t1; w.t4 = fe_sqr(w.t2); w.t5 = w.t4 * w.t1; w.t6 = fe_sqr(w.t3); w.t7 = w.t6 * w.t1;
    w.t8 = fe_sqr(w.t4); w.t9 = w.t8 * w.t1; w.t10 = fe_sqr(w.t5); w.t11 = w.t10 * w.t1; w.t12 = fe_sqr(w.t6); w.t13 = w.t12 * w.t1;
    w.t14 = fe_sqr(w.t7); w.t15 = w.t14 * w.t1;
    Fp acc = fp_win4_pick(w, fp_exp_sqrt_digit(MI_KEYFILE_ROOT_DIGITS - 1));
    for (int d = MI_KEYFILE_ROOT_DIGITS - 2; d >= 0; d--) {
        acc = fe_sqr(fe_sqr(fe_sqr(fe_sqr(acc))));
        const u32 digit = fp_exp_sqrt_digit(d);   // of a constant: no lane diverges here
        if (digit) acc = acc * fp_win4_pick(w, digit);
    }
    *y = acc;
}
MI_OOL bool fp2_sqrt_win4(Fp2 *out, const Fp2 *a);
struct FpRootWin4 {
    static MI_HD void candidate(Fp *y, const Fp *a) { fp_sqrt_candidate_win4(y, a); }
    static MI_HD bool sqrt2(Fp2 *y, const Fp2 *a) { return fp2_sqrt_win4(y, a); }
};
MI_OOL bool fp2_sqrt_win4(Fp2 *out, const Fp2 *a) { return fp2_sqrt_by<FpRootWin4>(out, a); }

// ---------------------------------------------------------------- one point of a stream -> Montgomery words; false = refused, *out = (0, 0)
#define MI_KEYFILE_G1_BYTES(compressed) ((compressed) ? 32 : 64)
#define MI_KEYFILE_G2_BYTES(compressed) ((compressed) ? 64 : 128)
// raw: flag 00 and both coordinates below p and on the curve, or flag 01 and no other bit; 10 / 11 belong to a compressed stream
MI_HD bool g1_decode_raw(G1Aff *out, const uint8_t *in) {
    *out = G1Aff{Fp::zero(), Fp::zero()};
    const u32 flag = in[0] >> 6;
    if (flag >= 2) return false;
    if (flag == 1) return decode_is_clean_infinity(in, 64);
    Fp x, y;
    bool ok = fp_from_be32(&x, in, true);
    ok = fp_from_be32(&y, in + 32, false) && ok;
    ok = ok && fe_sqr(y) == fe_sqr(x) * x + curve_b((const Fp *)0);
    if (ok) *out = G1Aff{x, y};
    return ok;
}
MI_HD bool g2_decode_raw(G2Aff *out, const uint8_t *in) {
    *out = G2Aff{Fp2::zero(), Fp2::zero()};
    const u32 flag = in[0] >> 6;
    if (flag >= 2) return false;
    if (flag == 1) return decode_is_clean_infinity(in, 128);
    Fp2 x, y;
    bool ok = fp_from_be32(&x.a1, in, true);
    ok = fp_from_be32(&x.a0, in + 32, false) && ok;
    ok = fp_from_be32(&y.a1, in + 64, false) && ok;
    ok = fp_from_be32(&y.a0, in + 96, false) && ok;
    ok = ok && fe_sqr(y) == fe_sqr(x) * x + fp12c_twist_b();
    if (ok) *out = G2Aff{x, y};
    return ok;
}
MI_HD bool g1_decode_stream(G1Aff *out, const uint8_t *in, bool compressed) { return compressed ? g1_decode_by<FpRootWin4>(out, in) : g1_decode_raw(out, in); }
MI_HD bool g2_decode_stream(G2Aff *out, const uint8_t *in, bool compressed) { return compressed ? g2_decode_by<FpRootWin4>(out, in) : g2_decode_raw(out, in); }

// ---------------------------------------------------------------- Montgomery words -> one point of a stream
MI_HD void encode_infinity(uint8_t *out, int len) {
    out[0] = 0x40;
    for (int i = 1; i < len; i++) out[i] = 0;
}
MI_HD void g1_encode_stream(uint8_t *out, const G1Aff &p, bool compressed) {
    if (p.is_inf()) { encode_infinity(out, MI_KEYFILE_G1_BYTES(compressed)); return; }
    fe_to_be32(out, p.x);
    if (compressed) out[0] |= fp_lex_largest(p.y) ? 0xC0 : 0x80;
    else fe_to_be32(out + 32, p.y);
}
MI_HD void g2_encode_stream(uint8_t *out, const G2Aff &p, bool compressed) {
    if (p.is_inf()) { encode_infinity(out, MI_KEYFILE_G2_BYTES(compressed)); return; }
    fe_to_be32(out, p.x.a1);
    fe_to_be32(out + 32, p.x.a0);
    if (compressed) out[0] |= fp2_lex_largest(p.y) ? 0xC0 : 0x80;
    else { fe_to_be32(out + 64, p.y.a1); fe_to_be32(out + 96, p.y.a0); }
}

// ---------------------------------------------------------------- the r-torsion of the twist by psi
// psi(x, y) = (conj(x) xi^((p - 1) / 3), conj(y) xi^((p - 1) / 2)); ZZ and ZZZ are conjugated with the numerators they divide
MI_HD G2X g2_psi(const G2X &p) { return G2X{fp2_conj(p.x) * fp12c_frob1_2(), fp2_conj(p.y) * fp12c_frob1_3(), fp2_conj(p.zz), fp2_conj(p.zzz)}; }
MI_HD bool g2x_equal(const G2X &p, const G2X &q) {
    if (p.is_inf() || q.is_inf()) return p.is_inf() && q.is_inf();
    return p.x * q.zz == q.x * p.zz && p.y * q.zzz == q.y * p.zzz;
}
// [x0] Q, Q affine and not infinity; bit 62 of x0 is its leading one
MI_OOL void g2_mul_x0(G2X *out, const G2Aff *q) {
    G2X acc{q->x, q->y, Fp2::one(), Fp2::one()};
    for (int i = 61; i >= 0; i--) {
        acc = xyzz_dbl(acc);
        if ((MI_BN_X0 >> i) & 1) xyzz_madd(acc, *q, false);   // x0 is a constant: no lane diverges here
    }
    *out = acc;
}
// Q on the twist (the caller has seen to that: a decoder accepted it) -> of order dividing r.  Infinity is a member.
// (the three additions behind the scalar multiple go through one out-of-line copy: inlined, their temporaries beside four live points
// took the kernel past 256 registers)
MI_OOL void g2x_add_call(G2X *acc, const G2X *q) { xyzz_add(*acc, *q); }
MI_OOL bool g2_in_subgroup_psi(const G2Aff *q) {
    if (q->is_inf()) return true;
    G2X a, lhs, p;
    g2_mul_x0(&a, q);
    lhs = G2X{q->x, q->y, Fp2::one(), Fp2::one()};
    g2x_add_call(&lhs, &a);
    p = g2_psi(a);
    g2x_add_call(&lhs, &p);
    p = g2_psi(p);
    g2x_add_call(&lhs, &p);
    p = g2_psi(g2_psi(g2_psi(xyzz_dbl(a))));
    return g2x_equal(lhs, p);
}

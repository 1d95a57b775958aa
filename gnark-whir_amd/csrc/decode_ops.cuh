// Reading a proof back from gnark's bytes (Proof.WriteTo): the square roots in Fp and Fp2 and the decoders of a
// compressed G1 / G2 point -- the inverse of mi_g1_compress / mi_g2_compress (api.hip).  One record per lane / per call, MI_HD: the
// decode kernels (verify_bytes.hip), the host entry point mi_proof_read (proof_read.hip) and the host build of the tests
// (tests/emu/emu_decode.cpp, overflow traps on) run this text.
//
// The work of a lane does not depend on its data: every exponent is fixed, every choice is a select, and the one data-dependent thing
// is the accept at the end (y^2 == a).  Lanes of a wave diverge on the two flag bits alone (an infinity has nothing to compute).
//
// ONE ENCODING, as everywhere in the verifier (include/mi355x_groth16_verify.h).  Byte 0 carries two flag bits:
//     10 y is the smaller of (y, p - y)    11 the larger    01 infinity    00 uncompressed
// and a string is MALFORMED when X (either component on G2) is not below p (possible: p < 2^254), when the flag is 00 (a proof holds
// compressed points only), when the flag is 01 and any other bit is set, or when X has no y on the curve.  "Larger" on G2 is decided on
// y.A1, or on y.A0 when y.A1 = 0, as mi_g2_compress decides it.  decode(compress(P)) == P word for word, infinity (0, 0) included.
#pragma once
#include "pairing.cuh"

// (p + 1) / 4 and (p - 1) / 2, plain integers, least significant word first
MI_HD u32 fp_exp_sqrt_word(int i) {
    constexpr u32 e[8] = {0xb61f3f52u, 0x4f082305u, 0x5a1c72a3u, 0x65e05aa4u, 0xa0605617u, 0x6e14116du, 0xb84c680au, 0x0c19139cu};
    return e[i];
}
MI_HD u32 fp_half_word(int i) {
    constexpr u32 h[8] = {0x6c3e7ea3u, 0x9e10460bu, 0xb438e546u, 0xcbc0b548u, 0x40c0ac2eu, 0xdc2822dbu, 0x7098d014u, 0x18322739u};
    return h[i];
}

// a^((p + 1) / 4): THE root of a that is itself a residue when a is one (p = 3 mod 4), a root of -a otherwise; 0 -> 0
MI_OOL void fp_sqrt_candidate(Fp *y, const Fp *a) {
    Fp acc = Fp::one();
    const Fp base = *a;
    for (int i = 251; i >= 0; i--) {   // the exponent has 252 bits
        acc = fe_sqr(acc);
        if ((fp_exp_sqrt_word(i >> 5) >> (i & 31)) & 1) acc = acc * base;   // the exponent is a constant: no lane diverges here
    }
    *y = acc;
}
// y = a^((p + 1) / 4); true when y^2 == a
MI_HD bool fp_sqrt(Fp *y, const Fp &a) {
    fp_sqrt_candidate(y, &a);
    return fe_sqr(*y) == a;
}
MI_HD Fp fp_select(bool c, const Fp &x, const Fp &y) {
    Fp z;
#pragma unroll
    for (int i = 0; i < 8; i++) z.l[i] = c ? x.l[i] : y.l[i];
    return z;
}
// the canonical integer of a Montgomery value is above (p - 1) / 2
MI_HD bool fp_lex_largest(const Fp &mont) {
    const Fp c = fe_from_mont(mont);
    u64 b = 0;   // (p - 1) / 2 - c borrows  <=>  c > (p - 1) / 2
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const u64 d = (u64)fp_half_word(i) - c.l[i] - b;
        b = (d >> 32) & 1;
    }
    return b != 0;
}

// A square root in Fp2 = Fp[u] / (u^2 + 1), total: with x = x0 + x1 u and x^2 = a,
//     x0^2 - x1^2 = a0,  2 x0 x1 = a1,  x0^2 + x1^2 = +-s  where s^2 = a0^2 + a1^2 (the norm),
// so x0^2 = (a0 + s') / 2 and x1^2 = (s' - a0) / 2 for the sign s' of s that makes the first a residue.  Both halves are taken as
// roots (four fixed exponentiations in all, no inversion); the sign of x1 is then set by 2 x0 x1 == a1.  Nothing is divided, so the
// degenerate inputs take the same path as every other: a = 0 gives 0; a1 = 0 with a0 a residue gives s = a0, (x0, x1) = (sqrt a0, 0);
// a1 = 0 with a0 a non-residue gives s = -a0, x0^2 = 0 and x1^2 = -a0, the purely imaginary root (where the "complex method" divides
// by 2 x0 = 0); a norm that is a non-residue has no s and whatever comes out fails the final x^2 == a, which alone decides.
// Root: who raises to (p + 1) / 4 (FpRootBitwise below; the windowed chain of keyfile_ops.cuh) -- the same value whichever chain.
template <class Root>
MI_HD bool fp2_sqrt_by(Fp2 *out, const Fp2 *a) {
    const Fp half = fp12c_half();
    const Fp n = fe_sqr(a->a0) + fe_sqr(a->a1);
    Fp s, cp, cm, x1;
    Root::candidate(&s, &n);
    const Fp hp = (a->a0 + s) * half, hm = (a->a0 - s) * half;
    Root::candidate(&cp, &hp);
    Root::candidate(&cm, &hm);
    const bool plus = fe_sqr(cp) == hp;
    const Fp x0 = fp_select(plus, cp, cm);
    const Fp k = fp_select(plus, hp, hm) - a->a0;   // (s' - a0) / 2 = (a0 + s') / 2 - a0
    Root::candidate(&x1, &k);
    const Fp t = x0 * x1;
    x1 = fp_select(t + t == a->a1, x1, fe_neg(x1));
    const Fp2 x{x0, x1};
    *out = x;
    return fe_sqr(x) == *a;
}
MI_OOL bool fp2_sqrt(Fp2 *out, const Fp2 *a);
// the roots of a proof's handful of points: the bit-by-bit chain
struct FpRootBitwise {
    static MI_HD void candidate(Fp *y, const Fp *a) { fp_sqrt_candidate(y, a); }
    static MI_HD bool sqrt2(Fp2 *y, const Fp2 *a) { return fp2_sqrt(y, a); }
};
MI_OOL bool fp2_sqrt(Fp2 *out, const Fp2 *a) { return fp2_sqrt_by<FpRootBitwise>(out, a); }

// 32 bytes, big-endian, the two flag bits of byte 0 cleared -> Montgomery form; false when the integer is not below p
MI_HD bool fp_from_be32(Fp *out, const uint8_t *in, bool mask_flags) {
    Fp c, t;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint8_t *w = in + 28 - 4 * i;
        u32 b0 = w[0];
        if (mask_flags && i == 7) b0 &= 0x3fu;
        c.l[i] = (b0 << 24) | ((u32)w[1] << 16) | ((u32)w[2] << 8) | (u32)w[3];
    }
    const bool below = fe_sub_raw(t, c, Fp::modulus()) != 0;
    if (!below) c = Fp::zero();   // nothing that is not reduced reaches the arithmetic
    *out = fe_to_mont(c);
    return below;
}
// Montgomery form -> 32 bytes, big-endian, canonical
template <class P>
MI_HD void fe_to_be32(uint8_t *out, const Fe<P> &mont) {
    const Fe<P> c = fe_from_mont(mont);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint8_t *w = out + 28 - 4 * i;
        w[0] = (uint8_t)(c.l[i] >> 24); w[1] = (uint8_t)(c.l[i] >> 16); w[2] = (uint8_t)(c.l[i] >> 8); w[3] = (uint8_t)c.l[i];
    }
}
// the flag is 01: a well-formed infinity has no other bit set in its len bytes
MI_HD bool decode_is_clean_infinity(const uint8_t *in, int len) {
    u32 o = in[0] & 0x3fu;
    for (int i = 1; i < len; i++) o |= in[i];
    return o == 0;
}

// false = malformed, and *out = (0, 0)
template <class Root>
MI_HD bool g1_decode_by(G1Aff *out, const uint8_t *in) {
    *out = G1Aff{Fp::zero(), Fp::zero()};
    const u32 flag = in[0] >> 6;
    if (flag == 0) return false;
    if (flag == 1) return decode_is_clean_infinity(in, 32);
    Fp x, y;
    bool ok = fp_from_be32(&x, in, true);
    const Fp rhs = fe_sqr(x) * x + curve_b((const Fp *)0);
    Root::candidate(&y, &rhs);
    ok = fe_sqr(y) == rhs && ok;
    const bool want_largest = flag == 3;
    y = fp_select(fp_lex_largest(y) == want_largest, y, fe_neg(y));
    ok = ok && fp_lex_largest(y) == want_largest;   // y = 0 has one encoding (no such point exists on this curve: its order is odd)
    if (ok) *out = G1Aff{x, y};
    return ok;
}
MI_HD bool g1_decode(G1Aff *out, const uint8_t *in) { return g1_decode_by<FpRootBitwise>(out, in); }
MI_HD bool fp2_lex_largest(const Fp2 &y) { return y.a1.is_zero() ? fp_lex_largest(y.a0) : fp_lex_largest(y.a1); }
template <class Root>
MI_HD bool g2_decode_by(G2Aff *out, const uint8_t *in) {
    *out = G2Aff{Fp2::zero(), Fp2::zero()};
    const u32 flag = in[0] >> 6;
    if (flag == 0) return false;
    if (flag == 1) return decode_is_clean_infinity(in, 64);
    Fp2 x, y;
    bool ok = fp_from_be32(&x.a1, in, true);
    ok = fp_from_be32(&x.a0, in + 32, false) && ok;
    const Fp2 rhs = fe_sqr(x) * x + fp12c_twist_b();
    ok = Root::sqrt2(&y, &rhs) && ok;
    const bool want_largest = flag == 3;
    const bool keep = fp2_lex_largest(y) == want_largest;
    y = Fp2{fp_select(keep, y.a0, fe_neg(y.a0)), fp_select(keep, y.a1, fe_neg(y.a1))};
    ok = ok && fp2_lex_largest(y) == want_largest;
    if (ok) *out = G2Aff{x, y};
    return ok;
}
MI_HD bool g2_decode(G2Aff *out, const uint8_t *in) { return g2_decode_by<FpRootBitwise>(out, in); }

// ---------------------------------------------------------------- Proof.WriteTo's layout
//     Ar (32) | Bs (64) | Krs (32) | u32 big-endian count | count x 32 commitments | pok (32)          164 + 32 count bytes
#define MI_PROOF_BYTES_BASE 164
#define MI_PROOF_OFF_BS 32
#define MI_PROOF_OFF_KRS 96
#define MI_PROOF_OFF_COUNT 128
#define MI_PROOF_OFF_COMMITMENTS 132
MI_HD size_t proof_bytes_len(u32 n_commitments) { return (size_t)MI_PROOF_BYTES_BASE + 32 * (size_t)n_commitments; }
MI_HD u32 proof_bytes_count(const uint8_t *proof) {
    const uint8_t *c = proof + MI_PROOF_OFF_COUNT;
    return ((u32)c[0] << 24) | ((u32)c[1] << 16) | ((u32)c[2] << 8) | (u32)c[3];
}
// G1 slot s of a proof with nc commitments: 0 Ar, 1 Krs, 2 .. 2 + nc commitments, 2 + nc pok -> its byte offset
MI_HD size_t proof_g1_slot_offset(u32 s) { return s == 0 ? 0 : s == 1 ? MI_PROOF_OFF_KRS : MI_PROOF_OFF_COMMITMENTS + 32 * (size_t)(s - 2); }
MI_HD u32 proof_g1_slots(u32 n_commitments) { return 3 + n_commitments; }

// Test records of the 9 x 29-bit arithmetic (field29.cuh, curve29.cuh, curve29_g2.cuh): one primitive or one group step per record, the
// same dispatch on the host (tests/emu/emu.cpp, overflow traps on) and on the device (mi_debug_limb29_op_dev, one record per lane), so the
// two builds can be compared limb for limb.  Nothing in the product calls this file.
//
// Record layout (u32 words; the numbers are mirrored in include/mi355x_groth16_debug.h):
//   in  [L29_IN_WORDS]: operands a..h as nine limbs each at in[9 k] (primitives); or an accumulator state at in[0..71] -- G1: X | Y | ZZ | ZZZ,
//                       nine limbs each; G2: component c at in[18 c], a0 then a1 -- an operand at in[72..] (packed 8 x u32 words per
//                       coordinate, the form the tables and the partial sums keep) and flags at in[136]: bit 0 = the accumulator is the point
//                       at infinity, bit 1 = negate the operand
//   out [L29_OUT_WORDS]: a result in limbs at out[0..]; a group step leaves the state at out[0..71] (same layout) and its infinity flag at out[72]
#pragma once
#include "curve29.cuh"
#include "curve29_g2.cuh"

#define L29_IN_WORDS 144
#define L29_OUT_WORDS 80
#define L29_OPERAND 72
#define L29_FLAGS 136
#define L29_OUT_INF 72
enum {
    // primitives over Fp: out[0..8] unless noted
    L29_MUL = 0, L29_MUL2 = 1, L29_SUB8 = 2, L29_SUB4 = 3, L29_SUB2 = 4, L29_WNORM = 5, L29_CONDSUB4 = 6, L29_CONDSUB2 = 7, L29_SQR = 8,
    L29_MUL4 = 9, L29_NORM = 10,
    L29_UNPACK = 11,     // in[0..7] words -> limbs
    L29_PACK = 12,       // a -> out[0..7] words
    L29_TO_STD = 13,     // a -> out[0..7]: canonical standard Montgomery form
    L29_FROM_STD = 14,   // in[0..7] standard form -> limbs
    L29_BELOW_2P = 15,
    L29_F2_IS_ZERO = 16, // (a, b) as one Fp2 element -> out[0] = 0 / 1
    L29_PRIM_END = 17,
    // G1 steps (curve29.cuh)
    L29_G1_MADD = 20,    // operand: 16 words x | y
    L29_G1_ADD = 21,     // operand: 32 words, a partial sum as g1x29_store_rp leaves it, read back with g1x29_load_rp
    L29_G1_STORE = 22,   // g1x29_store_rp then g1x29_load_rp: out[40..71] = the 32 stored words, out[0..35] / out[72] = what loads back
    // G2 steps (curve29_g2.cuh; on the device through the level-1 kernel's LDS accumulator image, msm_g2.hip)
    L29_G2_MADD = 23,    // operand: 32 words x.a0 | x.a1 | y.a0 | y.a1
    L29_G2_ADD = 24,     // operand: 64 words X | Y | ZZ | ZZZ packed (what the G2 partial sums hold); ZZ = 0 exactly is infinity
    L29_G2_STORE = 25,   // the packed partial sum the level kernels store: out[0..63]
    L29_OP_END = 26
};

MI_HD F29 l29_get(const u32 *w) { F29 x;
#pragma unroll
    for (int i = 0; i < 9; i++) x.l[i] = w[i];
    return x; }
MI_HD void l29_put(u32 *w, const F29 &x) {
#pragma unroll
    for (int i = 0; i < 9; i++) w[i] = x.l[i];
}

// primitives and G1 steps; returns -1 for an op it does not handle
MI_HD int limb29_op_g1(int op, const u32 *in, u32 *out) {
    typedef FpParams P;
    const u32 flags = in[L29_FLAGS];
    if (op >= L29_G1_MADD && op <= L29_G1_STORE) {
        G1X29 acc;
        acc.x = l29_get(in); acc.y = l29_get(in + 9); acc.zz = l29_get(in + 18); acc.zzz = l29_get(in + 27);
        acc.inf = flags & 1;
        if (op == L29_G1_MADD) g1x29_madd(acc, in + L29_OPERAND, (flags & 2) != 0);
        else if (op == L29_G1_ADD) g1x29_add(acc, g1x29_load_rp(in + L29_OPERAND));
        else { g1x29_store_rp(acc, out + 40); acc = g1x29_load_rp(out + 40); }
        l29_put(out, acc.x); l29_put(out + 9, acc.y); l29_put(out + 18, acc.zz); l29_put(out + 27, acc.zzz);
        out[L29_OUT_INF] = acc.inf;
        return 0;
    }
    const F29 a = l29_get(in), b = l29_get(in + 9), c = l29_get(in + 18), d = l29_get(in + 27);
    switch (op) {
    case L29_MUL: l29_put(out, f29_mul<P>(a, b)); break;
    case L29_MUL2: l29_put(out, f29_mul2<P>(a, b, c, d)); break;
    case L29_SUB8: l29_put(out, f29_sub<P>(a, b, P29<P>::c8)); break;
    case L29_SUB4: l29_put(out, f29_sub<P>(a, b, P29<P>::c4)); break;
    case L29_SUB2: l29_put(out, f29_sub<P>(a, b, P29<P>::c2)); break;
    case L29_WNORM: l29_put(out, f29_wnorm(a)); break;
    case L29_CONDSUB4: l29_put(out, f29_condsub(a, P29<P>::p4)); break;
    case L29_CONDSUB2: l29_put(out, f29_condsub(a, P29<P>::p2)); break;
    case L29_SQR: l29_put(out, f29_sqr<P>(a)); break;
    case L29_MUL4: l29_put(out, f29_mul4<P>(a, b, c, d, l29_get(in + 36), l29_get(in + 45), l29_get(in + 54), l29_get(in + 63))); break;
    case L29_NORM: l29_put(out, f29_norm(a)); break;
    case L29_UNPACK: l29_put(out, f29_unpack(in)); break;
    case L29_PACK: f29_pack(a, out); break;
    case L29_TO_STD: { const Fp s = f29_to_std<P>(a);
#pragma unroll
        for (int i = 0; i < 8; i++) out[i] = s.l[i];
        break; }
    case L29_FROM_STD: { Fp s;
#pragma unroll
        for (int i = 0; i < 8; i++) s.l[i] = in[i];
        l29_put(out, f29_from_std<P>(s)); break; }
    case L29_BELOW_2P: l29_put(out, f29_below_2p(a)); break;
    case L29_F2_IS_ZERO: out[0] = f2_29_is_zero_mod_p(F2_29{a, b}); break;
    default: return -1;
    }
    return 0;
}

// G2 mixed / full addition on an accumulator Acc (ld / st per component: registers on the host, the LDS image on the device)
template <class Acc>
MI_HD int limb29_op_g2(int op, Acc &A, const u32 *in, u32 *out) {
    if (op != L29_G2_MADD && op != L29_G2_ADD) return -1;
    const u32 flags = in[L29_FLAGS];
    for (int c = 0; c < 4; c++) A.st(c, F2_29{l29_get(in + 18 * c), l29_get(in + 18 * c + 9)});
    bool inf = flags & 1;
    const u32 *q = in + L29_OPERAND;
    if (op == L29_G2_MADD) {
        g2x29_madd(A, inf, q, (flags & 2) != 0);
    } else {
        u32 any = 0;
        for (int i = 32; i < 48; i++) any |= q[i];   // ZZ = 0 exactly: only the stored infinity (k_msm_accum_xyzz_g2_29)
        g2x29_add(A, inf, [q](int comp) { return f2_29_unpack(q + 16 * comp); }, any == 0);
    }
    for (int c = 0; c < 4; c++) { const F2_29 v = A.ld(c); l29_put(out + 18 * c, v.a0); l29_put(out + 18 * c + 9, v.a1); }
    out[L29_OUT_INF] = inf;
    return 0;
}

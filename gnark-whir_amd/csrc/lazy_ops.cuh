// Test records of the lazy 8 x 32-bit arithmetic under the NTT (field.cuh "lazy arithmetic", ntt_tile.cuh "lazy butterflies"): one primitive or
// one butterfly per record, the same dispatch on the host (tests/emu/emu.cpp, overflow traps on) and on the device (mi_debug_lazy_op_dev, one
// record per lane), so the inline-asm bodies and the portable ones can be compared word for word.  Nothing in the product calls this file.
//
// Record layout (u32 words; the numbers are mirrored in include/mi355x_groth16_debug.h), every operand over Fr:
//   in  [LZ_IN_WORDS]:  x at in[0..7], y at in[8..15], w (a twiddle, below p) at in[16..23]
//   out [LZ_OUT_WORDS]: the result at out[0..7]; a butterfly leaves x0 at out[0..7] and x1 at out[8..15].  Words an op does not write are zero.
#pragma once
#include "ntt_tile.cuh"

#define LZ_IN_WORDS 24
#define LZ_OUT_WORDS 16
enum {
    LZ_ADD_NORED = 0,    // fe_add_nored(x, y)                     x + y < 2^256
    LZ_SUB_PLUS2P = 1,   // fe_sub_plus2p(x, y)                    x, y < 2p
    LZ_CONDSUB_2P = 2,   // fe_condsub_2p(x)                       x < 4p
    LZ_CANON = 3,        // fe_canon(x)                            x < 4p
    LZ_MUL_LAZY = 4,     // fe_mul_lazy(x, y), raw                 x < 4p and y < p, or x, y < 2p
    LZ_MUL_LAZY2 = 5,    // ntt_mul_lazy2(x, y)                    x, y < 4p
    LZ_BFLY_DIF = 6,     // ntt_bfly_dif(x, y, &w), both outputs   x, y < 2p
    LZ_BFLY_DIF_1 = 7,   // the same with w == nullptr
    LZ_BFLY_DIT = 8,     // ntt_bfly_dit(x, y, &w), both outputs   x, y < 4p
    LZ_BFLY_DIT_1 = 9,   // the same with w == nullptr
    LZ_STORE_SUB = 10,   // what ntt_tile_store does with NttPass::store_sub on a canonical pass: fe_canon(fe_sub_plus2p(fe_condsub_2p(x), fe_condsub_2p(y)))
    LZ_OP_END = 11
};

MI_HD Fr lz_get(const u32 *w) { Fr x;
#pragma unroll
    for (int i = 0; i < 8; i++) x.l[i] = w[i];
    return x; }
MI_HD void lz_put(u32 *w, const Fr &x) {
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = x.l[i];
}

// returns -1 for an op it does not handle
MI_HD int lazy_op(int op, const u32 *in, u32 *out) {
    Fr x = lz_get(in), y = lz_get(in + 8);
    const Fr w = lz_get(in + 16);
    switch (op) {
    case LZ_ADD_NORED: lz_put(out, fe_add_nored(x, y)); break;
    case LZ_SUB_PLUS2P: lz_put(out, fe_sub_plus2p(x, y)); break;
    case LZ_CONDSUB_2P: lz_put(out, fe_condsub_2p(x)); break;
    case LZ_CANON: lz_put(out, fe_canon(x)); break;
    case LZ_MUL_LAZY: lz_put(out, fe_mul_lazy(x, y)); break;
    case LZ_MUL_LAZY2: lz_put(out, ntt_mul_lazy2(x, y)); break;
    case LZ_BFLY_DIF: ntt_bfly_dif(x, y, &w); lz_put(out, x); lz_put(out + 8, y); break;
    case LZ_BFLY_DIF_1: ntt_bfly_dif(x, y, nullptr); lz_put(out, x); lz_put(out + 8, y); break;
    case LZ_BFLY_DIT: ntt_bfly_dit(x, y, &w); lz_put(out, x); lz_put(out + 8, y); break;
    case LZ_BFLY_DIT_1: ntt_bfly_dit(x, y, nullptr); lz_put(out, x); lz_put(out + 8, y); break;
    case LZ_STORE_SUB: lz_put(out, fe_canon(fe_sub_plus2p(fe_condsub_2p(x), fe_condsub_2p(y)))); break;
    default: return -1;
    }
    return 0;
}

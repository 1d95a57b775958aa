// What the two sparse products over Fr share (setup.hip: column sums of the transposed product; r1cs.hip: row sums of M W): 32-byte
// loads and stores of an Fr, the sum over a wave, and the split of skewed lists -- a list of at most SPARSE_SHORT entries is summed by
// one lane (64 lists packed in a wave), a longer one is cut into pieces of SPARSE_CHUNK entries that a wave sums with its lanes striding
// over the piece, and a last pass adds a list's partials.  Field addition is exact and commutative: every order gives the same bits.
#pragma once
#include "field.cuh"

constexpr u32 SPARSE_SHORT = 16;
constexpr u32 SPARSE_CHUNK = 512;

MI_D Fr ld_fr(const Fr *p) {
    const uint4 *q = reinterpret_cast<const uint4 *>(p);
    const uint4 a = q[0], b = q[1];
    Fr r;
    r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w; r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
    return r;
}
MI_D void st_fr(Fr *p, const Fr &v) {
    uint4 *q = reinterpret_cast<uint4 *>(p);
    q[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
    q[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}
// the sum of v over the 64 lanes of a wave, in every lane (all lanes active)
MI_D Fr wave_sum(Fr v) {
#pragma unroll 1
    for (int o = 32; o >= 1; o >>= 1) {
        Fr t;
#pragma unroll
        for (int i = 0; i < 8; i++) t.l[i] = (u32)__shfl_xor((int)v.l[i], o);
        v = v + t;
    }
    return v;
}

// What the two sparse products over Fr share (setup.hip: column sums of the transposed product; r1cs.hip: row sums of M W), and the one
// home of the split sum of skewed lists.  A list is a run [lo, lo + len) of 8-byte entries; what an entry contributes is the caller's
// Term, `void term(Fr &acc, uint2 entry)`, which adds the entry's term into acc (an accumulate form, so that a term that is +-W[wire]
// costs an addition and no product).
//   short   a list of at most SPARSE_SHORT entries is summed by one lane, 64 lists packed in a wave          sparse_sum_short
//   cut     a longer one gets a SparseLong record and is cut into pieces of SPARSE_CHUNK entries            sparse_cut
//   pieces  a wave sums one piece, its lanes striding over it and meeting in a butterfly, into a partial    sparse_sum_pieces
//   combine a last wave pass adds a list's partials and stores the list's sum                               sparse_combine
// List lengths are heavily skewed -- the constant wire sits in a large share of all rows, a few linear combinations hold thousands of
// wires, most lists one to four entries -- and a lane per list would leave one lane on millions of entries.
// Field addition is exact and commutative: every order gives the same bits.
// The bodies are per thread (short) or grid-stride over waves (pieces, combine: any grid of whole waves); the __global__ wrappers, who
// plans (setup.hip on the device, per call; r1cs.hip on the host, at load) and how matrices are batched stay with the callers.
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

// a list of more than SPARSE_SHORT entries: where its sum goes (the caller's index: a column, a row) and its pieces
struct alignas(16) SparseLong { u32 index, first_piece, n_pieces, pad; };
static_assert(sizeof(SparseLong) == 16, "one 16-byte load");
// THE cut rule: the pieces (first entry, entries) of the list [lo, lo + len), every one of SPARSE_CHUNK entries but the last.  Returns
// their number; writes them unless pieces is null (a planner that has to claim room for them first asks for the number alone).
MI_HD u32 sparse_cut(u32 lo, u32 len, uint2 *pieces) {
    const u32 np = (len + SPARSE_CHUNK - 1) / SPARSE_CHUNK;
    if (pieces) {
        for (u32 c = 0; c < np; c++) {
            const u32 left = len - c * SPARSE_CHUNK;
            pieces[c] = make_uint2(lo + c * SPARSE_CHUNK, left < SPARSE_CHUNK ? left : SPARSE_CHUNK);
        }
    }
    return np;
}

// one lane: the sum of a short list
template <class Term>
MI_D Fr sparse_sum_short(const uint2 *entries, u32 lo, u32 len, const Term &term) {
    Fr acc = Fr::zero();
    for (u32 e = lo; e < lo + len; e++) term(acc, entries[e]);
    return acc;
}
// a wave per piece (grid-stride): partial[piece] = the sum of its entries
template <class Term>
MI_D void sparse_sum_pieces(Fr *partial, const uint2 *pieces, u32 n_pieces, const uint2 *entries, const Term &term) {
    const u32 lane = threadIdx.x & 63, wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    for (u32 it = wave; it < n_pieces; it += n_waves) {
        const uint2 pc = pieces[it];
        Fr acc = Fr::zero();
        for (u32 k = lane; k < pc.y; k += 64) term(acc, entries[pc.x + k]);
        acc = wave_sum(acc);
        if (lane == 0) st_fr(partial + it, acc);
    }
}
// a wave per long list (grid-stride): the sum of its partials, to out[the list's index] (compact: to out[its place in longs])
MI_D void sparse_combine(Fr *out, const SparseLong *longs, u32 n_long, const Fr *partial, bool compact) {
    const u32 lane = threadIdx.x & 63, wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    for (u32 it = wave; it < n_long; it += n_waves) {
        const SparseLong ll = longs[it];
        Fr acc = Fr::zero();
        for (u32 k = lane; k < ll.n_pieces; k += 64) acc = acc + ld_fr(partial + ll.first_piece + k);
        acc = wave_sum(acc);
        if (lane == 0) st_fr(out + (compact ? it : ll.index), acc);
    }
}

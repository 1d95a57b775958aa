// kSum of a whole batch (include/mi355x_groth16_verify_ksum.h): what the kernels of csrc/ksum.hip and the host build of the tests
// (tests/emu/emu_ksum.cpp, tests/cpp/ksum_asan.cpp; overflow traps on) both run, one record per lane.  All proofs of a batch share the
// bases K[1..] of their key, so the public-input sums are a matrix of scalars times ONE vector of fixed points: fixed_base.hip's window
// table, for many bases.
//   table    T[j][w][d - 1] = d 2^(c w) K[1 + j], j < ns, w < ceil(254 / c), 1 <= d < 2^c; affine, (0, 0) = infinity.  c is 8, 4 or 2: the
//            largest whose table fits the key's byte budget (ksum_window_bits), 0 when none does
//   build    ksum_rows_lane: 2^(c w) K_j by doublings down a lane; ksum_multiples_lane: the multiples of a row by repeated addition;
//            then one batched conversion to affine (batch_affine.cuh)
//   sum      the (j, w) terms of one proof are cut into slices (ksum_slices); ksum_lane adds the table entries of one slice's non-zero
//            digits with XYZZ mixed additions -- one partial sum; ksum_strided_sum adds a proof's partials with the general addition
//            (its doubling and cancelling branches: two bases may be equal or opposite)
// Every result goes back to affine through the field's one inversion, so it has one encoding: the words mi_msm_g1_dev gives for the row.
#pragma once
#include "curve.cuh"

#define MI_KSUM_SCALAR_BITS 254u                       // a scalar is below r < 2^254
#define MI_KSUM_MAX_SLICES 1024u                       // slices of one proof's terms at most
#define MI_KSUM_TARGET_LANES ((uint64_t)1 << 18)       // lanes the sum kernel is cut for: MI_KSUM_GRID_CAP workgroups of 64
#define MI_KSUM_GRID_CAP 4096u                         // workgroups of a grid; the kernels walk their items with the grid's stride
#define MI_KSUM_BUILD_CHUNK ((uint64_t)1 << 18)        // table entries converted to affine at a time while a table is built

MI_HD u32 ksum_windows(u32 c) { return (MI_KSUM_SCALAR_BITS + c - 1) / c; }
MI_HD uint64_t ksum_row_entries(u32 c) { return ((uint64_t)1 << c) - 1; }                                   // of one (j, w)
MI_HD uint64_t ksum_table_bytes(u32 ns, u32 c) { return (uint64_t)ns * ksum_windows(c) * ksum_row_entries(c) * sizeof(G1Aff); }
// The window width of a key with ns bases under a byte budget: 8, 4 or 2, the largest whose table fits; 0: none fits, or no base
MI_HD u32 ksum_window_bits(u32 ns, uint64_t budget) {
    if (!ns) return 0;
    for (u32 c = 8; c >= 2; c >>= 1)
        if (ksum_table_bytes(ns, c) <= budget) return c;
    return 0;
}
// Slices per proof of a batch of n: enough for MI_KSUM_TARGET_LANES lanes over the batch, at most one per term and MI_KSUM_MAX_SLICES.
// One proof alone spreads over min(terms, 1024) lanes; 16384 proofs get 16 slices each, and from 2^18 proofs on a lane is a proof.
MI_HD u32 ksum_slices(u32 ns, u32 c, uint64_t n) {
    const uint64_t terms = (uint64_t)ns * ksum_windows(c), want = n ? (MI_KSUM_TARGET_LANES + n - 1) / n : 1;
    const uint64_t cap = terms < MI_KSUM_MAX_SLICES ? terms : MI_KSUM_MAX_SLICES;
    const uint64_t s = want < cap ? want : cap;
    return s ? (u32)s : 1;
}
// terms of one slice: slice s of S takes the terms [s L, min((s + 1) L, ns windows)), term t = j windows + w
MI_HD uint64_t ksum_slice_terms(u32 ns, u32 c, u32 slices) { return ((uint64_t)ns * ksum_windows(c) + slices - 1) / slices; }
// lanes per proof of the second launch: the power of two at or above `slices`, at most a wave
MI_HD u32 ksum_reduce_lanes(u32 slices) {
    u32 r = 1;
    while (r < slices && r < 64) r <<= 1;
    return r;
}

// word i of a scalar without indexing its registers by a run-time value
MI_HD u32 ksum_word(const Fr &s, u32 i) {
    u32 r = s.l[0];
    for (u32 k = 1; k < 8; k++) r = i == k ? s.l[k] : r;
    return r;
}

// ---- the build.  rows[w] = 2^(c w) base for w < windows: c doublings from one row to the next; an infinite base gives infinite rows
MI_HD void ksum_rows_lane(const G1Aff &base, u32 c, u32 windows, G1X *rows) {
    G1X p = G1X::from_affine(base);
    for (u32 w = 0; w < windows; w++) {
        rows[w] = p;
        for (u32 b = 0; b < c; b++) p = xyzz_dbl(p);
    }
}
// out[d - 1] = d row for 1 <= d <= entries: one addition per entry (the first one is the doubling branch of xyzz_add)
MI_HD void ksum_multiples_lane(const G1X &row, u32 entries, G1X *out) {
    G1X acc = row;
    for (u32 d = 1; d <= entries; d++) {
        out[d - 1] = acc;
        if (d < entries) xyzz_add(acc, row);
    }
}

// ---- the sum.  One slice of one proof: the terms [t0, t1) of its row of ns Montgomery scalars over the table.  A scalar comes out of
// Montgomery form once per lane that meets it; a zero word is stepped over whole and a zero digit costs no lookup, so a byte-valued
// input costs one lookup at c = 8 and two at c = 4.
MI_HD G1X ksum_lane(const G1Aff *table, const Fr *row, u32 c, uint64_t t0, uint64_t t1) {
    const u32 windows = ksum_windows(c), per_word = 32 / c, mask = (1u << c) - 1;
    const uint64_t entries = ksum_row_entries(c);
    G1X acc = G1X::inf();
    u32 j = (u32)(t0 / windows), w = (u32)(t0 - (uint64_t)j * windows);
    for (uint64_t t = t0; t < t1; j++, w = 0) {
        const uint64_t left = t1 - t;
        const u32 wend = left < windows - w ? w + (u32)left : windows;
        const Fr s = fe_from_mont(row[j]);
        const G1Aff *tj = table + (uint64_t)j * windows * entries;
        t += wend - w;
        for (u32 ww = w; ww < wend;) {
            const u32 at = ww * c, word = ksum_word(s, at >> 5);
            if (!word) { ww = ((at >> 5) + 1) * per_word; continue; }
            const u32 d = (word >> (at & 31)) & mask;
            if (d) xyzz_madd(acc, tj[(uint64_t)ww * entries + d - 1], false);
            ww++;
        }
    }
    return acc;
}
// part[first] + part[first + step] + ... below `slices`: what one lane of the second launch starts from
MI_HD G1X ksum_strided_sum(const G1X *part, u32 slices, u32 first, u32 step) {
    G1X acc = G1X::inf();
    for (u32 s = first; s < slices; s += step) xyzz_add(acc, part[s]);
    return acc;
}

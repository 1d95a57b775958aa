// Host build of kSum over a window table (include/mi355x_groth16_verify_ksum.h): the per-lane text of gnark-whir_amd/csrc/ksum_ops.cuh
// -- the window policy, the build of a table, the sum of one slice, the sum of a row's partials -- and verify_assemble_lane of
// pairing_ops.cuh, compiled with -DMI_CHECK_NOWRAP so that every bound of the arithmetic underneath traps.  The loops around the lanes
// are those of csrc/ksum.hip's kernels (the same slices, the same lanes per row, the same tree); the conversions to affine are single
// inversions here where the device batches them: an inverse is unique, so the words are the same.  tests/test_ksum_cpu.py drives it.
#include <cstddef>
#include <cstdint>
#include <vector>
#include "../../gnark-whir_amd/csrc/ksum_ops.cuh"
#include "../../gnark-whir_amd/csrc/pairing_ops.cuh"

extern "C" {
unsigned emu_ksum_window_bits(unsigned ns, uint64_t budget) { return ksum_window_bits(ns, budget); }
unsigned emu_ksum_windows(unsigned c) { return ksum_windows(c); }
uint64_t emu_ksum_table_bytes(unsigned ns, unsigned c) { return ksum_table_bytes(ns, c); }
unsigned emu_ksum_slices(unsigned ns, unsigned c, uint64_t n) { return ksum_slices(ns, c, n); }
uint64_t emu_ksum_slice_terms(unsigned ns, unsigned c, unsigned slices) { return ksum_slice_terms(ns, c, slices); }
unsigned emu_ksum_reduce_lanes(unsigned slices) { return ksum_reduce_lanes(slices); }

// table: ksum_table_bytes(ns, c) bytes (k_ksum_rows, k_ksum_multiples, the conversion)
int emu_ksum_table(const void *k, unsigned ns, unsigned c, void *table) {
    if (c != 8 && c != 4 && c != 2) return -1;
    const u32 windows = ksum_windows(c), entries = (u32)ksum_row_entries(c);
    std::vector<G1X> rows(windows), mult(entries);
    G1Aff *out = (G1Aff *)table;
    for (unsigned j = 0; j < ns; j++) {
        ksum_rows_lane(((const G1Aff *)k)[j], c, windows, rows.data());
        for (u32 w = 0; w < windows; w++) {
            ksum_multiples_lane(rows[w], entries, mult.data());
            for (u32 d = 0; d < entries; d++) out[((size_t)j * windows + w) * entries + d] = xyzz_to_affine(mult[d]);
        }
    }
    return 0;
}
// out: n points (k_ksum_partial, k_ksum_reduce, the conversion); slices == 0: ksum_slices(ns, c, n), else that many (the tests force shapes)
int emu_ksum_batch(const void *table, unsigned ns, unsigned c, const void *scal, const uint8_t *skip, size_t n, unsigned slices, void *out) {
    if (!ns || (c != 8 && c != 4 && c != 2)) return -1;
    const u32 S = slices ? slices : ksum_slices(ns, c, n), R = ksum_reduce_lanes(S);
    const uint64_t terms = (uint64_t)ns * ksum_windows(c), L = ksum_slice_terms(ns, c, S);
    std::vector<G1X> part(S), acc(R);
    for (size_t i = 0; i < n; i++) {
        if (skip && skip[i]) { ((G1Aff *)out)[i] = G1Aff{Fp::zero(), Fp::zero()}; continue; }
        for (u32 s = 0; s < S; s++) {
            const uint64_t t0 = s * L, t1 = t0 + L < terms ? t0 + L : terms;
            part[s] = t0 < terms ? ksum_lane((const G1Aff *)table, (const Fr *)scal + i * ns, c, t0, t1) : G1X::inf();
        }
        for (u32 sub = 0; sub < R; sub++) acc[sub] = ksum_strided_sum(part.data(), S, sub, R);
        for (u32 h = R >> 1; h; h >>= 1)
            for (u32 sub = 0; sub < h; sub++) xyzz_add(acc[sub], acc[sub + h]);
        ((G1Aff *)out)[i] = xyzz_to_affine(acc[0]);
    }
    return 0;
}
// The pairs of n proofs from arrays that lie side by side, as k_verify_assemble reads them; p, q: n x verify_pairs_per_proof(nc) records
int emu_verify_assemble_arrays(const void *k0, const void *gamma2, const void *delta2, const void *ped, unsigned n_pub, unsigned nc, const void *ar,
                               const void *bs, const void *krs, const void *cm, const void *pok, const void *fold, const uint8_t *flags, const void *msm,
                               size_t n, void *p, void *q) {
    if (nc > 16) return -1;
    const VerifyAssembleArrays a{VerifyKeyRef{(const G1Aff *)k0, (const G2Aff *)gamma2, (const G2Aff *)delta2, (const G2Aff *)ped, n_pub, nc},
                                 (const G1Aff *)ar, (const G2Aff *)bs, (const G1Aff *)krs, (const G1Aff *)cm, (const G1Aff *)pok, (const Fr *)fold, flags,
                                 (const G1Aff *)msm};
    for (size_t i = 0; i < n; i++) verify_assemble_lane(a, i, (G1Aff *)p, (G2Aff *)q);
    return 0;
}
}

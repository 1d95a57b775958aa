// Host build of the combined batch verifier (include/mi355x_groth16_verify_combined.h): the coefficient derivation (gnark-whir_amd/csrc/
// combine_coeff.cuh), the 128-bit scaling, the product, the assembly of the tail pairs and the judgement (csrc/pairing_ops.cuh) -- the
// text csrc/verify_combined.hip's kernels and host code run, compiled with -DMI_CHECK_NOWRAP so that every bound of the arithmetic
// underneath traps.  The batch is staged by the library's own VerifyStage (well-formed flags, scalar matrix), the scalar combination is
// the kernels' arithmetic in a plain loop over that matrix, and the MSMs are naive here (the device's run
// through msm.hip).  The host twins of mi_debug_fp12_product_dev / mi_debug_g1_scale128_dev, and of mi_groth16_verify_combined.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../gnark-whir_amd/csrc/pairing_ops.cuh"
#include "../../gnark-whir_amd/csrc/combine_coeff.cuh"

namespace {
G1X mul_mont(const G1Aff &p, const Fr &s) { return xyzz_mul_256(G1X::from_affine(p), fe_from_mont(s).l); }
}

extern "C" {
// out: n x 2 uint64, r_i little-endian
int emu_combine_coefficients(const void *seed, size_t n, void *out) {
    for (size_t i = 0; i < n; i++) {
        u32 k[4];
        combine_coefficient((const uint8_t *)seed, n, i, k);
        std::memcpy((char *)out + 16 * i, k, 16);
    }
    return 0;
}
// the product from the left, one value after the other
int emu_fp12_product(const void *x, size_t n, void *out) {
    if (!n) return -1;
    fp12_product_run((Fp12 *)out, (const Fp12 *)x, n);
    return 0;
}
// k: n x 2 uint64
int emu_g1_scale128(const void *p, const void *k, size_t n, void *out) {
    for (size_t i = 0; i < n; i++) {
        u32 kk[4];
        std::memcpy(kk, (const char *)k + 16 * i, 16);
        ((G1Aff *)out)[i] = g1_scale128(((const G1Aff *)p)[i], kk);
    }
    return 0;
}
// One whole batch the way verify_combined.hip's mi_verify_combined_run judges it.  The key as emu_verify_assemble (emu_pairing.cpp)
// plus alpha1 and beta2; the proofs packed: raw n x (Ar | Bs | Krs), commitments n x nc points, pok n points, public_inputs
// n x (nb_public - 1), commitment_values n x nc, fold_challenge n (null where mi_verify_input allows it for every proof).
// verdict_and_index[0] = the verdict, [1] = first_malformed.  Returns 0, -1 for counts out of range.
int emu_verify_combined(const void *k, const void *alpha1, const void *beta2, const void *gamma2, const void *delta2, const void *ped,
                        unsigned nb_public, unsigned nc, const void *raw, const void *commitments, const void *pok, const void *public_inputs,
                        const void *commitment_values, const void *fold_challenge, size_t n, const void *seed, uint64_t *verdict_and_index) {
    if (nb_public == 0 || nc > 16) return -1;
    const G1Aff *kk = (const G1Aff *)k;
    const unsigned n_pub = nb_public - 1, ns = n_pub + nc, np = verify_combined_tail_pairs(nc);
    const VerifyKeyRef vk{kk, (const G2Aff *)gamma2, (const G2Aff *)delta2, (const G2Aff *)ped, n_pub, nc};
    const size_t raw_len = 2 * sizeof(G1Aff) + sizeof(G2Aff);
    std::vector<VerifyProofRef> refs(n);
    for (size_t i = 0; i < n; i++) {
        const char *r = (const char *)raw + i * raw_len;
        refs[i] = VerifyProofRef{(const G1Aff *)r, (const G2Aff *)(r + sizeof(G1Aff)), (const G1Aff *)(r + sizeof(G1Aff) + sizeof(G2Aff)),
                                 (const G1Aff *)commitments + i * nc, (const G1Aff *)pok + i, (const Fr *)public_inputs + i * n_pub,
                                 (const Fr *)commitment_values + i * nc, fold_challenge ? (const Fr *)fold_challenge + i : nullptr};
    }
    VerifyStage st(vk, refs, nullptr);   // the stage mi_verify_combined_run starts from: the host's flags and the scalar matrix
    // ---- malformed first: Bs of the proofs that passed the host's checks, as k_verify_g2_check answers
    std::vector<uint8_t> off_torsion(n);
    for (size_t i = 0; i < n; i++) off_torsion[i] = !st.flags[i] && !g2_in_subgroup(st.proofs[i].bs);
    st.merge(off_torsion.data());
    verdict_and_index[0] = st.first_flagged < n ? 3 : 0;
    verdict_and_index[1] = st.first_flagged;
    if (!n || st.first_flagged < n) return 0;
    // ---- the coefficients and the scalar combination (k_verify_locate_colsums' arithmetic over the root)
    std::vector<Fr> r(n), col(ns + 1, Fr::zero()), rc((size_t)n * nc);
    std::vector<u32> plain(4 * n);
    for (size_t i = 0; i < n; i++) {
        combine_coefficient((const uint8_t *)seed, n, i, &plain[4 * i]);
        r[i] = fr_from_u128(&plain[4 * i]);
        const VerifyProofRef in = st.proofs[i];
        for (unsigned j = 0; j < ns; j++) col[j] = col[j] + r[i] * st.scal[i * ns + j];
        col[ns] = col[ns] + r[i];
        Fr pw = r[i];
        for (unsigned c = 0; c < nc; c++) { rc[c * n + i] = pw; pw = pw * (nc > 1 ? *in.fold_challenge : Fr::one()); }
    }
    // ---- the MSMs, naively
    G1X mk = G1X::inf(), mkrs = G1X::inf(), mc = G1X::inf(), mpok = G1X::inf();
    std::vector<G1Aff> ck(nc);
    for (unsigned j = 0; j < ns; j++) xyzz_add(mk, mul_mont(kk[1 + j], col[j]));
    for (size_t i = 0; i < n; i++) {
        const VerifyProofRef in = st.proofs[i];
        xyzz_add(mkrs, mul_mont(*in.krs, r[i]));
        if (nc) xyzz_add(mpok, mul_mont(*in.pok, r[i]));
        for (unsigned c = 0; c < nc; c++) xyzz_add(mc, mul_mont(in.commitments[c], r[i]));
    }
    for (unsigned c = 0; c < nc; c++) {
        G1X acc = G1X::inf();
        for (size_t i = 0; i < n; i++) xyzz_add(acc, mul_mont(st.proofs[i].commitments[c], rc[c * n + i]));
        ck[c] = xyzz_to_affine(acc);
    }
    const VerifyCombinedSums sums{col[ns], xyzz_to_affine(mk), xyzz_to_affine(mkrs), xyzz_to_affine(mc), xyzz_to_affine(mpok), ck.data()};
    // ---- the pairs, the Miller loops, the two products, the verdict
    std::vector<G1Aff> P(n + np);
    std::vector<G2Aff> Q(n + np);
    for (size_t i = 0; i < n; i++) { P[i] = g1_scale128(*st.proofs[i].ar, &plain[4 * i]); Q[i] = *st.proofs[i].bs; }
    verify_combined_assemble(vk, *(const G1Aff *)alpha1, *(const G2Aff *)beta2, sums, &P[n], &Q[n]);
    std::vector<Fp12> ml(n + np);
    for (size_t i = 0; i < n + np; i++) pairing_miller_loop(&ml[i], &P[i], &Q[i]);
    Fp12 groth, pd;
    fp12_product_run(&groth, ml.data(), n + MI_VERIFY_GROTH_PAIRS);
    pairing_final_exp(&groth, &groth);
    if (nc) {
        fp12_product_run(&pd, ml.data() + n + MI_VERIFY_GROTH_PAIRS, nc + 1);
        pairing_final_exp(&pd, &pd);
    }
    verdict_and_index[0] = verify_combined_judge(&groth, nc ? &pd : nullptr);
    return 0;
}
}

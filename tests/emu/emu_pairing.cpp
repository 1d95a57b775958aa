// Host build of the tower, the pairing, the verifier's per-proof judgement and the host half of a verification (gnark-whir_amd/csrc/
// fp12.cuh, pairing.cuh, pairing_ops.cuh): the same bodies the device and verify.hip's host code run, compiled with -DMI_CHECK_NOWRAP so that every bound of the arithmetic underneath
// traps.  The host twins of mi_debug_fp12_op_dev / mi_debug_pairing_dev (same op numbers, same layouts).
#include <cstddef>
#include <cstring>
#include "../../gnark-whir_amd/csrc/pairing_ops.cuh"

extern "C" {
int emu_fp12_op(int op, void *z, const void *x, const void *y, size_t n) {
    Fp12 *zz = (Fp12 *)z;
    const Fp12 *xx = (const Fp12 *)x, *yy = (const Fp12 *)y;
    for (size_t i = 0; i < n; i++) {
        Fp12 r = Fp12{Fp6::zero(), Fp6::zero()};
        if (fp12_op(op, &r, &xx[i], yy ? &yy[i] : &xx[i]) != 0) return -1;
        zz[i] = r;
    }
    return 0;
}
// flags bit 0: 0 = the Miller value, 1 = the pairing value f^d'
int emu_pairing(const void *p, const void *q, size_t n, void *gt, unsigned flags) {
    for (size_t i = 0; i < n; i++) {
        Fp12 f;
        pairing_miller_loop(&f, (const G1Aff *)p + i, (const G2Aff *)q + i);
        if (flags & 1) pairing_final_exp(&f, &f);
        ((Fp12 *)gt)[i] = f;
    }
    return 0;
}
// one proof from its 3 + n_ped pairs (the order of pairing_ops.cuh): Miller loops, then verify_judge
int emu_verify_pairs(const void *p, const void *q, unsigned n_ped, const void *e_alpha_beta, int malformed) {
    Fp12 ml[MI_VERIFY_GROTH_PAIRS + 17];
    if (n_ped > 17) return -1;
    for (unsigned i = 0; i < MI_VERIFY_GROTH_PAIRS + n_ped; i++) pairing_miller_loop(&ml[i], (const G1Aff *)p + i, (const G2Aff *)q + i);
    return verify_judge(ml, n_ped, (const Fp12 *)e_alpha_beta, malformed != 0);
}
// One whole proof the way verify.hip's mi_verify_run judges it, host half included: the VerifyStage, the MSM of kSum's scalar part
// done naively here (the device's runs through msm.hip), verify_assemble, the Bs check of k_verify_g2_check, the Miller loops,
// verify_judge.  k: nb_public + nc points; ped: 2 nc twist points (G, GSigmaNeg per commitment); proof: Ar | Bs | Krs; the other
// pointers as mi_verify_input (null where the header allows it).  Returns the verdict, -1 for counts out of range.
int emu_verify_assemble(const void *k, const void *gamma2, const void *delta2, const void *ped, unsigned nb_public, unsigned nc,
                        const void *e_alpha_beta, const void *proof, const void *commitments, const void *pok, const void *public_inputs,
                        const void *commitment_values, const void *fold_challenge) {
    if (nb_public == 0 || nc > 16) return -1;
    const G1Aff *kk = (const G1Aff *)k;
    const unsigned np = verify_pairs_per_proof(nc);
    const VerifyKeyRef vk{kk, (const G2Aff *)gamma2, (const G2Aff *)delta2, (const G2Aff *)ped, nb_public - 1, nc};
    const char *raw = (const char *)proof;
    const VerifyProofRef in{(const G1Aff *)raw, (const G2Aff *)(raw + sizeof(G1Aff)), (const G1Aff *)(raw + sizeof(G1Aff) + sizeof(G2Aff)),
                            (const G1Aff *)commitments, (const G1Aff *)pok, (const Fr *)public_inputs, (const Fr *)commitment_values,
                            (const Fr *)fold_challenge};
    VerifyStage st(vk, {in}, nullptr);   // a batch of one, staged as mi_verify_run stages it: the flag and the row of scalars
    G1X msm = G1X::inf();
    if (!st.flags[0])
        for (unsigned i = 0; i < st.ns; i++) xyzz_add(msm, xyzz_mul_256(G1X::from_affine(kk[1 + i]), fe_from_mont(st.scal[i]).l));
    G1Aff p[MI_VERIFY_GROTH_PAIRS + 17];
    G2Aff q[MI_VERIFY_GROTH_PAIRS + 17];
    verify_assemble(vk, in, !st.flags[0], xyzz_to_affine(msm), p, q);
    const uint8_t off_torsion = !g2_in_subgroup(&q[0]);
    st.merge(&off_torsion);
    Fp12 ml[MI_VERIFY_GROTH_PAIRS + 17];
    for (unsigned i = 0; i < np; i++) pairing_miller_loop(&ml[i], &p[i], &q[i]);
    return verify_judge(ml, np - MI_VERIFY_GROTH_PAIRS, (const Fp12 *)e_alpha_beta, st.flags[0] != 0);
}
int emu_g1_reduced(const void *p) { return g1_reduced(*(const G1Aff *)p) ? 1 : 0; }
int emu_g2_reduced(const void *q) { return g2_reduced(*(const G2Aff *)q) ? 1 : 0; }
int emu_g1_on_curve(const void *p) { return g1_on_curve(*(const G1Aff *)p) ? 1 : 0; }
int emu_g2_on_twist(const void *q) { return g2_on_twist(*(const G2Aff *)q) ? 1 : 0; }
int emu_g2_in_subgroup(const void *q) { return g2_in_subgroup((const G2Aff *)q) ? 1 : 0; }
}

// Host build of the tower, the pairing and the verifier's per-proof judgement (gnark-whir_amd/csrc/fp12.cuh, pairing.cuh,
// pairing_ops.cuh): the same bodies the device runs, compiled with -DMI_CHECK_NOWRAP so that every bound of the arithmetic underneath
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
int emu_g1_on_curve(const void *p) { return g1_on_curve(*(const G1Aff *)p) ? 1 : 0; }
int emu_g2_on_twist(const void *q) { return g2_on_twist(*(const G2Aff *)q) ? 1 : 0; }
int emu_g2_in_subgroup(const void *q) { return g2_in_subgroup((const G2Aff *)q) ? 1 : 0; }
}

// Host build of the wave-per-pairing text (gnark-whir_amd/csrc/fp12_wave.cuh, pairing_wave.cuh): the phases csrc/verify_wave.hip runs
// on the 64 lanes of a workgroup, here as a loop over lane = 0 .. 63 (MI_WAVE_PHASE), compiled with -DMI_CHECK_NOWRAP so that every
// bound of the arithmetic underneath traps.  The host twins of mi_debug_fp12_op_wave_dev / mi_debug_pairing_wave_dev and of
// mi_verify_run_wave's device half; tests/test_pairing_wave_cpu.py compares them word for word with tests/emu/emu_pairing.cpp.
// Every image is allocated at exactly MI_WAVE_IMAGE_RECORDS records.
#include <cstddef>
#include <cstring>
#include <vector>
#include "../../gnark-whir_amd/csrc/pairing_wave.cuh"

extern "C" {
unsigned emu_wave_image_bytes() { return MI_WAVE_IMAGE_BYTES; }
// z[i] = op(x[i], y[i]) by the slots mi_debug_fp12_op_wave_dev uses (S0 <- op(S1, S2)).  alias: 0 = as the device entry point runs it;
// 1 / 2 = the operation itself with its output slot aliasing its first / second input slot (the ops with one call of fp12_wave.cuh)
int emu_wave_fp12_op(int op, void *z, const void *x, const void *y, size_t n, int alias) {
    std::vector<Fp2> im(MI_WAVE_IMAGE_RECORDS);
    for (size_t i = 0; i < n; i++) {
        const Fp12 *xx = (const Fp12 *)x + i, *yy = y ? (const Fp12 *)y + i : xx;
        MI_WAVE_PHASE(w12_ph_load(lane, im.data(), MI_WAVE_S(1), xx));
        MI_WAVE_PHASE(w12_ph_load(lane, im.data(), MI_WAVE_S(2), yy));
        MI_WAVE_PHASE(if (lane < 6) im[MI_WAVE_S(0) + lane] = Fp2::zero());
        u32 out = MI_WAVE_S(0);
        if (alias) {
            const u32 a = MI_WAVE_S(1), b = MI_WAVE_S(2);
            out = alias == 1 ? a : b;
            switch (op) {
            case F12_MUL: w12_mul(im.data(), out, a, b); break;
            case F12_SQR: w12_mul(im.data(), a, a, a); out = a; break;
            case F12_INV: w12_inv(im.data(), a, a); out = a; break;
            case F12_FROB1: case F12_FROB2: case F12_FROB3: w12_frob(im.data(), (u32)(op - F12_FROB1 + 1), a, a); out = a; break;
            case F12_CYCLO_SQR: w12_cyclo_sqr(im.data(), a, a); out = a; break;
            case F12_CONJ: w12_conj(im.data(), a, a); out = a; break;
            case F12_EASY: wave_easy_part(im.data(), a, a, MI_WAVE_S(3), MI_WAVE_S(4)); out = a; break;
            case F12_MUL_LINE: w12_mul_line(im.data(), out, a, b, b + 3, b + 4); break;
            case F12_ADD: MI_WAVE_PHASE(w12_ph_add(lane, im.data(), out, a, b, false)); break;
            case F12_SUB: MI_WAVE_PHASE(w12_ph_add(lane, im.data(), out, a, b, true)); break;
            default: return -2;   // no aliased form
            }
        } else if (wave_fp12_op(im.data(), op) != 0) {
            return -1;
        }
        MI_WAVE_PHASE(w12_ph_store(lane, im.data(), (Fp12 *)z + i, out));
    }
    return 0;
}
// flags bit 0: 0 = the Miller value, 1 = the pairing value f^d'
int emu_wave_pairing(const void *p, const void *q, size_t n, void *gt, unsigned flags) {
    std::vector<Fp2> im(MI_WAVE_IMAGE_RECORDS);
    for (size_t i = 0; i < n; i++) {
        wave_miller_loop(im.data(), (const G1Aff *)p + i, (const G2Aff *)q + i);
        if (flags & 1) wave_final_exp(im.data());
        MI_WAVE_PHASE(w12_ph_store(lane, im.data(), (Fp12 *)gt + i, MI_WAVE_S(0)));
    }
    return 0;
}
// The device half of mi_verify_run_wave for one proof, from its 3 + n_ped pairs: the Bs check, one Miller loop per pair, one judgement
// per equation, the verdict byte.  malformed: the host half's flag.
int emu_wave_verify_pairs(const void *p, const void *q, unsigned n_ped, const void *e_alpha_beta, int malformed) {
    if (n_ped > 17) return -1;
    const u32 np = MI_VERIFY_GROTH_PAIRS + n_ped, n_eq = wave_equations(np);
    std::vector<Fp2> im(MI_WAVE_IMAGE_RECORDS);
    std::vector<Fp12> ml(np);
    const bool flag = malformed != 0 || !wave_bs_in_subgroup(*(const G2Aff *)q);
    for (u32 i = 0; i < np; i++) {
        wave_miller_loop(im.data(), (const G1Aff *)p + i, (const G2Aff *)q + i);
        MI_WAVE_PHASE(w12_ph_store(lane, im.data(), &ml[i], MI_WAVE_S(0)));
    }
    const Fp12 one = Fp12::one();
    uint8_t pass[2] = {0, 0};
    for (u32 eq = 0; eq < n_eq; eq++)
        wave_judge_equation(im.data(), &ml[wave_equation_first(eq)], wave_equation_count(eq, np), eq ? &one : (const Fp12 *)e_alpha_beta, &pass[eq]);
    return wave_verdict(flag, pass, n_eq);
}
// One whole proof the way mi_verify_run_wave judges it, host half included: emu_verify_assemble of tests/emu/emu_pairing.cpp with the
// wave device half.  A proof the host half flags gets pairs of infinities, as on the device.
int emu_wave_verify_assemble(const void *k, const void *gamma2, const void *delta2, const void *ped, unsigned nb_public, unsigned nc,
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
    VerifyStage st(vk, {in}, nullptr);
    G1X msm = G1X::inf();
    if (!st.flags[0])
        for (unsigned i = 0; i < st.ns; i++) xyzz_add(msm, xyzz_mul_256(G1X::from_affine(kk[1 + i]), fe_from_mont(st.scal[i]).l));
    G1Aff p[MI_VERIFY_GROTH_PAIRS + 17];
    G2Aff q[MI_VERIFY_GROTH_PAIRS + 17];
    verify_assemble(vk, in, !st.flags[0], xyzz_to_affine(msm), p, q);
    return emu_wave_verify_pairs(p, q, np - MI_VERIFY_GROTH_PAIRS, e_alpha_beta, st.flags[0] != 0);
}
int emu_wave_bs_in_subgroup(const void *q) { return wave_bs_in_subgroup(*(const G2Aff *)q) ? 1 : 0; }
}

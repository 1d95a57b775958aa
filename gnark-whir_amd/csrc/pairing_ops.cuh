// What the verifier's kernels (verify.hip) and the host build of the tests (tests/emu/emu_pairing.cpp, overflow traps on) both run, one
// record per lane / per call: the Fp12 operations of mi_debug_fp12_op_dev, and the judgement of one proof from its Miller values.
#pragma once
#include "pairing.cuh"

// op numbers of mi_debug_fp12_op_dev (mirrored in include/mi355x_groth16_debug.h); x, y, z are Fp12 records of 12 x mi_fp
enum {
    F12_MUL = 0,         // x y
    F12_SQR = 1,         // x^2
    F12_INV = 2,         // 1 / x (0 -> 0)
    F12_FROB1 = 3,       // x^p
    F12_FROB2 = 4,       // x^(p^2)
    F12_FROB3 = 5,       // x^(p^3)
    F12_CYCLO_SQR = 6,   // x^2 by the cyclotomic formula: equals F12_SQR in the cyclotomic subgroup only
    F12_CONJ = 7,        // x^(p^6)
    F12_EASY = 8,        // x^((p^6 - 1)(p^2 + 1))
    F12_FINAL_EXP = 9,   // x^d' (pairing.cuh)
    F12_MUL_LINE = 10,   // x (l0 + l3 w + l4 v w) by the sparse product; l0 = y.C0.B0, l3 = y.C1.B0, l4 = y.C1.B1, the rest of y is not read
    F12_ADD = 11,
    F12_SUB = 12,
    F12_FP6_MUL = 13,    // the Fp6 layer alone, on the C0 halves: z.C0 = x.C0 y.C0, z.C1 = x.C1 y.C1
    F12_FP6_SQR = 14,    // z.C0 = x.C0^2, z.C1 = x.C1^2
    F12_FP6_INV = 15,    // z.C0 = 1 / x.C0, z.C1 = 1 / x.C1
    F12_OP_END = 16
};

// returns -1 for an op it does not handle
MI_HD int fp12_op(int op, Fp12 *z, const Fp12 *x, const Fp12 *y) {
    switch (op) {
    case F12_MUL: fp12_mul(z, x, y); break;
    case F12_SQR: fp12_sqr(z, x); break;
    case F12_INV: fp12_inv(z, x); break;
    case F12_FROB1: fp12_frob1(z, x); break;
    case F12_FROB2: fp12_frob2(z, x); break;
    case F12_FROB3: fp12_frob3(z, x); break;
    case F12_CYCLO_SQR: fp12_cyclo_sqr(z, x); break;
    case F12_CONJ: fp12_conj(z, x); break;
    case F12_EASY: pairing_easy_part(z, x); break;
    case F12_FINAL_EXP: pairing_final_exp(z, x); break;
    case F12_MUL_LINE: fp12_mul_by_line(z, x, &y->c0.b0, &y->c1.b0, &y->c1.b1); break;
    case F12_ADD: fp12_add(z, x, y); break;
    case F12_SUB: fp12_sub(z, x, y); break;
    case F12_FP6_MUL: fp6_mul(&z->c0, &x->c0, &y->c0); fp6_mul(&z->c1, &x->c1, &y->c1); break;
    case F12_FP6_SQR: fp6_sqr(&z->c0, &x->c0); fp6_sqr(&z->c1, &x->c1); break;
    case F12_FP6_INV: fp6_inv(&z->c0, &x->c0); fp6_inv(&z->c1, &x->c1); break;
    default: return -1;
    }
    return 0;
}

// The pairs of one proof, in the order the host lays them out (verify.hip):
//     0: (Ar, Bs)   1: (-kSum, gamma)   2: (-Krs, delta)   then, with n_commitments > 0:   3: (pok, G)   4 + k: (c^k C_k, GSigmaNeg_k)
// and its verdict from their Miller values ml[0 .. 3 + n_ped): MI_VERIFY_MALFORMED (3) first, then the Groth16 equation
// prod ml[0..3)^d' == e(alpha, beta)^s (1 when it fails), then the Pedersen one prod ml[3..)^d' == 1 (2), else 0.  n_ped = 0 or
// n_commitments + 1; it is the same for every proof of a key, so a wave does not diverge here.
#define MI_VERIFY_GROTH_PAIRS 3
MI_OOL uint8_t verify_judge(const Fp12 *ml, u32 n_ped, const Fp12 *e_alpha_beta, bool malformed) {
    Fp12 f;
    fp12_mul(&f, &ml[0], &ml[1]);
    fp12_mul(&f, &f, &ml[2]);
    pairing_final_exp(&f, &f);
    uint8_t verdict = f == *e_alpha_beta ? 0 : 1;
    if (n_ped) {
        f = ml[MI_VERIFY_GROTH_PAIRS];
        for (u32 k = 1; k < n_ped; k++) fp12_mul(&f, &f, &ml[MI_VERIFY_GROTH_PAIRS + k]);
        pairing_final_exp(&f, &f);
        if (verdict == 0 && !(f == Fp12::one())) verdict = 2;
    }
    return malformed ? 3 : verdict;
}

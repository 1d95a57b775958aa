// The pairing of pairing.cuh and the verifier's judgement of pairing_ops.cuh with one wave per pairing, in the phases of fp12_wave.cuh:
// the same loop over 6 x0 + 2, the same two correction lines, the same chain for d', and the point steps by the formulas of
// miller_double / miller_add, so that (c0, c1, c2) of every line and hence the Miller value are the same field elements -- and, every Fp
// result being fully reduced, the same words.  csrc/verify_wave.hip runs this text on the device, tests/emu/emu_pairing_wave.cpp on the
// host (-DMI_CHECK_NOWRAP); both compare it bit for bit with the one-lane bodies.
//
// A point step spreads its Fp2 products over lanes in dependency levels, one phase per level:
//   doubling   {xy, y^2, z^2, (y+z)^2, x^2}   {e = twist_b 3c, a = xy / 2, h, l3}   {a (b - f), g^2, e^2, b h, l0, l4}   {y' = g^2 - 3 e^2}
//   addition   {theta, lambda}   {theta^2, lambda^2, theta qx, lambda qy, l0, l3}   {e, f, g, l4}   {lambda h, theta (g - h), e y, z e}   {y'}
// The line leaves a step already evaluated at P (l0 = c0 yP, l3 = c1 xP, l4 = c2), ready for w12_mul_line.  T's levels do not depend
// on f; they run between f's products here, not beside them: the lanes of one wave that take different branches run one after the other,
// so sharing a phase would save barriers and no arithmetic.
#pragma once
#include "fp12_wave.cuh"
#include "pairing_ops.cuh"
#include "keyfile_ops.cuh"   // g2_in_subgroup_psi

// the Miller loop's records (fp12_wave.cuh: MI_WAVE_MILLER .. MI_WAVE_IMAGE_RECORDS)
enum {
    WM_TX = MI_WAVE_MILLER, WM_TY, WM_TZ,     // T, homogeneous projective on the twist
    WM_QX, WM_QY, WM_Q1X, WM_Q1Y, WM_Q2X, WM_Q2Y,   // Q, pi(Q), -pi^2(Q)
    WM_P,                                     // (xP, yP) as the two halves of one record
    WM_L0, WM_L3, WM_L4,                      // the line in flight, evaluated at P
    WM_D,                                     // 11 temporaries of a point step
    WM_END = WM_D + 11
};
static_assert(WM_END == MI_WAVE_IMAGE_RECORDS, "the image ends with the Miller loop's records");

// ---------------------------------------------------------------- phases of the Miller loop
// f = 1, T = Q, the three fixed points and P: one record per lane
MI_HD void wm_ph_init(u32 lane, Fp2 *im, const G1Aff *p, const G2Aff *q) {
    if (lane < 6) { w12_ph_set_one(lane, im, MI_WAVE_S(0)); return; }
    switch (lane) {
    case 6: im[WM_TX] = q->x; break;
    case 7: im[WM_TY] = q->y; break;
    case 8: im[WM_TZ] = Fp2::one(); break;
    case 9: im[WM_QX] = q->x; break;
    case 10: im[WM_QY] = q->y; break;
    case 11: im[WM_Q1X] = fp2_conj(q->x) * fp12c_frob1_2(); break;
    case 12: im[WM_Q1Y] = fp2_conj(q->y) * fp12c_frob1_3(); break;
    case 13: im[WM_Q2X] = fp2_mul_fp(q->x, fp12c_frob2_2().a0); break;
    case 14: im[WM_Q2Y] = fe_neg(fp2_mul_fp(q->y, fp12c_frob2_3().a0)); break;
    case 15: im[WM_P] = Fp2{p->x, p->y}; break;
    default: break;
    }
}
// doubling, level 1: D0 = x y, D1 = y^2, D2 = z^2, D3 = (y + z)^2, D4 = x^2 -- five lanes, one product text
MI_HD void wm_ph_dbl_1(u32 lane, Fp2 *im) {
    if (lane >= 5) return;
    Fp2 u = im[lane == 0 || lane == 4 ? WM_TX : lane == 2 ? WM_TZ : WM_TY];
    Fp2 v = im[lane == 0 || lane == 1 ? WM_TY : lane == 4 ? WM_TX : WM_TZ];
    if (lane == 3) { u = u + v; v = u; }
    im[WM_D + lane] = u * v;
}
// level 2: D5 = e = twist_b 3 c, D6 = a = x y / 2, D7 = h = (y + z)^2 - (b + c), l3 = 3 x^2 xP
MI_HD void wm_ph_dbl_2(u32 lane, Fp2 *im) {
    if (lane >= 4) return;
    if (lane == 0) { im[WM_D + 5] = fp12c_twist_b() * fp2_triple(im[WM_D + 2]); return; }
    if (lane == 2) { im[WM_D + 7] = im[WM_D + 3] - (im[WM_D + 1] + im[WM_D + 2]); return; }
    const Fp2 s = lane == 1 ? im[WM_D] : fp2_triple(im[WM_D + 4]);
    const Fp k = lane == 1 ? fp12c_half() : im[WM_P].a0;
    im[lane == 1 ? WM_D + 6 : WM_L3] = fp2_mul_fp(s, k);
}
// level 3: x' = a (b - f), D9 = g^2, D8 = e^2, z' = b h (f = 3 e, g = (b + f) / 2), l0 = -h yP, l4 = e - b
MI_HD void wm_ph_dbl_3(u32 lane, Fp2 *im) {
    if (lane >= 6) return;
    const Fp2 b = im[WM_D + 1], e = im[WM_D + 5];
    if (lane == 5) { im[WM_L4] = e - b; return; }
    const Fp2 f = fp2_triple(e);
    Fp2 w = Fp2::zero();
    if (lane == 1 || lane == 4) w = fp2_mul_fp(lane == 1 ? b + f : fe_neg(im[WM_D + 7]), lane == 1 ? fp12c_half() : im[WM_P].a1);
    if (lane == 4) { im[WM_L0] = w; return; }
    const Fp2 u = lane == 0 ? im[WM_D + 6] : lane == 1 ? w : lane == 2 ? e : b;
    const Fp2 v = lane == 0 ? b - f : lane == 1 ? w : lane == 2 ? e : im[WM_D + 7];
    im[lane == 0 ? WM_TX : lane == 1 ? WM_D + 9 : lane == 2 ? WM_D + 8 : WM_TZ] = u * v;
}
MI_HD void wm_ph_dbl_4(u32 lane, Fp2 *im) {
    if (lane == 0) im[WM_TY] = im[WM_D + 9] - fp2_triple(im[WM_D + 8]);
}
// addition of the point at records (qx, qx + 1), level 1: D0 = theta = y - qy z, D1 = lambda = x - qx z
MI_HD void wm_ph_add_1(u32 lane, Fp2 *im, u32 qx) {
    if (lane >= 2) return;
    im[WM_D + lane] = im[lane ? WM_TX : WM_TY] - im[lane ? qx : qx + 1] * im[WM_TZ];
}
// level 2: D2 = c = theta^2, D3 = d = lambda^2, D4 = theta qx, D5 = lambda qy, l0 = lambda yP, l3 = -theta xP
MI_HD void wm_ph_add_2(u32 lane, Fp2 *im, u32 qx) {
    if (lane >= 6) return;
    const Fp2 th = im[WM_D], la = im[WM_D + 1];
    if (lane >= 4) {
        im[lane == 4 ? WM_L0 : WM_L3] = fp2_mul_fp(lane == 4 ? la : fe_neg(th), lane == 4 ? im[WM_P].a1 : im[WM_P].a0);
        return;
    }
    const Fp2 u = (lane & 1) ? la : th;
    const Fp2 v = lane == 0 ? th : lane == 1 ? la : lane == 2 ? im[qx] : im[qx + 1];
    im[WM_D + 2 + lane] = u * v;
}
// level 3: D6 = e = lambda d, D7 = f = z c, D8 = g = x d, l4 = theta qx - lambda qy
MI_HD void wm_ph_add_3(u32 lane, Fp2 *im) {
    if (lane >= 4) return;
    if (lane == 3) { im[WM_L4] = im[WM_D + 4] - im[WM_D + 5]; return; }
    const Fp2 u = im[lane == 0 ? WM_D + 1 : lane == 1 ? WM_TZ : WM_TX];
    const Fp2 v = im[lane == 1 ? WM_D + 2 : WM_D + 3];
    im[WM_D + 6 + lane] = u * v;
}
// level 4, h = e + f - 2 g: x' = lambda h, D9 = theta (g - h), D10 = e y, z' = z e
MI_HD void wm_ph_add_4(u32 lane, Fp2 *im) {
    if (lane >= 4) return;
    const Fp2 e = im[WM_D + 6], g = im[WM_D + 8];
    const Fp2 h = e + im[WM_D + 7] - fe_dbl(g);
    const Fp2 u = lane == 0 ? im[WM_D + 1] : lane == 1 ? im[WM_D] : e;
    const Fp2 v = lane == 0 ? h : lane == 1 ? g - h : lane == 2 ? im[WM_TY] : im[WM_TZ];
    im[lane == 0 ? WM_TX : lane == 1 ? WM_D + 9 : lane == 2 ? WM_D + 10 : WM_TZ] = u * v;
}
MI_HD void wm_ph_add_5(u32 lane, Fp2 *im) {
    if (lane == 0) im[WM_TY] = im[WM_D + 9] - im[WM_D + 10];
}

// ---------------------------------------------------------------- the Miller loop: S0 <- the Miller value of (*p, *q)
// T <- 2 T, f <- f l
MI_OOL void wm_double_step(Fp2 *im) {
    MI_WAVE_PHASE(wm_ph_dbl_1(lane, im));
    MI_WAVE_PHASE(wm_ph_dbl_2(lane, im));
    MI_WAVE_PHASE(wm_ph_dbl_3(lane, im));
    MI_WAVE_PHASE(wm_ph_dbl_4(lane, im));
    w12_mul_line(im, MI_WAVE_S(0), MI_WAVE_S(0), WM_L0, WM_L3, WM_L4);
}
// T <- T + the point at qx, f <- f l
MI_OOL void wm_add_step(Fp2 *im, u32 qx) {
    MI_WAVE_PHASE(wm_ph_add_1(lane, im, qx));
    MI_WAVE_PHASE(wm_ph_add_2(lane, im, qx));
    MI_WAVE_PHASE(wm_ph_add_3(lane, im));
    MI_WAVE_PHASE(wm_ph_add_4(lane, im));
    MI_WAVE_PHASE(wm_ph_add_5(lane, im));
    w12_mul_line(im, MI_WAVE_S(0), MI_WAVE_S(0), WM_L0, WM_L3, WM_L4);
}
// *p and *q are read by every lane, from the same addresses: P or Q at infinity is decided once for the wave
MI_OOL void wave_miller_loop(Fp2 *im, const G1Aff *p, const G2Aff *q) {
    if (p->is_inf() || q->is_inf()) {
        MI_WAVE_PHASE(w12_ph_set_one(lane, im, MI_WAVE_S(0)));
        return;
    }
    MI_WAVE_PHASE(wm_ph_init(lane, im, p, q));
    for (int i = 63; i >= 0; i--) {   // bit 64 is the leading one
        w12_mul(im, MI_WAVE_S(0), MI_WAVE_S(0), MI_WAVE_S(0));
        wm_double_step(im);
        if ((MI_BN_ATE_LOW64 >> i) & 1) wm_add_step(im, WM_QX);
    }
    wm_add_step(im, WM_Q1X);
    wm_add_step(im, WM_Q2X);
}

// ---------------------------------------------------------------- the final exponentiation: pairing_final_exp's sequence over slots
// z <- x^x0 in the cyclotomic subgroup; z and x are different slots
MI_OOL void wave_exp_x0(Fp2 *im, u32 z, u32 x) {
    w12_copy(im, z, x);
    for (int i = 61; i >= 0; i--) {
        w12_cyclo_sqr(im, z, z);
        if ((MI_BN_X0 >> i) & 1) w12_mul(im, z, z, x);
    }
}
// z <- f^((p^6 - 1)(p^2 + 1)); t and u are two slots to work in (z may be f)
MI_OOL void wave_easy_part(Fp2 *im, u32 z, u32 f, u32 t, u32 u) {
    w12_inv(im, t, f);
    w12_conj(im, u, f);
    w12_mul(im, t, u, t);
    w12_frob(im, 2, u, t);
    w12_mul(im, z, u, t);
}
// S0 <- S0^d'
MI_OOL void wave_final_exp(Fp2 *im) {
    const u32 f = MI_WAVE_S(0), m = MI_WAVE_S(1), t0 = MI_WAVE_S(2), t1 = MI_WAVE_S(3), t2 = MI_WAVE_S(4), t3 = MI_WAVE_S(5), t4 = MI_WAVE_S(6);
    wave_easy_part(im, m, f, t0, t1);
    wave_exp_x0(im, t0, m);
    w12_conj(im, t0, t0);
    w12_cyclo_sqr(im, t0, t0);            // m^(-2 x0)
    w12_cyclo_sqr(im, t1, t0);
    w12_mul(im, t1, t0, t1);              // m^(-6 x0)
    wave_exp_x0(im, t2, t1);
    w12_conj(im, t2, t2);                 // m^(6 x0^2)
    w12_conj(im, t3, t1);
    w12_mul(im, t1, t2, t3);
    w12_cyclo_sqr(im, t3, t2);
    wave_exp_x0(im, t4, t3);              // m^(12 x0^3)
    w12_mul(im, t4, t1, t4);
    w12_mul(im, t3, t0, t4);
    w12_mul(im, t0, t2, t4);
    w12_mul(im, t0, m, t0);
    w12_frob(im, 1, t2, t3);
    w12_mul(im, t0, t2, t0);
    w12_frob(im, 2, t2, t4);
    w12_mul(im, t0, t2, t0);
    w12_conj(im, t2, m);
    w12_mul(im, t2, t2, t3);
    w12_frob(im, 3, t2, t2);
    w12_mul(im, f, t2, t0);
}

// ---------------------------------------------------------------- fp12_op's numbers (pairing_ops.cuh) over slots: S0 <- op(S1, S2).
// Inversion and the Fp6 layer are one lane's call of fp12.cuh: the inversion runs once per final exponentiation, and nothing here calls
// the Fp6 layer.  Returns -1 for an op it does not handle (the same in every lane).
MI_OOL int wave_fp12_op(Fp2 *im, int op) {
    const u32 z = MI_WAVE_S(0), x = MI_WAVE_S(1), y = MI_WAVE_S(2);
    switch (op) {
    case F12_MUL: w12_mul(im, z, x, y); break;
    case F12_SQR: w12_mul(im, z, x, x); break;
    case F12_INV: w12_inv(im, z, x); break;
    case F12_FROB1: w12_frob(im, 1, z, x); break;
    case F12_FROB2: w12_frob(im, 2, z, x); break;
    case F12_FROB3: w12_frob(im, 3, z, x); break;
    case F12_CYCLO_SQR: w12_cyclo_sqr(im, z, x); break;
    case F12_CONJ: w12_conj(im, z, x); break;
    case F12_EASY: wave_easy_part(im, z, x, MI_WAVE_S(3), MI_WAVE_S(4)); break;
    case F12_FINAL_EXP: w12_copy(im, z, x); wave_final_exp(im); break;
    case F12_MUL_LINE: w12_mul_line(im, z, x, y, y + 3, y + 4); break;
    case F12_ADD: MI_WAVE_PHASE(w12_ph_add(lane, im, z, x, y, false)); break;
    case F12_SUB: MI_WAVE_PHASE(w12_ph_add(lane, im, z, x, y, true)); break;
    case F12_FP6_MUL:
    case F12_FP6_SQR:
    case F12_FP6_INV:
        MI_WAVE_PHASE(if (lane == 0) {
            const Fp12 a = w12_get(im, x), b = w12_get(im, y);
            Fp12 r = Fp12{Fp6::zero(), Fp6::zero()};
            (void)fp12_op(op, &r, &a, &b);
            w12_put(im, z, r);
        });
        break;
    default: return -1;
    }
    return 0;
}

// ---------------------------------------------------------------- the judgement (verify_judge of pairing_ops.cuh), one wave per
// (proof, equation): S0 <- ml[0] ... ml[cnt - 1], cnt >= 1, its final exponentiation, and *pass = it equals *target (lane 0 writes)
MI_OOL void wave_judge_equation(Fp2 *im, const Fp12 *ml, u32 cnt, const Fp12 *target, uint8_t *pass) {
    MI_WAVE_PHASE(w12_ph_load(lane, im, MI_WAVE_S(0), ml));
    for (u32 k = 1; k < cnt; k++) {
        MI_WAVE_PHASE(w12_ph_load(lane, im, MI_WAVE_S(1), ml + k));
        w12_mul(im, MI_WAVE_S(0), MI_WAVE_S(0), MI_WAVE_S(1));
    }
    wave_final_exp(im);
    MI_WAVE_PHASE(if (lane == 0) *pass = w12_equals(im, MI_WAVE_S(0), *target) ? 1 : 0);
}
// equation eq of a proof with pairs_per_proof Miller values: which of them, and what their product must equal
MI_HD u32 wave_equation_first(u32 eq) { return eq ? MI_VERIFY_GROTH_PAIRS : 0; }
MI_HD u32 wave_equation_count(u32 eq, u32 pairs_per_proof) { return eq ? pairs_per_proof - MI_VERIFY_GROTH_PAIRS : MI_VERIFY_GROTH_PAIRS; }
MI_HD u32 wave_equations(u32 pairs_per_proof) { return pairs_per_proof > MI_VERIFY_GROTH_PAIRS ? 2 : 1; }
// the verdict byte with verify_judge's precedence: malformed (3) over the Groth16 equation (1) over the Pedersen one (2)
MI_HD uint8_t wave_verdict(bool malformed, const uint8_t *pass, u32 n_eq) {
    if (malformed) return 3;
    if (!pass[0]) return 1;
    return n_eq > 1 && !pass[1] ? 2 : 0;
}
// Bs belongs to the r-torsion of the twist: on the twist, then the 63-bit endomorphism test the key loaders use (keyfile_ops.cuh) --
// the answer of g2_in_subgroup at a quarter of its doublings.  One lane's work; coordinates below p (the host has seen to that)
MI_HD bool wave_bs_in_subgroup(const G2Aff &bs) { return g2_on_twist(bs) && g2_in_subgroup_psi(&bs); }

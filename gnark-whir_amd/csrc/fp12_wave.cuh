// The Fp12 of fp12.cuh with ONE WAVE per value: the 36 (or 18, or 9) Fp2 products of an operation on 36 lanes at once, where fp12.cuh
// runs a chain of 54 Fp products in one lane.  Latency is what this buys (csrc/verify_wave.hip: one proof); lanes are free.
//
// The view.  The tower is Fp2[w]/(w^6 - xi): coefficient C_i.B_j of fp12.cuh belongs to w^e, e = i + 2 j, so a product is
//     z_k = sum_{i+j=k} x_i y_j + xi sum_{i+j=k+6} x_i y_j                                    (k = 0 .. 5)
// -- 36 independent Fp2 products, then six sums of six terms.  No Karatsuba, no pre-additions.  Every Fp result of field.cuh is fully
// reduced, so this order of evaluation gives the very words fp12_mul gives: the tests compare bit for bit.
//
// The contract.  Values live in an IMAGE: an array of MI_WAVE_IMAGE_RECORDS Fp2 records (64 B each; LDS on the device, any memory on
// the host).  An Fp12 is six consecutive records in the tower order of fp12.cuh (record 3 i + j = C_i.B_j), named by its first record.
// Every operation is a short sequence of PHASES.  A phase is an MI_HD function phase(lane, im, ...): the lane reads the records its
// lane number selects -- as ADDRESSES into the image, never as a register array indexed at run time --, does at most one Fp2 product
// (beside additions and at most one product by an element of Fp), and writes at most one record and one line coefficient.  Within a
// phase no record is written by one lane and read by another, so the lanes of a phase may run in any order: the device runs them as
// the 64 lanes of a single-wave workgroup with __syncthreads() behind every phase, the host build of the tests (tests/emu/
// emu_pairing_wave.cpp) as a loop over lane = 0 .. 63.  MI_WAVE_PHASE is that difference and nothing else; the text is the same.
// On the device every lane of the workgroup must reach every phase: what decides the control flow around a phase is the same in all
// 64 lanes (arguments, constants, values every lane read from the same address).
// Outputs may alias inputs: a product reads its operands in one phase and writes its result in the next.
#pragma once
#include "fp12.cuh"

#define MI_WAVE_LANES 64
// the image: seven Fp12 slots (S0 is the value an operation chain works on, S1 .. S6 are the temporaries of the final exponentiation),
// the products of the operation in flight, then what pairing_wave.cuh keeps of a Miller loop
#define MI_WAVE_S(i) (6u * (i))
#define MI_WAVE_T 42u                  // 36 records
#define MI_WAVE_MILLER 78u             // pairing_wave.cuh: 24 records
#define MI_WAVE_IMAGE_RECORDS 102u
#define MI_WAVE_IMAGE_BYTES (MI_WAVE_IMAGE_RECORDS * 64u)
static_assert(sizeof(Fp2) == 64, "a record is one Fp2");

#if defined(__HIP_DEVICE_COMPILE__)
#define MI_WAVE_PHASE(...) do { const u32 lane = threadIdx.x; __VA_ARGS__; __syncthreads(); } while (0)
#else
#define MI_WAVE_PHASE(...) do { for (u32 lane = 0; lane < MI_WAVE_LANES; lane++) { __VA_ARGS__; } } while (0)
#endif

// the record of the coefficient of w^e inside an Fp12, and the power of w of record k
MI_HD u32 w12_rec(u32 e) { return (e & 1u) * 3u + (e >> 1); }
MI_HD u32 w12_pow(u32 k) { return k >= 3 ? 2 * (k - 3) + 1 : 2 * k; }

// ---------------------------------------------------------------- phases
// lane 6 i + j: T[6 i + j] = x_i y_j (coefficients by their power of w)
MI_HD void w12_ph_mul_products(u32 lane, Fp2 *im, u32 x, u32 y) {
    if (lane >= 36) return;
    const u32 i = lane / 6, j = lane - 6 * i;
    im[MI_WAVE_T + lane] = im[x + w12_rec(i)] * im[y + w12_rec(j)];
}
// lane k: z_k = sum_{i <= k} T[i][k - i] + xi sum_{i > k} T[i][k + 6 - i]
MI_HD void w12_ph_mul_sums(u32 lane, Fp2 *im, u32 z) {
    if (lane >= 6) return;
    Fp2 lo = Fp2::zero(), hi = Fp2::zero();
    for (u32 i = 0; i < 6; i++) {
        const bool wrap = i > lane;
        const Fp2 t = im[MI_WAVE_T + 6 * i + (wrap ? lane + 6 - i : lane - i)];
        if (wrap) hi = hi + t;
        else lo = lo + t;
    }
    im[z + w12_rec(lane)] = lo + fp2_mul_xi(hi);
}
// the line l0 + l3 w + l4 w^3 (three records anywhere in the image), lane 3 i + t: T[3 i + t] = x_i l_t
MI_HD void w12_ph_line_products(u32 lane, Fp2 *im, u32 x, u32 l0, u32 l3, u32 l4) {
    if (lane >= 18) return;
    const u32 i = lane / 3, t = lane - 3 * i;
    im[MI_WAVE_T + lane] = im[x + w12_rec(i)] * im[t == 0 ? l0 : t == 1 ? l3 : l4];
}
MI_HD void w12_ph_line_sums(u32 lane, Fp2 *im, u32 z) {
    if (lane >= 6) return;
    Fp2 lo = Fp2::zero(), hi = Fp2::zero();
    for (u32 t = 0; t < 3; t++) {
        const u32 pw = t + (t >> 1);   // 0, 1, 3
        const bool wrap = lane < pw;
        const Fp2 v = im[MI_WAVE_T + 3 * (wrap ? lane + 6 - pw : lane - pw) + t];
        if (wrap) hi = hi + v;
        else lo = lo + v;
    }
    im[z + w12_rec(lane)] = lo + fp2_mul_xi(hi);
}
// Granger-Scott (fp12_cyclo_sqr), records in the tower order (x0 .. x5): lanes 0 .. 5: T[k] = x_k^2; lanes 6, 7, 8: (x0 + x4)^2,
// (x2 + x3)^2, (x1 + x5)^2
MI_HD void w12_ph_cyclo_squares(u32 lane, Fp2 *im, u32 x) {
    if (lane >= 9) return;
    const u32 m = lane - 6;
    Fp2 u = im[x + (lane < 6 ? lane : m == 0 ? 0 : m == 1 ? 2 : 1)];
    if (lane >= 6) u = u + im[x + (m == 0 ? 4 : m == 1 ? 3 : 5)];
    im[MI_WAVE_T + lane] = fe_sqr(u);
}
// lane k reads x_k and writes z_k: in place is fine
MI_HD void w12_ph_cyclo_sums(u32 lane, Fp2 *im, u32 z, u32 x) {
    if (lane >= 6) return;
    const Fp2 *q = im + MI_WAVE_T;
    const Fp2 xk = im[x + lane];
    Fp2 s;
    if (lane < 3) {   // xi q_a + q_b, (a, b) = (4, 0), (2, 3), (5, 1); then 3 s - 2 x_k
        s = fp2_mul_xi(q[lane == 0 ? 4 : lane == 1 ? 2 : 5]) + q[lane == 0 ? 0 : lane == 1 ? 3 : 1];
        im[z + lane] = fe_dbl(s - xk) + s;
    } else {          // the cross term 2 x_a x_b = T[c] - q_a - q_b, (c, a, b) = (8, 1, 5) and xi, (6, 0, 4), (7, 2, 3); then 3 s + 2 x_k
        s = q[lane == 3 ? 8 : lane == 4 ? 6 : 7] - q[lane == 3 ? 1 : lane == 4 ? 0 : 2] - q[lane == 3 ? 5 : lane == 4 ? 4 : 3];
        if (lane == 3) s = fp2_mul_xi(s);
        im[z + lane] = fe_dbl(s + xk) + s;
    }
}
MI_HD void w12_ph_conj(u32 lane, Fp2 *im, u32 z, u32 x) {
    if (lane >= 6) return;
    const Fp2 v = im[x + lane];
    im[z + lane] = lane >= 3 ? fe_neg(v) : v;
}
MI_HD void w12_ph_copy(u32 lane, Fp2 *im, u32 z, u32 x) {
    if (lane < 6) im[z + lane] = im[x + lane];
}
MI_HD void w12_ph_add(u32 lane, Fp2 *im, u32 z, u32 x, u32 y, bool sub) {
    if (lane >= 6) return;
    const Fp2 a = im[x + lane], b = im[y + lane];
    im[z + lane] = sub ? a - b : a + b;
}
// xi^(e (p^k - 1) / 6) by name: the lane's power of w picks a constant, nothing is indexed
MI_HD Fp2 w12_frob_const(u32 k, u32 e) {
    switch (6 * (k - 1) + e) {
    case 1: return fp12c_frob1_1();
    case 2: return fp12c_frob1_2();
    case 3: return fp12c_frob1_3();
    case 4: return fp12c_frob1_4();
    case 5: return fp12c_frob1_5();
    case 7: return fp12c_frob2_1();
    case 8: return fp12c_frob2_2();
    case 9: return fp12c_frob2_3();
    case 10: return fp12c_frob2_4();
    case 11: return fp12c_frob2_5();
    case 13: return fp12c_frob3_1();
    case 14: return fp12c_frob3_2();
    case 15: return fp12c_frob3_3();
    case 16: return fp12c_frob3_4();
    case 17: return fp12c_frob3_5();
    default: return Fp2::one();   // e = 0
    }
}
// x^(p^k), k = 1, 2, 3: one constant product per lane (the product by one leaves the words as they are)
MI_HD void w12_ph_frob(u32 lane, Fp2 *im, u32 k, u32 z, u32 x) {
    if (lane >= 6) return;
    const Fp2 c = w12_frob_const(k, w12_pow(lane)), v = im[x + lane];
    im[z + lane] = k == 2 ? fp2_mul_fp(v, c.a0) : fp2_conj(v) * c;
}
MI_HD Fp12 w12_get(const Fp2 *im, u32 x) { return Fp12{Fp6{im[x], im[x + 1], im[x + 2]}, Fp6{im[x + 3], im[x + 4], im[x + 5]}}; }
MI_HD void w12_put(Fp2 *im, u32 z, const Fp12 &v) {
    im[z] = v.c0.b0; im[z + 1] = v.c0.b1; im[z + 2] = v.c0.b2; im[z + 3] = v.c1.b0; im[z + 4] = v.c1.b1; im[z + 5] = v.c1.b2;
}
// lanes 0 .. 5 carry one record each between an Fp12 in memory and the image
MI_HD void w12_ph_load(u32 lane, Fp2 *im, u32 z, const Fp12 *src) {
    if (lane < 6) im[z + lane] = ((const Fp2 *)src)[lane];
}
MI_HD void w12_ph_store(u32 lane, const Fp2 *im, Fp12 *dst, u32 x) {
    if (lane < 6) ((Fp2 *)dst)[lane] = im[x + lane];
}
MI_HD void w12_ph_set_one(u32 lane, Fp2 *im, u32 z) {
    if (lane < 6) im[z + lane] = lane ? Fp2::zero() : Fp2::one();
}
// lane 0: the six records at x equal v
MI_HD bool w12_equals(const Fp2 *im, u32 x, const Fp12 &v) { return w12_get(im, x) == v; }

// ---------------------------------------------------------------- operations: phases in order.  Out of line on the device, as the
// operations of fp12.cuh are: a final exponentiation calls a few hundred of them
MI_OOL void w12_mul(Fp2 *im, u32 z, u32 x, u32 y) {
    MI_WAVE_PHASE(w12_ph_mul_products(lane, im, x, y));
    MI_WAVE_PHASE(w12_ph_mul_sums(lane, im, z));
}
MI_OOL void w12_mul_line(Fp2 *im, u32 z, u32 x, u32 l0, u32 l3, u32 l4) {
    MI_WAVE_PHASE(w12_ph_line_products(lane, im, x, l0, l3, l4));
    MI_WAVE_PHASE(w12_ph_line_sums(lane, im, z));
}
MI_OOL void w12_cyclo_sqr(Fp2 *im, u32 z, u32 x) {
    MI_WAVE_PHASE(w12_ph_cyclo_squares(lane, im, x));
    MI_WAVE_PHASE(w12_ph_cyclo_sums(lane, im, z, x));
}
MI_OOL void w12_conj(Fp2 *im, u32 z, u32 x) { MI_WAVE_PHASE(w12_ph_conj(lane, im, z, x)); }
MI_OOL void w12_copy(Fp2 *im, u32 z, u32 x) { MI_WAVE_PHASE(w12_ph_copy(lane, im, z, x)); }
MI_OOL void w12_frob(Fp2 *im, u32 k, u32 z, u32 x) { MI_WAVE_PHASE(w12_ph_frob(lane, im, k, z, x)); }
// one lane's fp12_inv: about 400 serial Fp products, once per final exponentiation
MI_OOL void w12_inv(Fp2 *im, u32 z, u32 x) {
    MI_WAVE_PHASE(if (lane == 0) { Fp12 v = w12_get(im, x); fp12_inv(&v, &v); w12_put(im, z, v); });
}

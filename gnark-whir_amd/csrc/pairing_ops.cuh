// What the verifier's kernels (verify.hip) and the host build of the tests (tests/emu/emu_pairing.cpp, overflow traps on) both run, one
// record per lane / per call: the Fp12 operations of mi_debug_fp12_op_dev, the judgement of one proof from its Miller values, and the
// host half of one proof (its range and curve checks, kSum, the folds, the layout of its pairs) and of one batch (VerifyStage), which
// the host code of verify.hip and verify_combined.hip runs.
#pragma once
#include "pairing.cuh"
#include <cstring>
#include <utility>
#include <vector>

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

// ---------------------------------------------------------------- the host half of one proof (verify.hip's verify_run; the host build
// of the tests runs the same two functions).  The layouts are those of include/mi355x_groth16_verify.h: G1Aff = mi_g1_affine,
// G2Aff = mi_g2_affine, Fr = mi_fr, two G2Aff per mi_pedersen_vk.
struct VerifyKeyRef {
    const G1Aff *k0;                 // K[0]; K[1..] are the bases of the MSM, which the caller runs
    const G2Aff *gamma2, *delta2;
    const G2Aff *ped;                // 2 n_commitments points: G, GSigmaNeg of each commitment
    u32 n_pub, n_commitments;        // n_pub = nb_public - 1: without the ONE wire
};
struct VerifyProofRef {
    const G1Aff *ar;
    const G2Aff *bs;
    const G1Aff *krs, *commitments, *pok;
    const Fr *public_inputs, *commitment_values, *fold_challenge;
};
MI_HD u32 verify_pairs_per_proof(u32 n_commitments) { return MI_VERIFY_GROTH_PAIRS + (n_commitments ? n_commitments + 1 : 0); }
MI_HD G1Aff g1_aff_neg(const G1Aff &p) { return G1Aff{p.x, fe_neg(p.y)}; }

// What the host can say about a proof before any arithmetic: every coordinate below p, every scalar below r (fe_is_reduced), every G1
// point on the curve.  (Bs on the twist and in its r-torsion is the device's question, k_verify_g2_check.)  fold_challenge is read, and
// therefore checked, with more than one commitment only.  A proof that fails here is MI_VERIFY_MALFORMED and none of its words reaches
// the MSM, the group law or a Miller loop.  check_public = false: public_inputs is not read (the device decoded and checked them).
inline bool verify_well_formed(const VerifyKeyRef &vk, const VerifyProofRef &in, bool check_public = true) {
    const u32 nc = vk.n_commitments;
    bool ok = g1_on_curve(*in.ar) && g1_on_curve(*in.krs) && g2_reduced(*in.bs);
    if (nc) ok = ok && g1_on_curve(*in.pok);
    for (u32 k = 0; k < nc; k++) ok = ok && g1_on_curve(in.commitments[k]) && fe_is_reduced(in.commitment_values[k]);
    for (u32 i = 0; check_public && i < vk.n_pub; i++) ok = ok && fe_is_reduced(in.public_inputs[i]);
    if (nc > 1) ok = ok && fe_is_reduced(*in.fold_challenge);
    return ok;
}
// The pairs of one proof, p[] and q[] of verify_pairs_per_proof entries in the order below.  msm = sum_i public_inputs[i] K[1 + i] +
// sum_k commitment_values[k] K[nb_public + k], affine ((0, 0) = infinity, also when there is no scalar at all).  A proof that is not
// well formed gets pairs of infinities: its verdict is decided, and its words stay out of the arithmetic.
MI_HD void verify_assemble(const VerifyKeyRef &vk, const VerifyProofRef &in, bool well_formed, const G1Aff &msm, G1Aff *p, G2Aff *q) {
    const u32 nc = vk.n_commitments, np = verify_pairs_per_proof(nc);
    if (!well_formed) {
        for (u32 j = 0; j < np; j++) { p[j] = G1Aff{Fp::zero(), Fp::zero()}; q[j] = G2Aff{Fp2::zero(), Fp2::zero()}; }
        return;
    }
    G1X acc = G1X::from_affine(*vk.k0);
    xyzz_madd(acc, msm, false);
    for (u32 k = 0; k < nc; k++) xyzz_madd(acc, in.commitments[k], false);
    p[0] = *in.ar;                            q[0] = *in.bs;
    p[1] = g1_aff_neg(xyzz_to_affine(acc));   q[1] = *vk.gamma2;
    p[2] = g1_aff_neg(*in.krs);               q[2] = *vk.delta2;
    if (nc) {
        p[3] = *in.pok;                       q[3] = vk.ped[0];
        Fr ch = Fr::one(), pw = Fr::one();
        if (nc > 1) ch = *in.fold_challenge;
        for (u32 k = 0; k < nc; k++) {
            const G1Aff c = in.commitments[k];
            p[4 + k] = k ? xyzz_to_affine(xyzz_mul_256(G1X::from_affine(c), fe_from_mont(pw).l)) : c;   // c^0 = 1
            q[4 + k] = vk.ped[2 * k + 1];
            pw = pw * ch;
        }
    }
}

// The same for proof i of a staged batch whose arrays lie side by side: what one lane of k_verify_assemble (verify.hip) runs over device
// arrays and the host build of the tests over host ones.  ar, bs, krs, pok: one record per proof; cm: nc per proof; fold: one per proof,
// read with nc > 1 only; flags[i] != 0: not well formed; msm[i]: the scalar part of kSum.  p, q: verify_pairs_per_proof entries per proof.
struct VerifyAssembleArrays {
    VerifyKeyRef key;
    const G1Aff *ar;
    const G2Aff *bs;
    const G1Aff *krs, *cm, *pok;
    const Fr *fold;
    const uint8_t *flags;
    const G1Aff *msm;
};
MI_HD void verify_assemble_lane(const VerifyAssembleArrays &a, size_t i, G1Aff *p, G2Aff *q) {
    const u32 nc = a.key.n_commitments, np = verify_pairs_per_proof(nc);
    const VerifyProofRef in{a.ar + i, a.bs + i, a.krs + i, a.cm + i * nc, a.pok + i, nullptr, nullptr, a.fold + i};
    const G1Aff msm = a.msm[i];
    verify_assemble(a.key, in, a.flags[i] == 0, msm, p + i * np, q + i * np);
}

// The host's view of one batch before any device work: what mi_verify_run and mi_verify_combined_run (through mi_verify_open, verify.hip)
// and the host build of the tests all start from.  A proof whose decode_malformed byte (the array may be null) is set has none of its
// words read.  The references point into the caller's memory, which outlives the stage.
// pub_dev (optional): the public inputs of the batch already on the DEVICE, n x n_pub Montgomery values, row i for proof i, decoded and
// range-checked there (k_witness_decode, verify_bytes.hip: its answer arrives through decode_malformed).  With it the host neither reads
// nor checks public_inputs, and scal holds the commitment values alone.
struct VerifyStage {
    VerifyKeyRef key{};
    u32 n_pub = 0, nc = 0, ns = 0;         // ns = n_pub + nc: the scalars of one proof's kSum
    std::vector<VerifyProofRef> proofs;
    std::vector<uint8_t> flags;            // flags[i] = decode_malformed[i] || !verify_well_formed(proof i)
    const Fr *pub_dev = nullptr;
    u32 scal_cols = 0;                     // ns, or nc with pub_dev
    std::vector<Fr> scal;                  // n x scal_cols, row-major: public_inputs | commitment_values; a flagged proof's row is zero, never read
    size_t first_flagged = 0;              // the lowest i with flags[i], n() when there is none
    VerifyStage() = default;
    VerifyStage(const VerifyKeyRef &k, std::vector<VerifyProofRef> refs, const uint8_t *decode_malformed, const Fr *public_dev = nullptr)
        : key(k), n_pub(k.n_pub), nc(k.n_commitments), ns(n_pub + nc), proofs(std::move(refs)), flags(proofs.size(), 0), pub_dev(public_dev),
          scal_cols(public_dev ? nc : ns), scal(proofs.size() * scal_cols, Fr::zero()), first_flagged(proofs.size()) {
        const u32 own = pub_dev ? 0 : n_pub;   // the public columns this stage holds itself
        for (size_t i = n(); i-- > 0;) {
            const VerifyProofRef &in = proofs[i];
            if ((decode_malformed && decode_malformed[i]) || !verify_well_formed(key, in, !pub_dev)) { flags[i] = 1; first_flagged = i; continue; }
            if (own) std::memcpy(&scal[i * scal_cols], in.public_inputs, (size_t)own * sizeof(Fr));
            if (nc) std::memcpy(&scal[i * scal_cols + own], in.commitment_values, (size_t)nc * sizeof(Fr));
        }
    }
    size_t n() const { return proofs.size(); }
    // The device's half (k_verify_g2_check, Bs in the r-torsion of the twist): dev[i] != 0 flags proof i.  dev may be flags.data()
    // itself, after the kernel's bytes were copied back over it: the kernel only ever sets a byte.
    void merge(const uint8_t *dev) {
        for (size_t i = n(); i-- > 0;)
            if (dev[i]) { flags[i] = 1; first_flagged = i < first_flagged ? i : first_flagged; }
    }
};

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

// ---------------------------------------------------------------- one verdict for a batch (include/mi355x_groth16_verify_combined.h;
// csrc/verify_combined.hip and tests/emu/emu_verify_combined.cpp both run this text).  With coefficients r_i < 2^128 and S = sum r_i:
//     prod_i e(r_i Ar_i, Bs_i) e(-S alpha, beta) e(-(S K[0] + sum_j (sum_i r_i s_ij) K[1 + j] + sum_i r_i sum_k C_ik), gamma)
//            e(-sum_i r_i Krs_i, delta) = 1                                                                      else 1
//     e(sum_i r_i pok_i, G) prod_k e(sum_i (r_i c_i^k) C_ik, GSigmaNeg_k) = 1                                    else 2
// The n pairs (r_i Ar_i, Bs_i) come first, then the tail in the order of the single proof's pairs:
//     n: (-S alpha, beta)   n + 1: (-kSum, gamma)   n + 2: (-sum r_i Krs_i, delta)   then, with commitments:   n + 3: (sum r_i pok_i, G)
//     n + 4 + k: (sum_i r_i c_i^k C_ik, GSigmaNeg_k)

// a coefficient: four little-endian words of a plain integer below 2^128 -> the Montgomery scalar
MI_HD Fr fr_from_u128(const u32 k[4]) {
    Fr x = Fr::zero();
    for (int i = 0; i < 4; i++) x.l[i] = k[i];
    return fe_to_mont(x);
}
// k p for a plain integer k < 2^128: double-and-add (mixed additions of p) from the top bit in XYZZ, one inversion on the way back to affine.  (0, 0) = infinity
// in and out; k = 0 gives infinity.
MI_OOL G1Aff g1_scale128(const G1Aff &p, const u32 k[4]) {
    G1X acc = G1X::inf();
    for (int i = 127; i >= 0; i--) {
        acc = xyzz_dbl(acc);
        if ((k[i >> 5] >> (i & 31)) & 1) xyzz_madd(acc, p, false);
    }
    return xyzz_to_affine(acc);   // p = infinity: every mixed addition left acc at infinity
}
// x[0] x[1] ... x[cnt - 1] from the left, cnt >= 1.  Fp elements are fully reduced, so any grouping gives the same words.
MI_OOL void fp12_product_run(Fp12 *z, const Fp12 *x, size_t cnt) {
    Fp12 f = x[0];
    for (size_t i = 1; i < cnt; i++) {
        const Fp12 y = x[i];
        fp12_mul(&f, &f, &y);
    }
    *z = f;
}
#define MI_FP12_PRODUCT_FAN_IN 8   // values one lane of k_fp12_product multiplies; a level of m values leaves ceil(m / 8)

// What the MSMs of a batch give (affine, (0, 0) = infinity) and the sum of the coefficients
struct VerifyCombinedSums {
    Fr s;                   // S = sum r_i, Montgomery
    G1Aff k;                // sum_j (sum_i r_i s_ij) K[1 + j]
    G1Aff krs;              // sum_i r_i Krs_i
    G1Aff c;                // sum_i r_i sum_k C_ik
    G1Aff pok;              // sum_i r_i pok_i
    const G1Aff *ck;        // n_commitments points: sum_i (r_i c_i^k) C_ik
};
MI_HD u32 verify_combined_tail_pairs(u32 n_commitments) { return verify_pairs_per_proof(n_commitments); }
// The tail pairs, p[] and q[] of verify_combined_tail_pairs entries.  S K[0] and S alpha are single scalar multiplications.
inline void verify_combined_assemble(const VerifyKeyRef &vk, const G1Aff &alpha1, const G2Aff &beta2, const VerifyCombinedSums &m, G1Aff *p, G2Aff *q) {
    const u32 nc = vk.n_commitments;
    const Fr s = fe_from_mont(m.s);
    G1X acc = xyzz_mul_256(G1X::from_affine(*vk.k0), s.l);
    xyzz_madd(acc, m.k, false);
    xyzz_madd(acc, m.c, false);
    p[0] = g1_aff_neg(xyzz_to_affine(xyzz_mul_256(G1X::from_affine(alpha1), s.l)));   q[0] = beta2;
    p[1] = g1_aff_neg(xyzz_to_affine(acc));                                           q[1] = *vk.gamma2;
    p[2] = g1_aff_neg(m.krs);                                                         q[2] = *vk.delta2;
    if (nc) {
        p[3] = m.pok;                                                                 q[3] = vk.ped[0];
        for (u32 k = 0; k < nc; k++) { p[4 + k] = m.ck[k]; q[4 + k] = vk.ped[2 * k + 1]; }
    }
}
// The verdict from the two products after their final exponentiations (ped = null without commitments): 1, 2 or 0
MI_HD uint8_t verify_combined_judge(const Fp12 *groth, const Fp12 *ped) {
    if (!(*groth == Fp12::one())) return 1;
    if (ped && !(*ped == Fp12::one())) return 2;
    return 0;
}

// ---------------------------------------------------------------- which proof (include/mi355x_groth16_verify_locate.h;
// csrc/verify_locate.hip and tests/emu/emu_verify_locate.cpp both run this text).  The combined test is linear, so it judges any subset
// of a batch; the subsets are the nodes of the tree k_fp12_product walks: node (l, j) covers the proofs [j 8^l, min(n, (j + 1) 8^l)),
// level 0 is single proofs, the root is at level L = the number of product levels of n (at least 1).  What a node's test needs is
// computed once per proof and summed up the tree: the Miller values ml_i (Fp12 product tree) and the points below (G1 sum trees).
#define MI_LOCATE_ROUND_NODES 64   // node tests of one round, unless mi_debug_set_locate_round_nodes says otherwise

// The point arrays of the G1 sum trees: 0: r Krs   then, with commitments, 1: r sum_k C_k   2: r pok   and with more than one
// commitment 3 + k: (r c^k) C_k.  With one commitment array 1 IS (r c^0) C_0: it is not computed twice.
MI_HD u32 verify_locate_arrays(u32 nc) { return 1 + (nc ? 2 : 0) + (nc > 1 ? nc : 0); }
// One proof's points for the trees, out[a * stride] for array a; affine, (0, 0) = infinity in and out.  r: the coefficient, a plain
// integer below 2^128 (0 for a malformed proof: everything comes out infinite).  cm: the proof's nc commitments; fold is read with
// nc > 1 only.  (r c^k) is a full-width scalar: the canonical product goes through xyzz_mul_256.
MI_OOL void verify_locate_points(const u32 r[4], const G1Aff &krs, const G1Aff *cm, const G1Aff *pok, const Fr *fold, u32 nc, G1Aff *out, size_t stride) {
    out[0] = g1_scale128(krs, r);
    if (!nc) return;
    G1X sum = G1X::inf();
    for (u32 k = 0; k < nc; k++) xyzz_madd(sum, cm[k], false);
    out[stride] = g1_scale128(xyzz_to_affine(sum), r);
    out[2 * stride] = g1_scale128(*pok, r);
    if (nc == 1) return;
    const Fr c = *fold;
    Fr pw = fr_from_u128(r);
    for (u32 k = 0; k < nc; k++) {
        out[(3 + k) * stride] = xyzz_to_affine(xyzz_mul_256(G1X::from_affine(cm[k]), fe_from_mont(pw).l));
        pw = pw * c;
    }
}
// p[0] + ... + p[cnt - 1], cnt >= 1: XYZZ accumulation by the mixed addition (its doubling and cancelling branches included), one
// inversion back to affine
MI_OOL G1Aff g1_sum_run(const G1Aff *p, size_t cnt) {
    G1X acc = G1X::inf();
    for (size_t i = 0; i < cnt; i++) xyzz_madd(acc, p[i], false);
    return xyzz_to_affine(acc);
}
// One equation of a node before its final exponentiation.  eq 0: the tree's value (prod ml_i over the node) times the Miller values of
// tail pairs 0..2; eq 1 (with commitments): the product of the tail's values 3 .. np - 1.
MI_OOL void verify_locate_node_product(Fp12 *z, const Fp12 *tree, const Fp12 *tail, u32 np, u32 eq) {
    if (eq == 0) {
        Fp12 f = *tree;
        for (u32 t = 0; t < MI_VERIFY_GROTH_PAIRS; t++) { const Fp12 y = tail[t]; fp12_mul(&f, &f, &y); }
        *z = f;
    } else {
        fp12_product_run(z, tail + MI_VERIFY_GROTH_PAIRS, np - MI_VERIFY_GROTH_PAIRS);
    }
}

// The shape of the tree over n >= 1 proofs: cnt[l] nodes at level l = 0 .. L, off[l] = where level l starts in an array that keeps every level
struct LocateTree {
    size_t n = 0;
    u32 L = 0;
    std::vector<size_t> cnt, off;
    size_t total = 0;
    explicit LocateTree(size_t n_) : n(n_) {
        cnt.push_back(n);
        do cnt.push_back((cnt.back() + MI_FP12_PRODUCT_FAN_IN - 1) / MI_FP12_PRODUCT_FAN_IN); while (cnt.back() > 1);
        L = (u32)cnt.size() - 1;
        for (size_t c : cnt) { off.push_back(total); total += c; }
    }
    size_t first(u32 l, size_t j) const { return j << (3 * l); }                                  // the proofs of node (l, j): [first, end)
    size_t end(u32 l, size_t j) const { const size_t e = (j + 1) << (3 * l); return e < n ? e : n; }
};
static_assert(MI_FP12_PRODUCT_FAN_IN == 8, "LocateTree shifts by 3 bits per level");

struct LocateStats { uint32_t rounds = 0; uint64_t nodes_tested = 0, judged_alone = 0, malformed = 0, rejected = 0; };
// The descent: which nodes to test next, from the answers to the last round.  flags[i] != 0: proof i is malformed (decided, 3) and
// counts in no node.  Use: if (start()) do { pass[t] = the test of node (level, query[t]) } while (next(pass)); then suspects().
// A round is `query`, all on `level`.  A node test only ever decides "accepted": whatever fails or cannot be told goes on as a suspect.
struct LocatePlan {
    LocateTree tree;
    u32 cap;
    std::vector<size_t> good;          // good[i] = well-formed proofs below index i (n + 1 entries)
    u32 level = 0;                     // of `query`
    std::vector<size_t> query;         // node indices of this round, ascending
    std::vector<size_t> parent_end;    // query[parent_end[t - 1] .. parent_end[t]) are the children of the t-th failing node of the round before
    std::vector<size_t> failing;       // after the last round: the failing nodes, on `level`
    bool done_clean = false;           // the root passed, or there was nothing to test
    LocateStats stats;
    LocatePlan(size_t n, const uint8_t *flags, u32 cap_) : tree(n), cap(cap_ ? cap_ : MI_LOCATE_ROUND_NODES), good(n + 1, 0) {
        for (size_t i = 0; i < n; i++) good[i + 1] = good[i] + (flags[i] ? 0 : 1);
        stats.malformed = n - good[n];
    }
    size_t under(u32 l, size_t j) const { return good[tree.end(l, j)] - good[tree.first(l, j)]; }
    bool start() {
        if (!good[tree.n]) { done_clean = true; return false; }
        level = tree.L;
        query.assign(1, 0);
        parent_end.assign(1, 1);
        return round();
    }
    // pass[t] != 0: node query[t] passed
    bool next(const uint8_t *pass) {
        failing.clear();
        size_t t = 0;
        for (size_t e : parent_end) {
            const size_t from = failing.size(), t0 = t;
            for (; t < e; t++)
                if (!pass[t]) failing.push_back(query[t]);
            if (failing.size() == from && level != tree.L)     // every child of a failing node passed: all of them stay under suspicion
                for (size_t s = t0; s < e; s++) failing.push_back(query[s]);
        }
        if (failing.empty()) { done_clean = true; return false; }   // the root passed
        const u32 l = level;
        if (l == 1) return false;
        auto nodes_under = [&](u32 lo) {   // level-lo nodes under the failing ones
            size_t m = 0;
            for (size_t j : failing) m += children_end(l, j, lo) - (j << (3 * (l - lo)));
            return m;
        };
        u32 lo = l - 1;
        for (u32 c = 1; c < l; c++)
            if (nodes_under(c) <= cap) { lo = c; break; }
        size_t u = 0;
        for (size_t j : failing) u += under(l, j);
        if (u <= 2 * nodes_under(lo)) return false;   // a round that buys less than a halving
        query.clear();
        parent_end.clear();
        for (size_t j : failing) {
            for (size_t c = j << (3 * (l - lo)), e = children_end(l, j, lo); c < e; c++) query.push_back(c);
            parent_end.push_back(query.size());
        }
        level = lo;
        return round();
    }
    // the well-formed proofs under the failing nodes, ascending: what the per-proof body judges
    std::vector<size_t> suspects() {
        std::vector<size_t> out;
        if (!done_clean)
            for (size_t j : failing)
                for (size_t i = tree.first(level, j); i < tree.end(level, j); i++)
                    if (good[i + 1] != good[i]) out.push_back(i);
        stats.judged_alone = out.size();
        return out;
    }
private:
    size_t children_end(u32 l, size_t j, u32 lo) const { const size_t e = (j + 1) << (3 * (l - lo)); return e < tree.cnt[lo] ? e : tree.cnt[lo]; }
    bool round() { stats.rounds++; stats.nodes_tested += query.size(); return true; }
};

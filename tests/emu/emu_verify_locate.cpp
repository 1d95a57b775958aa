// Host build of the locating batch verifier (include/mi355x_groth16_verify_locate.h): the per-proof points, the G1 sum, the node's
// product, the shape of the tree and the descent (LocateTree, LocatePlan) of gnark-whir_amd/csrc/pairing_ops.cuh with the coefficients of
// combine_coeff.cuh -- the text csrc/verify_locate.hip's kernels and host code run, compiled with -DMI_CHECK_NOWRAP so that every bound
// of the arithmetic underneath traps.  The batch is staged by the library's own VerifyStage, both kinds of tree keep every level as on
// the device, the column sums are the kernels' arithmetic in a plain loop over a node's rows, and the MSMs are naive here (the device's
// run through msm.hip).  The host twins of mi_debug_g1_sum_tree_dev / mi_debug_locate_points_dev / mi_debug_locate_colsums_dev, of
// mi_groth16_verify_locate, and of mi_groth16_verify_batch for the proofs the descent hands over.
#include <cstddef>
#include <cstdint>
#include <algorithm>
#include <cstring>
#include <vector>
#include "../../gnark-whir_amd/csrc/pairing_ops.cuh"
#include "../../gnark-whir_amd/csrc/combine_coeff.cuh"

namespace {
G1X mul_mont(const G1Aff &p, const Fr &s) { return xyzz_mul_256(G1X::from_affine(p), fe_from_mont(s).l); }

struct Batch {
    VerifyKeyRef vk;
    const G1Aff *k, *alpha1;
    const G2Aff *beta2;
    std::vector<VerifyProofRef> refs;
};
Batch batch_of(const void *k, const void *alpha1, const void *beta2, const void *gamma2, const void *delta2, const void *ped, unsigned nb_public, unsigned nc,
               const void *raw, const void *commitments, const void *pok, const void *public_inputs, const void *commitment_values,
               const void *fold_challenge, size_t n) {
    const unsigned n_pub = nb_public - 1;
    Batch b{VerifyKeyRef{(const G1Aff *)k, (const G2Aff *)gamma2, (const G2Aff *)delta2, (const G2Aff *)ped, n_pub, nc}, (const G1Aff *)k,
            (const G1Aff *)alpha1, (const G2Aff *)beta2, std::vector<VerifyProofRef>(n)};
    const size_t raw_len = 2 * sizeof(G1Aff) + sizeof(G2Aff);
    for (size_t i = 0; i < n; i++) {
        const char *r = (const char *)raw + i * raw_len;
        b.refs[i] = VerifyProofRef{(const G1Aff *)r, (const G2Aff *)(r + sizeof(G1Aff)), (const G1Aff *)(r + sizeof(G1Aff) + sizeof(G2Aff)),
                                   (const G1Aff *)commitments + i * nc, (const G1Aff *)pok + i, (const Fr *)public_inputs + i * n_pub,
                                   (const Fr *)commitment_values + i * nc, fold_challenge ? (const Fr *)fold_challenge + i : nullptr};
    }
    return b;
}
// one proof the way mi_verify_run judges it (emu_pairing.cpp's emu_verify_assemble, with e(alpha, beta)^s computed here)
uint8_t judge_alone(const Batch &b, const VerifyProofRef &in, const Fp12 &eab) {
    const unsigned np = verify_pairs_per_proof(b.vk.n_commitments);
    VerifyStage st(b.vk, {in}, nullptr);
    G1X msm = G1X::inf();
    if (!st.flags[0])
        for (unsigned i = 0; i < st.ns; i++) xyzz_add(msm, mul_mont(b.k[1 + i], st.scal[i]));
    G1Aff p[MI_VERIFY_GROTH_PAIRS + 17];
    G2Aff q[MI_VERIFY_GROTH_PAIRS + 17];
    verify_assemble(b.vk, in, !st.flags[0], xyzz_to_affine(msm), p, q);
    const uint8_t off_torsion = !g2_in_subgroup(&q[0]);
    st.merge(&off_torsion);
    Fp12 ml[MI_VERIFY_GROTH_PAIRS + 17];
    for (unsigned i = 0; i < np; i++) pairing_miller_loop(&ml[i], &p[i], &q[i]);
    return verify_judge(ml, np - MI_VERIFY_GROTH_PAIRS, &eab, st.flags[0] != 0);
}
Fp12 e_alpha_beta(const Batch &b) {
    Fp12 f;
    pairing_miller_loop(&f, b.alpha1, b.beta2);
    pairing_final_exp(&f, &f);
    return f;
}
// sums[j] = sum over the rows of node (level, node) of r_i scal[i * ns + j]; sums[ns] = the sum of the r_i
void node_colsums(const Fr *scal, unsigned ns, const Fr *r, const LocateTree &tree, unsigned level, size_t node, Fr *sums) {
    for (unsigned j = 0; j <= ns; j++) sums[j] = Fr::zero();
    for (size_t i = tree.first(level, node); i < tree.end(level, node); i++) {
        const Fr ri = fe_to_mont(r[i]);
        for (unsigned j = 0; j < ns; j++) sums[j] = sums[j] + ri * scal[i * ns + j];
        sums[ns] = sums[ns] + ri;
    }
}
}   // namespace

extern "C" {
// levels: every level above p's, level 1 first (mi_debug_g1_sum_tree_dev)
int emu_g1_sum_tree(const void *p, size_t n, void *levels) {
    if (!n) return -1;
    const LocateTree tree(n);
    G1Aff *lv = (G1Aff *)levels;
    for (u32 l = 0; l < tree.L; l++) {
        const G1Aff *src = l ? lv + (tree.off[l] - n) : (const G1Aff *)p;
        for (size_t j = 0; j < tree.cnt[l + 1]; j++) {
            const size_t at = j * MI_FP12_PRODUCT_FAN_IN, left = tree.cnt[l] - at;
            lv[tree.off[l + 1] - n + j] = g1_sum_run(src + at, left < MI_FP12_PRODUCT_FAN_IN ? left : MI_FP12_PRODUCT_FAN_IN);
        }
    }
    return 0;
}
// r: n x 2 uint64; out[a * n + i] (mi_debug_locate_points_dev)
int emu_locate_points(const void *r, const void *krs, const void *cm, const void *pok, const void *fold, unsigned nc, size_t n, void *out) {
    if (nc > 16) return -1;
    const G1Aff inf{Fp::zero(), Fp::zero()};
    for (size_t i = 0; i < n; i++) {
        u32 rr[4];
        std::memcpy(rr, (const char *)r + 16 * i, 16);
        const G1Aff pk = nc ? ((const G1Aff *)pok)[i] : inf;
        const Fr f = nc > 1 ? ((const Fr *)fold)[i] : Fr::one();
        verify_locate_points(rr, ((const G1Aff *)krs)[i], (const G1Aff *)cm + i * nc, &pk, &f, nc, (G1Aff *)out + i, n);
    }
    return 0;
}
// nodes: m uint32; sums: m x (ns + 1) (mi_debug_locate_colsums_dev)
int emu_locate_colsums(const void *scal, unsigned ns, const void *r, size_t n, unsigned level, const uint32_t *nodes, size_t m, void *sums) {
    const LocateTree tree(n);
    if (level > tree.L) return -1;
    for (size_t t = 0; t < m; t++) {
        if (nodes[t] >= tree.cnt[level]) return -1;
        node_colsums((const Fr *)scal, ns, (const Fr *)r, tree, level, nodes[t], (Fr *)sums + t * (ns + 1));
    }
    return 0;
}
// every proof alone, as mi_groth16_verify_batch: verdicts[n]
int emu_verify_each(const void *k, const void *alpha1, const void *beta2, const void *gamma2, const void *delta2, const void *ped, unsigned nb_public,
                    unsigned nc, const void *raw, const void *commitments, const void *pok, const void *public_inputs, const void *commitment_values,
                    const void *fold_challenge, size_t n, uint8_t *verdicts) {
    if (nb_public == 0 || nc > 16) return -1;
    const Batch b = batch_of(k, alpha1, beta2, gamma2, delta2, ped, nb_public, nc, raw, commitments, pok, public_inputs, commitment_values, fold_challenge, n);
    const Fp12 eab = e_alpha_beta(b);
    for (size_t i = 0; i < n; i++) verdicts[i] = judge_alone(b, b.refs[i], eab);
    return 0;
}
// One whole batch the way verify_locate.hip's mi_verify_locate_run judges it.  The arguments of emu_verify_combined (emu_verify_combined.cpp),
// cap as mi_debug_set_locate_round_nodes; verdicts[n]; stats: rounds, nodes_tested, judged_alone, malformed, rejected.
int emu_verify_locate(const void *k, const void *alpha1, const void *beta2, const void *gamma2, const void *delta2, const void *ped, unsigned nb_public,
                      unsigned nc, const void *raw, const void *commitments, const void *pok, const void *public_inputs, const void *commitment_values,
                      const void *fold_challenge, size_t n, const void *seed, unsigned cap, uint8_t *verdicts, uint64_t *stats) {
    if (nb_public == 0 || nc > 16) return -1;
    for (int s = 0; s < 5; s++) stats[s] = 0;
    if (!n) return 0;
    const Batch b = batch_of(k, alpha1, beta2, gamma2, delta2, ped, nb_public, nc, raw, commitments, pok, public_inputs, commitment_values, fold_challenge, n);
    const unsigned np = verify_combined_tail_pairs(nc), na = verify_locate_arrays(nc);
    VerifyStage st(b.vk, b.refs, nullptr);
    const unsigned ns = st.ns;
    std::vector<uint8_t> off_torsion(n);
    for (size_t i = 0; i < n; i++) off_torsion[i] = !st.flags[i] && !g2_in_subgroup(st.proofs[i].bs);
    st.merge(off_torsion.data());
    for (size_t i = 0; i < n; i++)
        if (st.flags[i]) std::fill(st.scal.begin() + i * st.ns, st.scal.begin() + (i + 1) * st.ns, Fr::zero());
    LocatePlan plan(n, st.flags.data(), cap);
    const LocateTree &tree = plan.tree;
    for (size_t i = 0; i < n; i++) verdicts[i] = st.flags[i] ? 3 : 0;
    if (plan.start()) {
        // ---- once per batch: the coefficients (0 for a malformed proof), the Miller values, the per-proof points, both kinds of tree
        const G1Aff inf{Fp::zero(), Fp::zero()};
        std::vector<Fr> r(n, Fr::zero());
        std::vector<Fp12> ml(tree.total);
        std::vector<G1Aff> g1(na * tree.total);
        for (size_t i = 0; i < n; i++) {
            G1Aff p = inf;
            G2Aff q{Fp2::zero(), Fp2::zero()};
            if (!st.flags[i]) {
                const VerifyProofRef &in = st.proofs[i];
                combine_coefficient((const uint8_t *)seed, n, i, r[i].l);
                p = g1_scale128(*in.ar, r[i].l);
                q = *in.bs;
                verify_locate_points(r[i].l, *in.krs, in.commitments, in.pok, in.fold_challenge, nc, &g1[i], tree.total);
            } else {
                for (unsigned a = 0; a < na; a++) g1[a * tree.total + i] = inf;
            }
            pairing_miller_loop(&ml[i], &p, &q);
        }
        for (u32 l = 0; l < tree.L; l++)
            for (size_t j = 0; j < tree.cnt[l + 1]; j++) {
                const size_t at = j * MI_FP12_PRODUCT_FAN_IN, left = tree.cnt[l] - at, cnt = left < MI_FP12_PRODUCT_FAN_IN ? left : MI_FP12_PRODUCT_FAN_IN;
                fp12_product_run(&ml[tree.off[l + 1] + j], &ml[tree.off[l] + at], cnt);
                for (unsigned a = 0; a < na; a++) g1[a * tree.total + tree.off[l + 1] + j] = g1_sum_run(&g1[a * tree.total + tree.off[l] + at], cnt);
            }
        // ---- the rounds
        std::vector<uint8_t> pass;
        std::vector<Fr> col(ns + 1);
        std::vector<G1Aff> ck(nc), P(np);
        std::vector<G2Aff> Q(np);
        do {
            const u32 l = plan.level;
            pass.assign(plan.query.size(), 0);
            for (size_t t = 0; t < plan.query.size(); t++) {
                const size_t j = plan.query[t], at = tree.off[l] + j;
                node_colsums(st.scal.data(), ns, r.data(), tree, l, j, col.data());
                G1X mk = G1X::inf();
                for (unsigned c = 0; c < ns; c++) xyzz_add(mk, mul_mont(b.k[1 + c], col[c]));
                VerifyCombinedSums sums{col[ns], xyzz_to_affine(mk), g1[at], inf, inf, ck.data()};
                if (nc) { sums.c = g1[tree.total + at]; sums.pok = g1[2 * tree.total + at]; }
                for (unsigned c = 0; c < nc; c++) ck[c] = nc > 1 ? g1[(3 + c) * tree.total + at] : sums.c;
                verify_combined_assemble(b.vk, *b.alpha1, *b.beta2, sums, P.data(), Q.data());
                std::vector<Fp12> tail(np);
                for (unsigned s = 0; s < np; s++) pairing_miller_loop(&tail[s], &P[s], &Q[s]);
                Fp12 groth, pd;
                verify_locate_node_product(&groth, &ml[at], tail.data(), np, 0);
                pairing_final_exp(&groth, &groth);
                if (nc) {
                    verify_locate_node_product(&pd, &ml[at], tail.data(), np, 1);
                    pairing_final_exp(&pd, &pd);
                }
                pass[t] = verify_combined_judge(&groth, nc ? &pd : nullptr) == 0;
            }
        } while (plan.next(pass.data()));
    }
    const std::vector<size_t> sus = plan.suspects();
    if (!sus.empty()) {
        const Fp12 eab = e_alpha_beta(b);
        for (size_t i : sus) {
            verdicts[i] = judge_alone(b, b.refs[i], eab);
            if (verdicts[i] == 1 || verdicts[i] == 2) plan.stats.rejected++;
        }
    }
    stats[0] = plan.stats.rounds; stats[1] = plan.stats.nodes_tested; stats[2] = plan.stats.judged_alone;
    stats[3] = plan.stats.malformed; stats[4] = plan.stats.rejected;
    return 0;
}
}

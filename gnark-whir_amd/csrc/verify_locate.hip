// One verdict PER PROOF at the combined test's price for a good batch (include/mi355x_groth16_verify_locate.h): the combined test of
// verify_combined.hip on a tree of subsets of the batch, descending only into subsets that fail.  The per-proof bodies, the node's
// product, the shape of the tree (LocateTree) and the descent (LocatePlan) are in pairing_ops.cuh; the host build of the tests
// (tests/emu/emu_verify_locate.cpp) runs the same text.
//
// Once per batch, every launch on ctx->stream:
//   host      mi_verify_open (verify.hip): the argument checks and the VerifyStage, as the other three bodies.  The front from here to
//             mi_verify_put_coeffs' uploads is the combined body's, the same functions (verify_combined.hip)
//   k_verify_g2_check (verify.hip)   Bs of every proof that passed the host's checks -> the malformed flags (mi_verify_flag_bs).  A
//             malformed proof gets 3, coefficient 0 and infinities for all of its points from here on: none of its words reaches any arithmetic
//   host      the coefficients r_i of the combined verifier: combine_coefficient(seed, n, i), the full n and the original index
//   k_g1_scale128, k_pairing_miller   r_i Ar_i, then ONE Miller launch over the n pairs -> ml[i] (one for a malformed proof)
//   k_verify_locate_points   one lane per proof: r_i Krs_i, r_i sum_k C_ik, r_i pok_i and with more than one commitment (r_i c_i^k) C_ik
//   k_g1_sum_level   per level, all point arrays in one launch: out[j] = the sum of up to 8 points.  EVERY level is kept
//   k_fp12_product (verify_combined.hip)   per level over ml: EVERY level is kept, and no tail is inside the tree
// Per round (m nodes of one level, LocatePlan::query):
//   k_verify_locate_colsums / _reduce   sum_{i in node} r_i s_ij per (node, column), column ns = S: (node, column, block) -> partials
//             -> one sum each.  The scalar matrix stays level 0 only; the cost is the rows the queried nodes cover.  The combined
//             body runs the same pair over the root (mi_verify_colsums_enqueue)
//   k_verify_locate_gather   the m nodes' values of every G1 tree, side by side for one copy
//   host      per node one mi_verify_msm over the resident K[1..] with the node's column sums (host-synchronous: the known cost of a
//             node); the other sums are those gathered out of the G1 trees; verify_combined_assemble, unchanged, gives the node's tail pairs
//   k_pairing_miller   ONE launch over the m * tail pairs
//   k_verify_locate_node_products   one lane per (node, equation): the tree's value times its tails
//   k_pairing_final_exp   ONE launch over them
//   k_verify_locate_judge   m pass / fail bytes, back in one copy
// At the end the proofs still under suspicion go, as one contiguous array, through mi_verify_run (verify.hip): verdicts 1 and 2 come
// from there only.
// Workspace: the locate layout has a slot of its own, WS_VERIFY_LOCATE (ctx.h), because mi_verify_run and mi_verify_msm lay WS_VERIFY
// and the MSM's slots out their own way while the trees must live across rounds.  Everything of a batch, the rounds' regions sized for
// the largest round the tree allows, is reserved in ONE mi_reserve before the first launch: a later growth would drop the trees.
#include "verify_internal.h"
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

namespace {

#define MI_LOCATE_MAX_NODE_BLOCKS 256   // blocks over one node's rows in k_verify_locate_colsums

// One lane per proof.  r: the coefficients, four words each, r_stride words apart.  cm: n x nc.  out[a * stride + i]: array a of
// verify_locate_arrays(nc).  pok, cm are read with nc > 0, fold with nc > 1.
__global__ void __launch_bounds__(64, 1) k_verify_locate_points(const u32 *r, u32 r_stride, const G1Aff *krs, const G1Aff *cm, const G1Aff *pok,
                                                                const Fr *fold, u32 nc, size_t n, G1Aff *out, size_t stride) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 rr[4];
    for (int w = 0; w < 4; w++) rr[w] = r[i * r_stride + w];
    G1Aff c[MI_PK_RAW_MAX_COMMITMENTS];
    for (u32 k = 0; k < nc; k++) c[k] = cm[i * nc + k];
    const G1Aff kr = krs[i], pk = nc ? pok[i] : G1Aff{Fp::zero(), Fp::zero()};
    const Fr f = nc > 1 ? fold[i] : Fr::one();
    verify_locate_points(rr, kr, c, &pk, &f, nc, out + i, stride);
}
// One level of na sum trees in one launch: lane (a, j) writes out[a * out_stride + j] = the sum of in[a * in_stride + 8 j ..], up to 8
// points and n_in in all per array; j < n_out = ceil(n_in / 8)
__global__ void __launch_bounds__(64, 1) k_g1_sum_level(const G1Aff *in, size_t in_stride, size_t n_in, G1Aff *out, size_t out_stride, size_t n_out, u32 na) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_out * na) return;
    const size_t a = t / n_out, j = t % n_out, at = j * MI_FP12_PRODUCT_FAN_IN, left = n_in - at;
    const size_t cnt = left < MI_FP12_PRODUCT_FAN_IN ? left : MI_FP12_PRODUCT_FAN_IN;
    G1Aff p[MI_FP12_PRODUCT_FAN_IN];
    for (size_t s = 0; s < cnt; s++) p[s] = in[a * in_stride + at + s];
    out[a * out_stride + j] = g1_sum_run(p, cnt);
}
// The column sums of both coefficient bodies (mi_verify_colsums_enqueue, verify_internal.h).  scal: n x ns Montgomery scalars,
// row-major.  Block ((t (ns + 1) + j) bpn + b) adds up column j (column ns: the coefficients themselves, S) over the proofs first +
// b * 64 + lane, + bpn * 64, ... of node (level, nodes[t]); nodes == null: node t.  r: canonical records below 2^128, 0 for a malformed
// proof.  partial[blockIdx.x].  With rc (the combined body, one node: the root) the blocks of column ns also write r_i c_i^k
// (Montgomery; c_i = fold[i], or 1 without fold) and r_i again (canonical) at [k * n + i], k < nc, for the MSMs over the commitments.
// Exact field arithmetic: the order of the additions does not reach the result.
__global__ void __launch_bounds__(64, 1) k_verify_locate_colsums(const Fr *scal, u32 ns, const Fr *r, size_t n, u32 level, const u32 *nodes, u32 bpn, Fr *partial,
                                                                 const Fr *fold, u32 nc, Fr *rc, Fr *rrep) {
    __shared__ Fr sh[64];
    const u32 b = blockIdx.x % bpn, lane = threadIdx.x;
    const size_t tj = blockIdx.x / bpn, t = tj / (ns + 1);
    const u32 j = (u32)(tj % (ns + 1));
    const size_t first = (nodes ? (size_t)nodes[t] : t) << (3 * level);
    size_t end = first + ((size_t)1 << (3 * level));
    if (end > n) end = n;
    Fr acc = Fr::zero();
    for (size_t i = first + (size_t)b * 64 + lane; i < end; i += (size_t)bpn * 64) {
        const Fr plain = r[i];
        const Fr ri = fe_to_mont(plain);
        acc = j < ns ? acc + ri * scal[i * ns + j] : acc + ri;
        if (j < ns || !rc) continue;
        const Fr c = fold ? fold[i] : Fr::one();
        Fr pw = ri;
        for (u32 k = 0; k < nc; k++) {
            rc[(size_t)k * n + i] = pw;
            rrep[(size_t)k * n + i] = plain;
            pw = pw * c;
        }
    }
    sh[lane] = acc;
    __syncthreads();
    for (u32 s = 32; s > 0; s >>= 1) {
        if (lane < s) sh[lane] = sh[lane] + sh[lane + s];
        __syncthreads();
    }
    if (lane == 0) partial[blockIdx.x] = sh[0];
}
// sums[c] = the sum of the bpn partials of (node, column) c
__global__ void __launch_bounds__(64, 1) k_verify_locate_colsums_reduce(const Fr *partial, u32 bpn, Fr *sums, size_t count) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= count) return;
    Fr acc = Fr::zero();
    for (u32 b = 0; b < bpn; b++) acc = acc + partial[c * bpn + b];
    sums[c] = acc;
}
// One lane per (node, equation): res[t * neq + eq]; tree_level: the level of the Fp12 tree the nodes are on; tail: m x np Miller values
__global__ void __launch_bounds__(64, 1) k_verify_locate_node_products(const Fp12 *tree_level, const u32 *nodes, const Fp12 *tail, u32 np, u32 neq, Fp12 *res, size_t m) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m * neq) return;
    const size_t t = i / neq;
    const Fp12 tr = tree_level[nodes[t]];
    Fp12 f;
    verify_locate_node_product(&f, &tr, tail + t * np, np, (u32)(i % neq));
    res[i] = f;
}
// out[a * m + t] = the value of array a at node nodes[t] of one level (level: where that level starts in array 0; arrays `stride` apart):
// what a round reads out of the G1 trees, gathered so that the copy to the host is proportional to the round
__global__ void __launch_bounds__(64, 1) k_verify_locate_gather(const G1Aff *level, size_t stride, const u32 *nodes, size_t m, u32 na, G1Aff *out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m * na) return;
    out[i] = level[(i / m) * stride + nodes[i % m]];
}
// pass[t] = both results of node t (one without commitments) are one
__global__ void __launch_bounds__(64, 1) k_verify_locate_judge(const Fp12 *res, u32 neq, uint8_t *pass, size_t m) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m) return;
    pass[t] = verify_combined_judge(&res[t * neq], neq > 1 ? &res[t * neq + 1] : nullptr) == 0 ? 1 : 0;
}

// the most nodes a round over this tree can have: the root alone, or every node of level 1
size_t max_round_nodes(const LocateTree &t) { return t.L >= 2 ? t.cnt[1] : 1; }
size_t max_round_partials(const LocateTree &t, u32 ns) {
    size_t most = 0;
    for (u32 l = 1; l <= t.L; l++) {
        const size_t m = t.cnt[l] < max_round_nodes(t) ? t.cnt[l] : max_round_nodes(t), p = m * (ns + 1) * mi_verify_node_blocks(l, t.n);
        most = p > most ? p : most;
    }
    return most;
}

}   // namespace

// blocks over the rows of one node of `level` in a tree over n proofs
u32 mi_verify_node_blocks(u32 level, size_t n) {
    size_t rows = (size_t)1 << (3 * level);
    if (rows > n) rows = n;
    const size_t b = mi_blocks_of(rows, 64);
    return (u32)(b < MI_LOCATE_MAX_NODE_BLOCKS ? b : MI_LOCATE_MAX_NODE_BLOCKS);
}
int32_t mi_verify_colsums_enqueue(mi_ctx *ctx, const Fr *scal, u32 ns, const Fr *r, size_t n, u32 level, const u32 *nodes_dev, size_t m, Fr *partial, Fr *sums,
                                  const Fr *fold, u32 nc, Fr *rc, Fr *rrep) {
    const u32 bpn = mi_verify_node_blocks(level, n);
    const size_t blocks = m * (ns + 1) * bpn;
    if (blocks > 0x7fffffffu) MI_FAIL(ctx, MI_EINVAL, "verify locate: a round of " + std::to_string(m) + " nodes times the key's scalar columns exceeds one launch");
    MI_TRY(mi_launch64(ctx, k_verify_locate_colsums, blocks * 64, scal, ns, r, n, level, nodes_dev, bpn, partial, fold, nc, rc, rrep));
    return mi_launch64(ctx, k_verify_locate_colsums_reduce, m * (ns + 1), (const Fr *)partial, bpn, sums, m * (ns + 1));
}

int32_t mi_verify_locate_run(mi_ctx *ctx, const mi_vk *vk, const mi_verify_input *in, size_t n, const uint8_t *seed, uint8_t *verdicts,
                             mi_verify_locate_stats *stats, const uint8_t *decode_malformed, const Fr *pub_dev) {
    // the combined call's refusals, in its order
    MI_TRY(mi_verify_refuse_msm_pairs(ctx, vk, in && verdicts, n, "verify locate: n * n_commitments above MI_MSM_MAX_PAIRS"));
    VerifyStage st;
    MI_TRY(mi_verify_open(ctx, "verify locate: ", vk, in, n, verdicts || !n, decode_malformed, &st, pub_dev));
    const u32 nc = st.nc, ns = st.ns, np = verify_combined_tail_pairs(nc), na = verify_locate_arrays(nc), neq = nc ? 2 : 1;
    uint8_t own_seed[32];
    if (n) MI_TRY(mi_verify_seed(ctx, "verify locate: ", seed, own_seed));
    auto report = [&](const LocateStats &s) {
        if (stats) *stats = mi_verify_locate_stats{s.rounds, s.nodes_tested, s.judged_alone, s.malformed, s.rejected};
    };
    if (!n) { report(LocateStats{}); return MI_OK; }

    // ---- workspace: the batch, the two kinds of tree with every level, then the regions of one round
    const LocateTree tree(n);
    const size_t m_max = max_round_nodes(tree);
    WsCut cut;
    const size_t off_scal = cut.take(n * ns * sizeof(Fr)), off_r = cut.take(n * sizeof(Fr)), off_fold = cut.take(n * sizeof(Fr));
    const size_t off_krs = cut.take(n * sizeof(G1Aff)), off_pok = cut.take(n * sizeof(G1Aff)), off_cm = cut.take(n * nc * sizeof(G1Aff));
    const size_t off_p = cut.take(n * sizeof(G1Aff)), off_q = cut.take(n * sizeof(G2Aff)), off_fl = cut.take(n);
    const size_t off_ml = cut.take(tree.total * sizeof(Fp12)), off_g1 = cut.take(na * tree.total * sizeof(G1Aff));
    const size_t off_nodes = cut.take(m_max * sizeof(u32)), off_part = cut.take(max_round_partials(tree, ns) * sizeof(Fr));
    const size_t off_sum = cut.take(m_max * (ns + 1) * sizeof(Fr)), off_tp = cut.take(m_max * np * sizeof(G1Aff)), off_tq = cut.take(m_max * np * sizeof(G2Aff));
    const size_t off_tml = cut.take(m_max * np * sizeof(Fp12)), off_res = cut.take(m_max * neq * sizeof(Fp12)), off_pass = cut.take(m_max);
    const size_t off_gather = cut.take(m_max * na * sizeof(G1Aff));
    MI_TRY(mi_reserve(ctx, ctx->ws[WS_VERIFY_LOCATE], cut.total));
    char *ws = (char *)ctx->ws[WS_VERIFY_LOCATE].p;

    // ---- malformed first, per proof: Bs of the proofs that passed the host's checks (infinity stands in for the others)
    const G1Aff inf{Fp::zero(), Fp::zero()};
    std::vector<G2Aff> Q(n);
    MI_TRY(mi_verify_flag_bs(ctx, st, Q.data(), (G2Aff *)(ws + off_q), (uint8_t *)(ws + off_fl)));
    LocatePlan plan(n, st.flags.data(), ctx->locate_round_nodes);
    std::vector<uint8_t> out(n, MI_VERIFY_OK);
    for (size_t i = 0; i < n; i++) {   // a proof the device's check flagged too: its scalar row and its Bs go the way of its points
        if (!st.flags[i]) continue;
        out[i] = MI_VERIFY_MALFORMED;
        std::fill(st.scal.begin() + i * st.scal_cols, st.scal.begin() + (i + 1) * st.scal_cols, Fr::zero());
        Q[i] = G2Aff{Fp2::zero(), Fp2::zero()};
    }

    if (plan.start()) {
        // ---- host: the coefficients and the points ([i][k]); a malformed proof has coefficient 0, infinities and a zero scalar row
        VerifyCoeffs h;
        MI_TRY(mi_verify_upload(ctx, ws + off_q, Q.data(), n * sizeof(G2Aff)));   // again: a proof the device's check flagged becomes infinity
        MI_TRY(mi_verify_put_coeffs(ctx, st, in, seed, false, &h, ws, VerifyCoeffsAt{off_scal, off_r, off_fold, off_krs, off_pok, off_cm, off_p}));

        // ---- device, once per batch: the Miller values, the per-proof points, both kinds of tree
        Fp12 *ml = (Fp12 *)(ws + off_ml);
        G1Aff *g1 = (G1Aff *)(ws + off_g1);
        const Fr *r_dev = (const Fr *)(ws + off_r);
        MI_TRY(mi_g1_scale128_enqueue(ctx, (const G1Aff *)(ws + off_p), (const u32 *)r_dev, 8u, (G1Aff *)(ws + off_p), n));
        MI_TRY(mi_pairing_enqueue(ctx, (const G1Aff *)(ws + off_p), (const G2Aff *)(ws + off_q), n, ml, false));
        MI_TRY(mi_launch64(ctx, k_verify_locate_points, n, (const u32 *)r_dev, 8u, (const G1Aff *)(ws + off_krs), (const G1Aff *)(ws + off_cm),
                           (const G1Aff *)(ws + off_pok), (const Fr *)(ws + off_fold), nc, n, g1, tree.total));
        for (u32 l = 0; l < tree.L; l++) {
            MI_TRY(mi_launch64(ctx, k_g1_sum_level, tree.cnt[l + 1] * na, (const G1Aff *)(g1 + tree.off[l]), tree.total, tree.cnt[l], g1 + tree.off[l + 1],
                               tree.total, tree.cnt[l + 1], na));
            MI_TRY(mi_fp12_product_level_enqueue(ctx, ml + tree.off[l], tree.cnt[l], ml + tree.off[l + 1], tree.cnt[l + 1]));
        }

        // ---- the rounds
        std::vector<u32> nodes;
        std::vector<Fr> hsum;
        std::vector<G1Aff> hpts, tp, ck(nc, inf);
        std::vector<G2Aff> tq;
        std::vector<uint8_t> pass;
        do {
            const u32 l = plan.level;
            const size_t m = plan.query.size();
            if (m > m_max) MI_FAIL(ctx, MI_EINVAL, "verify locate: a round larger than the tree allows");
            nodes.assign(plan.query.begin(), plan.query.end());
            MI_TRY(mi_verify_upload(ctx, ws + off_nodes, nodes.data(), m * sizeof(u32)));
            const u32 *nodes_dev = (const u32 *)(ws + off_nodes);
            MI_TRY(mi_verify_colsums_enqueue(ctx, (const Fr *)(ws + off_scal), ns, r_dev, n, l, nodes_dev, m, (Fr *)(ws + off_part), (Fr *)(ws + off_sum)));
            hsum.resize(m * (ns + 1));
            hpts.resize(na * m);
            MI_TRY(mi_launch64(ctx, k_verify_locate_gather, m * na, (const G1Aff *)(g1 + tree.off[l]), tree.total, nodes_dev, m, na, (G1Aff *)(ws + off_gather)));
            MI_CHECK_HIP(ctx, hipMemcpyAsync(hsum.data(), ws + off_sum, hsum.size() * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
            MI_CHECK_HIP(ctx, hipMemcpyAsync(hpts.data(), ws + off_gather, hpts.size() * sizeof(G1Aff), hipMemcpyDeviceToHost, ctx->stream));
            MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
            tp.resize(m * np);
            tq.resize(m * np);
            for (size_t t = 0; t < m; t++) {
                VerifyCombinedSums sums{};
                sums.s = hsum[t * (ns + 1) + ns];
                sums.k = sums.c = sums.pok = inf;
                if (ns && plan.under(l, plan.query[t]))   // host-synchronous, one per node: the known cost of a node
                    MI_TRY(mi_verify_msm(ctx, vk->k_dev, ws + off_sum + t * (ns + 1) * sizeof(Fr), ns, 0, &sums.k));
                sums.krs = hpts[t];
                if (nc) { sums.c = hpts[m + t]; sums.pok = hpts[2 * m + t]; }
                for (u32 k = 0; k < nc; k++) ck[k] = nc > 1 ? hpts[(3 + k) * m + t] : sums.c;
                sums.ck = ck.data();
                verify_combined_assemble(st.key, vk->alpha1, vk->beta2, sums, &tp[t * np], &tq[t * np]);
            }
            MI_TRY(mi_verify_upload(ctx, ws + off_tp, tp.data(), m * np * sizeof(G1Aff)));
            MI_TRY(mi_verify_upload(ctx, ws + off_tq, tq.data(), m * np * sizeof(G2Aff)));
            Fp12 *tml = (Fp12 *)(ws + off_tml), *res = (Fp12 *)(ws + off_res);
            MI_TRY(mi_pairing_enqueue(ctx, (const G1Aff *)(ws + off_tp), (const G2Aff *)(ws + off_tq), m * np, tml, false));
            MI_TRY(mi_launch64(ctx, k_verify_locate_node_products, m * neq, (const Fp12 *)(ml + tree.off[l]), nodes_dev, (const Fp12 *)tml, np, neq, res, m));
            MI_TRY(mi_final_exp_enqueue(ctx, res, m * neq));
            MI_TRY(mi_launch64(ctx, k_verify_locate_judge, m, (const Fp12 *)res, neq, (uint8_t *)(ws + off_pass), m));
            pass.resize(m);
            MI_CHECK_HIP(ctx, hipMemcpyAsync(pass.data(), ws + off_pass, m, hipMemcpyDeviceToHost, ctx->stream));
            MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        } while (plan.next(pass.data()));
    }

    // ---- the proofs still under suspicion: one contiguous array through the per-proof body, verdicts back by original index
    const std::vector<size_t> sus = plan.suspects();
    if (!sus.empty()) {
        std::vector<mi_verify_input> alone(sus.size());
        std::vector<uint8_t> vd(sus.size(), 255);
        for (size_t t = 0; t < sus.size(); t++) alone[t] = in[sus[t]];
        // a device-resident public block: the suspects' rows, gathered over the scalar matrix, which the rounds have finished with
        Fr *sus_pub = st.pub_dev ? (Fr *)(ws + off_scal) : nullptr;
        for (size_t t = 0; sus_pub && t < sus.size(); t++)
            MI_CHECK_HIP(ctx, hipMemcpyAsync(sus_pub + t * st.n_pub, st.pub_dev + sus[t] * st.n_pub, (size_t)st.n_pub * sizeof(Fr), hipMemcpyDeviceToDevice, ctx->stream));
        MI_TRY(mi_verify_run(ctx, vk, alone.data(), alone.size(), vd.data(), nullptr, sus_pub));
        for (size_t t = 0; t < sus.size(); t++) {
            out[sus[t]] = vd[t];
            if (vd[t] == MI_VERIFY_PAIRING || vd[t] == MI_VERIFY_PEDERSEN) plan.stats.rejected++;
        }
    }
    std::memcpy(verdicts, out.data(), n);
    report(plan.stats);
    return MI_OK;
}

extern "C" {

int32_t mi_groth16_verify_locate(mi_ctx *ctx, const mi_vk *vk, const mi_verify_input *in, size_t n, const uint8_t *seed, uint8_t *verdicts,
                                 mi_verify_locate_stats *stats) {
    return mi_verify_locate_run(ctx, vk, in, n, seed, verdicts, stats, nullptr);
}

// ---------------------------------------------------------------- debug surface (include/mi355x_groth16_debug.h)
int32_t mi_debug_g1_sum_tree_dev(mi_ctx *ctx, const mi_g1_affine *p_dev, size_t n, mi_g1_affine *levels_dev) {
    if (!ctx || !p_dev || !levels_dev || n == 0 || n > ((size_t)1 << 24)) return MI_EINVAL;
    const LocateTree tree(n);
    G1Aff *lv = (G1Aff *)levels_dev;
    for (u32 l = 0; l < tree.L; l++) {
        const G1Aff *src = l ? lv + (tree.off[l] - n) : (const G1Aff *)p_dev;
        MI_TRY(mi_launch64(ctx, k_g1_sum_level, tree.cnt[l + 1], src, (size_t)0, tree.cnt[l], lv + (tree.off[l + 1] - n), (size_t)0, tree.cnt[l + 1], 1u));
    }
    return MI_OK;
}
int32_t mi_debug_locate_points_dev(mi_ctx *ctx, const uint64_t *r_dev, const mi_g1_affine *krs_dev, const mi_g1_affine *cm_dev, const mi_g1_affine *pok_dev,
                                   const mi_fr *fold_dev, uint32_t nc, size_t n, mi_g1_affine *out_dev) {
    if (!ctx || !r_dev || !krs_dev || !out_dev || n == 0 || n > ((size_t)1 << 24) || nc > MI_PK_RAW_MAX_COMMITMENTS) return MI_EINVAL;
    if ((nc && (!cm_dev || !pok_dev)) || (nc > 1 && !fold_dev)) return MI_EINVAL;
    return mi_launch64(ctx, k_verify_locate_points, n, (const u32 *)r_dev, 4u, (const G1Aff *)krs_dev, (const G1Aff *)cm_dev, (const G1Aff *)pok_dev,
                       (const Fr *)fold_dev, nc, n, (G1Aff *)out_dev, n);
}
int32_t mi_debug_locate_colsums_dev(mi_ctx *ctx, const mi_fr *scal_dev, uint32_t ns, const mi_fr *r_dev, size_t n, uint32_t level, const uint32_t *nodes_dev,
                                    size_t m, mi_fr *sums_dev) {
    if (!ctx || (!scal_dev && ns) || !r_dev || !nodes_dev || !sums_dev || n == 0 || n > ((size_t)1 << 24) || m == 0 || m > n) return MI_EINVAL;
    if (level > LocateTree(n).L) return MI_EINVAL;
    const size_t partials = m * (ns + 1) * mi_verify_node_blocks(level, n);
    MI_TRY(mi_reserve(ctx, ctx->ws[WS_VERIFY_LOCATE], partials * sizeof(Fr)));
    return mi_verify_colsums_enqueue(ctx, (const Fr *)scal_dev, ns, (const Fr *)r_dev, n, level, nodes_dev, m, (Fr *)ctx->ws[WS_VERIFY_LOCATE].p, (Fr *)sums_dev);
}
int32_t mi_debug_set_locate_round_nodes(mi_ctx *ctx, uint32_t cap) {
    if (!ctx) return MI_EINVAL;
    ctx->locate_round_nodes = cap;
    return MI_OK;
}
}

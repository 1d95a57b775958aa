// What the verifier's files share (not part of the C-ABI): the resident key and the one structure of a batch.  mi_verify_open (argument
// checks under the body's message prefix, proof references, the VerifyStage of pairing_ops.cuh) opens it for one of FOUR bodies:
//   a verdict per proof    mi_verify_run ("verify: ") and mi_verify_run_wave ("verify wave: ") start from mi_verify_stage_pairs
//   the coefficients r_i   mi_verify_combined_run ("verify combined: ") and mi_verify_locate_run ("verify locate: ") start from
//                          mi_verify_refuse_msm_pairs, mi_verify_seed, mi_verify_flag_bs and mi_verify_put_coeffs, and share the column sums
// verify_bytes.hip decodes a batch and calls the same bodies.  Then the launches other files reuse, WsCut, mi_launch64 and small helpers.
#pragma once
#include "ctx.h"
#include "../../include/mi355x_groth16_verify.h"
#include "../../include/mi355x_groth16_verify_combined.h"
#include "../../include/mi355x_groth16_verify_locate.h"
#include "../../include/mi355x_groth16_verify_wave.h"
#include "../../include/mi355x_groth16_verify_ksum.h"
#include "pairing_ops.cuh"
#include "abi_glue.h"
#include <vector>

struct mi_vk {
    G1Aff alpha1;
    G2Aff beta2, gamma2, delta2;
    std::vector<G1Aff> k;              // host copy: K[0] and the counts
    G1Aff *k_dev = nullptr;            // K[1 .. n_k): the bases of kSum's MSM, uploaded once
    Fp12 *e_alpha_beta_dev = nullptr;  // e(alpha, beta)^s, computed once
    uint32_t nb_public = 0, n_commitments = 0;
    std::vector<mi_pedersen_vk> ped;
    // gnark's PublicAndCommitmentCommitted in CSR form (mi_vk_set_public_committed, verify_bytes.hip): offsets of n_commitments + 1
    // entries (all 0 until set: empty lists) and the indices; host memory only, a batch carries them to the device in its workspace
    std::vector<uint32_t> pc_off, pc_idx;
    // The window table of K[1..] (ksum.hip, include/mi355x_groth16_verify_ksum.h): T[j][w][d - 1] = d 2^(c w) K[1 + j], built on the first
    // verdict-per-proof call or by mi_vk_ksum_prepare, freed with the key.  c == 0: no table, and `state` (MI_KSUM_*) says why.  The stage
    // of a batch builds it through a const key: it is a cache of what the key's bases already say.
    struct Ksum {
        G1Aff *table = nullptr;
        uint32_t c = 0, state = MI_KSUM_NOT_BUILT;
        uint64_t bytes = 0, budget = MI_KSUM_DEFAULT_TABLE_BYTES;
        float build_ms = 0;
    };
    mutable Ksum ksum;
    uint32_t ksum_bases() const { return nb_public - 1 + n_commitments; }
};

// How every body starts: the checks of ctx, vk, in, n and the pointers of every proof (messages under `who`, the body's prefix;
// has_verdict = the caller's verdict pointer passes its own rule), then *st over the proofs' references.
// decode_malformed (may be null): n bytes; a non-zero byte makes proof i malformed before any of its words is read (verify_bytes.hip).
// pub_dev (may be null; the bodies pass it on): VerifyStage's device-resident public block.  With it in[i].public_inputs is not read.
int32_t mi_verify_open(mi_ctx *ctx, const char *who, const mi_vk *vk, const mi_verify_input *in, size_t n, bool has_verdict,
                       const uint8_t *decode_malformed, VerifyStage *st, const Fr *pub_dev = nullptr);
// mi_groth16_verify_batch's body (verify.hip)
int32_t mi_verify_run(mi_ctx *ctx, const mi_vk *vk, const mi_verify_input *in, size_t n, uint8_t *verdicts, const uint8_t *decode_malformed,
                      const Fr *pub_dev = nullptr);
// mi_groth16_verify_wave's body (verify_wave.hip): mi_verify_run's inputs and verdict bytes, one wave per pairing.  split_ms (may be
// null): MI_VERIFY_WAVE_SPLIT_PHASES times of the call, which then sends the Bs checks and the Miller loops as two launches
int32_t mi_verify_run_wave(mi_ctx *ctx, const mi_vk *vk, const mi_verify_input *in, size_t n, uint8_t *verdicts, const uint8_t *decode_malformed,
                           const Fr *pub_dev = nullptr, float *split_ms = nullptr);
// mi_groth16_verify_combined's body (verify_combined.hip): one verdict for the batch.  seed may be null.
int32_t mi_verify_combined_run(mi_ctx *ctx, const mi_vk *vk, const mi_verify_input *in, size_t n, const uint8_t *seed, uint8_t *verdict,
                               uint64_t *first_malformed, const uint8_t *decode_malformed, const Fr *pub_dev = nullptr);
// mi_groth16_verify_locate's body (verify_locate.hip): one verdict per proof.  seed and stats may be null.
int32_t mi_verify_locate_run(mi_ctx *ctx, const mi_vk *vk, const mi_verify_input *in, size_t n, const uint8_t *seed, uint8_t *verdicts,
                             mi_verify_locate_stats *stats, const uint8_t *decode_malformed, const Fr *pub_dev = nullptr);
// ---- the stage of the two per-proof bodies (verify.hip), all on ctx->stream: WS_VERIFY cut as scal | p | q | ml | flags | verdicts |
// extra | the stage's own regions, the scalars and the flags up, then the pairs of every proof into p, q.  With a window table on the
// key (mi_vk::ksum; the knob "verify_ksum" is 1) the host only gathers: Ar, Bs, Krs, the commitments, pok and the fold challenges of
// the batch go up in ONE copy behind the key's own points, mi_ksum_enqueue sums every row, and k_verify_assemble lays the pairs out, one
// lane per proof.  Without one it is the older loop: one mi_verify_msm per well-formed proof and verify_assemble on the host, then the
// pairs up.  `host` is the copy the upload reads: it lives until the body's last synchronise.  extra: extra_bytes of the body's own.
struct VerifyPairs {
    u32 np = 0;   // pairs per proof
    std::vector<char> host;
    G1Aff *p = nullptr;
    G2Aff *q = nullptr;
    Fp12 *ml = nullptr;
    uint8_t *flags = nullptr, *verdicts = nullptr, *extra = nullptr;
};
int32_t mi_verify_stage_pairs(mi_ctx *ctx, const mi_vk *vk, const VerifyStage &st, size_t extra_bytes, VerifyPairs *out);
// ---- kSum of a whole batch over the key's window table (ksum.hip).  mi_ksum_ready: the key has a table, building it first when no call
// has asked for one yet (under the key's budget; a key that ends without one is no error).  mi_ksum_scratch_bytes: what mi_ksum_enqueue
// needs at `scratch` for n rows (partials | sums | running products).  mi_ksum_enqueue: out_dev[i] = sum_j scal_dev[i ns + j] K[1 + j],
// affine, infinity where skip_dev[i] != 0 (skip_dev may be null); three launches whatever n is, counted into *launches (may be null).
// Proofs from which the stage of a batch takes the table; below, the older loop.  profiles/verify.txt, both stages alternating: at n = 1
// the table is not faster on either body (wave body 5.20 ms against 4.96, 5.90 against 5.57 with 4096 inputs: three launches and a
// gather against one MSM), at n = 8 it is on the wave body (5.76 against 8.20) and no slower on the one-lane body; not measured in between
#define MI_VERIFY_KSUM_MIN_BATCH 8
static_assert(MI_VERIFY_KSUM_MIN_BATCH == 8, "mi_ctx::verify_ksum_min_batch starts from this value (ctx.h)");
int32_t mi_ksum_ready(mi_ctx *ctx, const mi_vk *vk, bool *ready);
size_t mi_ksum_scratch_bytes(const mi_vk *vk, size_t n);
int32_t mi_ksum_enqueue(mi_ctx *ctx, const mi_vk *vk, const Fr *scal_dev, const uint8_t *skip_dev, size_t n, G1Aff *out_dev, char *scratch, uint64_t *launches);
// ---- the front of the two coefficient bodies (verify_combined.hip), in the order they call it.  The refusal of n * n_commitments above
// MI_MSM_MAX_PAIRS under msg, the body's own text, before mi_verify_open and under its first checks (args_ok: in and the verdict pointer)
int32_t mi_verify_refuse_msm_pairs(mi_ctx *ctx, const mi_vk *vk, bool args_ok, size_t n, const char *msg);
// seed stays, or becomes own filled with 32 bytes of the operating system's (MI_ENODEV under `who`)
int32_t mi_verify_seed(mi_ctx *ctx, const char *who, const uint8_t *&seed, uint8_t own[32]);
// Malformed first: Q[i] = Bs of proof i where the host's checks passed, else infinity (Q: n host entries); Q and the flags up to the
// body's regions, k_verify_g2_check, the flags back, synchronise, st.merge: st.flags and st.first_flagged are final on return
int32_t mi_verify_flag_bs(mi_ctx *ctx, VerifyStage &st, G2Aff *Q, G2Aff *q_dev, uint8_t *flags_dev);
// The inputs of the combination: r_i = combine_coefficient(seed, n, i), the fold challenges (more than one commitment), Ar (p), Krs, pok
// and the commitments, [k][i] (cm_by_column) or [i][k]; a proof st flags keeps coefficient 0 and infinities.  Then the uploads, the
// scalar matrix first, to the offsets `at` in the body's workspace ws.  *h: the host copies, alive until the body's last synchronise.
struct VerifyCoeffs {
    std::vector<Fr> r, fold;
    std::vector<G1Aff> p, krs, pok, cm;
};
struct VerifyCoeffsAt { size_t scal, r, fold, krs, pok, cm, p; };
int32_t mi_verify_put_coeffs(mi_ctx *ctx, const VerifyStage &st, const mi_verify_input *in, const uint8_t *seed, bool cm_by_column, VerifyCoeffs *h,
                             char *ws, const VerifyCoeffsAt &at);
// ---- the column sums of both (verify_locate.hip): sums[t (ns + 1) + j] = sum of r_i scal[i ns + j] over the proofs i of node (level,
// nodes_dev[t]) of the tree over n proofs, column ns = sum of r_i; nodes_dev == null: node t is t.  One launch over (node, column,
// block) into partial (m (ns + 1) mi_verify_node_blocks(level, n) records), one reduce.  rc (may be null) with rrep, fold (null: c_i =
// 1) and nc: the column-ns blocks also write rc[k n + i] = r_i c_i^k (Montgomery) and rrep[k n + i] = r_i, k < nc.
u32 mi_verify_node_blocks(u32 level, size_t n);
int32_t mi_verify_colsums_enqueue(mi_ctx *ctx, const Fr *scal, u32 ns, const Fr *r, size_t n, u32 level, const u32 *nodes_dev, size_t m, Fr *partial, Fr *sums,
                                  const Fr *fold = nullptr, u32 nc = 0, Fr *rc = nullptr, Fr *rrep = nullptr);
// What mi_vk_load and mi_vk_load_stream (vkfile.hip) share: the resident key over a descriptor whose conditions the caller has checked.
// k_dev_adopt (may be null): K[1 .. n_k) already on the device in an allocation of (n_k - 1) * 64 + 64 bytes, which the key takes
// (and has freed when the call fails); without it K is uploaded from d->k.
int32_t mi_vk_build(mi_ctx *ctx, const mi_vk_desc *d, G1Aff *k_dev_adopt, mi_vk **out);
// verify.hip's kernels for the other translation units, enqueued on ctx->stream: Miller values of n pairs on the device (then, with
// final_exp, f^d' in place), f^d' in place alone, and flags[i] = 1 where q[i * stride] is not a point of the r-torsion of the twist
// (else flags[i] stays)
int32_t mi_final_exp_enqueue(mi_ctx *ctx, Fp12 *io_dev, size_t n);
int32_t mi_pairing_enqueue(mi_ctx *ctx, const G1Aff *p_dev, const G2Aff *q_dev, size_t n, Fp12 *gt_dev, bool final_exp);
int32_t mi_verify_g2_check_enqueue(mi_ctx *ctx, const G2Aff *q_dev, u32 stride, uint8_t *flags_dev, size_t n);
// verify_combined.hip's kernels the same way: one level of the Fp12 product tree (out[j] = x[8 j] x[8 j + 1] ..., m_out = ceil(m / 8)), and
// out[i] = k_i p[i] with k_i the four words at k + i * stride
int32_t mi_fp12_product_level_enqueue(mi_ctx *ctx, const Fp12 *x_dev, size_t m, Fp12 *out_dev, size_t m_out);
int32_t mi_g1_scale128_enqueue(mi_ctx *ctx, const G1Aff *p_dev, const u32 *k_dev, u32 stride, G1Aff *out_dev, size_t n);
// mi_msm_g1_dev (msm.hip) over bases and scalars on the device; *out affine, (0, 0) for infinity
int32_t mi_verify_msm(mi_ctx *ctx, const void *bases_dev, const void *scalars_dev, size_t count, uint32_t msm_flags, G1Aff *out);

// The layout of a workspace: regions in the order they are taken, each at a multiple of 256 bytes; total is what to reserve
struct WsCut {
    size_t total = 0;
    size_t take(size_t bytes) { const size_t at = total; total += (bytes + 255) & ~(size_t)255; return at; }
};
// k over `lanes` lanes, 64 per workgroup, on ctx->stream, and the one checked hipGetLastError of a launch; no lane, no launch
template <class K, class... A> int32_t mi_launch64(mi_ctx *ctx, K k, size_t lanes, A... args) {
    if (!lanes) return MI_OK;
    hipLaunchKernelGGL(k, dim3(mi_blocks_of(lanes, 64)), dim3(64), 0, ctx->stream, args...);
    MI_CHECK_HIP(ctx, hipGetLastError());
    return MI_OK;
}
// A stage's scalar matrix (n x ns, row-major: public_inputs | commitment_values) at a device address, enqueued on ctx->stream.  Without
// a device-resident public block it is one upload of st.scal.  With one, the public columns are a strided device-to-device copy of the
// block, the commitment-value columns a strided upload of st.scal, and the row of every proof st.flags marks now is zeroed, as the
// host's rows of such proofs are.
inline int32_t mi_verify_put_scalars(mi_ctx *ctx, const VerifyStage &st, Fr *dst_dev) {
    const size_t n = st.n(), row = (size_t)st.ns * sizeof(Fr);
    if (!n || !st.ns) return MI_OK;
    if (!st.pub_dev) {
        MI_CHECK_HIP(ctx, hipMemcpyAsync(dst_dev, st.scal.data(), st.scal.size() * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
        return MI_OK;
    }
    const size_t pub = (size_t)st.n_pub * sizeof(Fr), cv = (size_t)st.nc * sizeof(Fr);
    if (pub) MI_CHECK_HIP(ctx, hipMemcpy2DAsync(dst_dev, row, st.pub_dev, pub, pub, n, hipMemcpyDeviceToDevice, ctx->stream));
    if (cv) MI_CHECK_HIP(ctx, hipMemcpy2DAsync(dst_dev + st.n_pub, row, st.scal.data(), cv, cv, n, hipMemcpyHostToDevice, ctx->stream));
    for (size_t i = 0; i < n;) {   // one fill per RUN of flagged rows: a batch that is malformed throughout costs one enqueue
        size_t e = i;
        while (e < n && st.flags[e]) e++;
        if (e > i) MI_CHECK_HIP(ctx, hipMemsetAsync(dst_dev + i * st.ns, 0, (e - i) * row, ctx->stream));
        i = e + 1;
    }
    return MI_OK;
}
// bytes from the host to a device address on ctx->stream; no byte, no call
inline int32_t mi_verify_upload(mi_ctx *ctx, void *dst_dev, const void *src, size_t bytes) {
    if (bytes) MI_CHECK_HIP(ctx, hipMemcpyAsync(dst_dev, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return MI_OK;
}

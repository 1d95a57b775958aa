// What verify.hip, verify_bytes.hip, verify_combined.hip, verify_locate.hip and verify_wave.hip share (not part of the C-ABI): the resident key, the opening of a batch
// (mi_verify_open: argument checks, proof references, the VerifyStage of pairing_ops.cuh), the four bodies that judge it, the launches of
// verify.hip's kernels that the combined body reuses, and three helpers: WsCut (a workspace's layout), mi_launch64, mi_verify_msm.
#pragma once
#include "ctx.h"
#include "../../include/mi355x_groth16_verify.h"
#include "../../include/mi355x_groth16_verify_combined.h"
#include "../../include/mi355x_groth16_verify_locate.h"
#include "../../include/mi355x_groth16_verify_wave.h"
#include "pairing_ops.cuh"
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
};

// How both bodies start: the checks of ctx, vk, in, n and the pointers of every proof (messages under `who`, "verify: " or
// "verify combined: "; has_verdict = the caller's verdict pointer passes its own rule), then *st over the proofs' references.
// decode_malformed (may be null): n bytes; a non-zero byte makes proof i malformed before any of its words is read (verify_bytes.hip).
// pub_dev (may be null; the three bodies pass it on): VerifyStage's device-resident public block.  With it in[i].public_inputs is not read.
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

// What verify.hip, verify_bytes.hip and verify_combined.hip share (not part of the C-ABI): the resident key, the body that judges a batch
// proof by proof, the body that judges it with one verdict, and the launches of verify.hip's kernels that the latter reuses.
#pragma once
#include "ctx.h"
#include "../../include/mi355x_groth16_verify.h"
#include "../../include/mi355x_groth16_verify_combined.h"
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

// mi_groth16_verify_batch's body (verify.hip).  decode_malformed (may be null): n bytes; a non-zero byte makes proof i malformed before
// any of its words is read -- what mi_groth16_verify_bytes_batch knows from decoding.
int32_t mi_verify_run(mi_ctx *ctx, const mi_vk *vk, const mi_verify_input *in, size_t n, uint8_t *verdicts, const uint8_t *decode_malformed);

// mi_groth16_verify_combined's body (verify_combined.hip): one verdict for the batch; decode_malformed as above.  seed may be null.
int32_t mi_verify_combined_run(mi_ctx *ctx, const mi_vk *vk, const mi_verify_input *in, size_t n, const uint8_t *seed, uint8_t *verdict,
                               uint64_t *first_malformed, const uint8_t *decode_malformed);
// verify.hip's kernels for the other translation units, enqueued on ctx->stream: Miller values of n pairs on the device (then, with
// final_exp, f^d' in place), f^d' in place alone, and flags[i] = 1 where q[i * stride] is not a point of the r-torsion of the twist
// (else flags[i] stays)
int32_t mi_final_exp_enqueue(mi_ctx *ctx, Fp12 *io_dev, size_t n);
int32_t mi_pairing_enqueue(mi_ctx *ctx, const G1Aff *p_dev, const G2Aff *q_dev, size_t n, Fp12 *gt_dev, bool final_exp);
int32_t mi_verify_g2_check_enqueue(mi_ctx *ctx, const G2Aff *q_dev, u32 stride, uint8_t *flags_dev, size_t n);

inline unsigned grid64(size_t n) { return (unsigned)((n + 63) / 64); }
inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

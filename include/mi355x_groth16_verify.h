/* mi355x_groth16_verify.h -- groth16.Verify on the device (BN254): the pairing check behind a device-resident verifying key.
 *
 * Replaces the call
 *     err = groth16.Verify(proof, vk, publicWitness)
 * at mt.go:497 of the reference, the last of the Setup / Prove / Verify sequence (mi355x_groth16_setup.h, mi355x_groth16.h).  A proof is
 * accepted when both equations hold:
 *     e(Ar, Bs) = e(alpha, beta) e(kSum, gamma) e(Krs, delta)
 *         kSum = K[0] + sum_i public_inputs[i] K[1 + i] + sum_k commitment_values[k] K[nb_public + k] + sum_k C_k
 *     prod_k e(c^k C_k, GSigmaNeg_k) e(pok, G) = 1                    (BSB22 commitments C_k, c = fold_challenge; only with commitments)
 * with e the optimal ate pairing of BN254 (csrc/pairing.cuh: Miller loop over 6 x0 + 2, final exponentiation to the exact exponent that
 * file states).  kSum's scalar part runs through the library's G1 MSM over the key's K points, which are uploaded once, at mi_vk_load.
 *
 * Same library and conventions as mi355x_groth16.h / mi355x_groth16_setup.h: int32 status codes, Montgomery mi_fr / mi_fp, HOST
 * pointers, mi_last_error; the library keeps no caller pointer after return.  The workspace belongs to the context and only grows.
 *
 * THESE ENTRY POINTS TAKE THE HASHES AS INPUTS: commitment_values[k] -- gnark's SHA-256 hash-to-field of commitment k (and of the
 * public committed values) -- and fold_challenge are passed in.  mi355x_groth16_verify_bytes.h computes them (and decodes the proof's
 * bytes) on the device and lands here; mi_hash_to_field of that header is the same hash on the host for a caller of this one.
 *
 * NOT PINNED TO gnark's SOURCE, like the Pedersen bases of mi_groth16_setup: the verifier is defined by the two equations above and by
 * mi_pedersen_vk_make below, which match the keys mi_groth16_setup makes.  Before relying on it against keys or proofs from gnark itself,
 * verify one gnark proof with it.
 */
#ifndef MI355X_GROTH16_VERIFY_H
#define MI355X_GROTH16_VERIFY_H
#include "mi355x_groth16.h"
#include "mi355x_groth16_setup.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi_vk mi_vk;

/* pedersen.VerifyingKey of one commitment: G and GSigmaNeg = -sigma G on the twist. */
typedef struct mi_pedersen_vk { mi_g2_affine g, g_sigma_neg; } mi_pedersen_vk;

typedef struct mi_vk_desc {
    mi_g1_affine alpha1;
    mi_g2_affine beta2, gamma2, delta2;
    const mi_g1_affine *k;           /* vk.G1.K, as mi_vk_out.k */
    uint64_t n_k;                    /* must equal nb_public + n_commitments */
    uint32_t nb_public;              /* includes the ONE wire, as mi_pk_desc: >= 1 */
    uint32_t n_commitments;          /* 0 .. MI_PK_RAW_MAX_COMMITMENTS */
    const mi_pedersen_vk *ped;       /* n_commitments entries; may be NULL when n_commitments == 0 */
} mi_vk_desc;

/* Uploads the key and computes e(alpha, beta) once.  MI_EINVAL, decided on the host before any allocation: a null pointer, nb_public
 * of 0, n_k != nb_public + n_commitments, n_commitments above MI_PK_RAW_MAX_COMMITMENTS, a coordinate that is not reduced (see ONE
 * ENCODING below), a point off its curve, a G2 point outside the r-torsion of the twist, gamma2 or delta2 at infinity, or Pedersen keys
 * that do not all share one G (gnark's BatchVerifyMultiVk condition: one pairing with G serves every commitment).  mi_last_error names
 * the field.  K[i] at infinity is a valid key (gnark emits it for a public wire no constraint uses). */
int32_t mi_vk_load(mi_ctx *ctx, const mi_vk_desc *desc, mi_vk **out);
int32_t mi_vk_free(mi_ctx *ctx, mi_vk *vk);

/* The Pedersen verifying keys that match the keys of mi_groth16_setup (BasisExpSigma = sigma Basis): out[k].g = the G2 generator,
 * out[k].g_sigma_neg = (r - sigma[k]) g.  sigma: n Montgomery scalars, the trapdoor's. */
int32_t mi_pedersen_vk_make(mi_ctx *ctx, const mi_fr *sigma, uint32_t n, mi_pedersen_vk *out);

typedef struct mi_verify_input {
    mi_proof_out proof;
    const mi_g1_affine *commitments;        /* n_commitments points C_k (may be NULL when the key has none) */
    const mi_g1_affine *pok;                /* ONE point: the folded proof of knowledge, as pok_out of mi_prover_submit_bsb22 (idem) */
    const mi_fr *public_inputs;             /* nb_public - 1 values: the ONE wire is implied (may be NULL when nb_public == 1) */
    const mi_fr *commitment_values;         /* n_commitments values: the hash-to-field of each commitment, computed by the caller.
                                               Value k multiplies K[nb_public + k]: the order of the key's commitment-wire points, which
                                               mi_groth16_setup emits by ascending wire index.  That is the order of commitments[] when
                                               the commitment wires ascend with k, as gnark's do; otherwise order the values as K is */
    const mi_fr *fold_challenge;            /* as the challenge of mi_prover_submit_bsb22; may be NULL when n_commitments <= 1 */
} mi_verify_input;

/* ONE ENCODING.  An mi_fp / mi_fr is four Montgomery words; read as one 256-bit integer they must lie BELOW the modulus (p for a
 * coordinate, r for a scalar).  The arithmetic would take x + p for x (2p < 2^256), so a word string that is not reduced would be a
 * second encoding of the same proof -- for public_inputs it is the public-input aliasing of pairing verifiers, and (p, p) would be a
 * second infinity.  The verifier refuses them:
 *   - mi_groth16_verify[_batch]: any coordinate of proof, commitments or pok not below p, or any of public_inputs, commitment_values,
 *     fold_challenge not below r, makes the verdict MI_VERIFY_MALFORMED.  (fold_challenge is read, and checked, only with more than one
 *     commitment.)  This is decided on the host, before anything of that proof reaches the MSM or a pairing.
 *   - mi_vk_load: MI_EINVAL for any such coordinate of the descriptor; mi_last_error names the field. */

/* verdicts; the checks run in the order 3, 1, 2 and the first that fails names the verdict */
#define MI_VERIFY_OK 0          /* both equations hold */
#define MI_VERIFY_PAIRING 1     /* e(Ar, Bs) != e(alpha, beta) e(kSum, gamma) e(Krs, delta) */
#define MI_VERIFY_PEDERSEN 2    /* prod_k e(c^k C_k, GSigmaNeg_k) e(pok, G) != 1 */
#define MI_VERIFY_MALFORMED 3   /* a coordinate or scalar that is not reduced (ONE ENCODING); Ar, Krs, pok or a commitment off the
                                   curve; Bs off the twist or outside its r-torsion */

/* Both return MI_OK whenever a verdict was reached: a rejected proof is a verdict, not an error.  MI_EINVAL (null pointers, a missing
 * array the key's counts call for) is decided on the host before any device work.  A batch judges every proof on its own: verdicts[i] is exactly
 * what mi_groth16_verify says for in[i].  (ONE verdict for a whole batch, by a random linear combination of the proofs' equations and at
 * a fraction of the cost: mi355x_groth16_verify_combined.h.) */
int32_t mi_groth16_verify(mi_ctx *ctx, const mi_vk *vk, const mi_verify_input *in, uint8_t *verdict);
int32_t mi_groth16_verify_batch(mi_ctx *ctx, const mi_vk *vk, const mi_verify_input *in, size_t n, uint8_t *verdicts);

#ifdef __cplusplus
}
#endif
#endif

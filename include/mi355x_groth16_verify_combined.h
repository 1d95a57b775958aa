/* mi355x_groth16_verify_combined.h -- a batch of Groth16 proofs under one key judged by ONE pairing product: the random linear
 * combination of the per-proof equations of mi355x_groth16_verify.h.
 *
 * mi_groth16_verify_batch judges every proof on its own: 3 + n_commitments + 1 Miller loops, two final exponentiations and one
 * synchronous G1 MSM per proof.  Both equations are linear in the exponent, so with coefficients r_0 .. r_(n-1) and S = sum_i r_i mod r
 * the whole batch is the two checks
 *     prod_i e(r_i Ar_i, Bs_i) e(-S alpha, beta) e(-(S K[0] + sum_j (sum_i r_i s_ij) K[1 + j] + sum_i r_i sum_k C_ik), gamma)
 *            e(-sum_i r_i Krs_i, delta) = 1                                                                       (the Groth16 equation)
 *     e(sum_i r_i pok_i, G) prod_k e(sum_i (r_i c_i^k) C_ik, GSigmaNeg_k) = 1                   (the Pedersen equation; with commitments)
 * where s_ij are proof i's public_inputs followed by its commitment_values, c_i is its fold_challenge and c_i = 1 when n_commitments <= 1.
 * Per batch that is n + 3 (+ n_commitments + 1) Miller loops, two final exponentiations and 2 MSM calls without commitments (1 when the
 * key has no public input either), 4 + n_commitments with them (at most 20), whatever n is; per proof the new work is one 128-bit G1
 * scalar multiplication.  This is the standard batched verifier, and for the Pedersen half what gnark's BatchVerifyMultiVk does.
 *
 * COEFFICIENTS.  r_i is the little-endian integer of the first 16 bytes of
 *     SHA-256("mi355x-g16-combine" | seed (32 bytes) | le64(n) | le64(i))
 * computed on the host.  seed == NULL: the library draws the 32 bytes from the operating system (getrandom); if that fails the call
 * returns an error and no verdict (RETURN VALUES).
 * THE SOUNDNESS CLAIM BELOW HOLDS ONLY FOR A SEED THE MAKER OF THE PROOFS CANNOT PREDICT: whoever knows the seed before choosing the
 * proofs knows every r_i and can make defects cancel.  A fixed seed is for tests and for reproducing a verdict, never for judging proofs
 * from someone else.
 *
 * GUARANTEES.
 *   - A batch in which mi_groth16_verify accepts every proof is always accepted (verdict 0), for every seed.
 *   - A batch with at least one proof that mi_groth16_verify rejects with 1 or 2 is accepted with probability at most about 2^-128 over
 *     the seed: after the checks of verdict 3 every point lies in a group of prime order r, so each equation reads sum_i r_i d_i = 0
 *     mod r with d_i proof i's defect in the exponent, and a non-zero d_i leaves one value of r_i (of 2^128) that satisfies it.
 *   - Verdicts 1 and 2 do not say WHICH proof is at fault; mi_groth16_verify_batch does.  mi_groth16_verify_locate
 *     (mi355x_groth16_verify_locate.h) names them by running this test on a tree of subsets of the batch.
 *
 * VERDICTS (MI_VERIFY_* of mi355x_groth16_verify.h), one for the whole batch, decided in the order 3, 1, 2:
 *   3  MI_VERIFY_MALFORMED  some proof is malformed by the rules of mi_groth16_verify (a word that is not reduced, a G1 point off the
 *                           curve, Bs off the twist or outside its r-torsion; in the bytes twin also a count or a point that does not
 *                           decode).  *first_malformed = the lowest such index.  Malformedness is decided FIRST, for the whole batch, by
 *                           the host's checks and the device's Bs check; when it is found nothing else of the batch runs, and no word of
 *                           a malformed proof reaches an MSM, the group law or a Miller loop.
 *   1  MI_VERIFY_PAIRING    the combined Groth16 equation fails
 *   2  MI_VERIFY_PEDERSEN   it holds and the combined Pedersen equation fails
 *   0  MI_VERIFY_OK         neither
 * *first_malformed = n for every verdict but 3.
 *
 * RETURN VALUES.  MI_OK whenever a verdict was reached; n == 0 gives MI_OK and verdict 0.  MI_EINVAL, before any device work: ctx, vk or
 * verdict null, in null with n > 0, n above 2^24, n * n_commitments above MI_MSM_MAX_PAIRS, or a missing array the key's counts call
 * for (as mi_groth16_verify_batch).  MI_ENODEV when seed == NULL and the operating system gives no randomness: no verdict is written.
 * Same library and conventions otherwise: HOST pointers, mi_last_error, a workspace that belongs to the context and only grows.
 */
#ifndef MI355X_GROTH16_VERIFY_COMBINED_H
#define MI355X_GROTH16_VERIFY_COMBINED_H
#include "mi355x_groth16_verify.h"
#include "mi355x_groth16_verify_bytes.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ONE verdict for the whole batch. */
int32_t mi_groth16_verify_combined(mi_ctx *ctx, const mi_vk *vk, const mi_verify_input *in, size_t n, const uint8_t seed[32] /* may be NULL */,
                                   uint8_t *verdict, uint64_t *first_malformed /* may be NULL */);
/* The same from the bytes of the proofs: decodes and hashes exactly as mi_groth16_verify_bytes_batch does (its MI_EINVAL cases too),
 * then the body above over the decoded proofs. */
int32_t mi_groth16_verify_bytes_combined(mi_ctx *ctx, const mi_vk *vk, const mi_verify_bytes_input *in, size_t n, const uint8_t seed[32] /* may be NULL */,
                                         uint8_t *verdict, uint64_t *first_malformed /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif

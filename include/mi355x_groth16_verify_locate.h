/* mi355x_groth16_verify_locate.h -- a batch of Groth16 proofs under one key, one verdict PER PROOF, at the price of the combined test
 * when the batch is good: the random linear combination of mi355x_groth16_verify_combined.h run on a tree of subsets of the batch.
 *
 * mi_groth16_verify_batch names every rejected proof and pays a full verification per proof.  mi_groth16_verify_combined pays one
 * pairing product for the batch and gives one verdict.  Both of its equations are linear in the exponent, so the same test judges any
 * SUBSET of the batch, and what is expensive in it is per proof and shared by every subset: the Miller values ML(r_i Ar_i, Bs_i) and the
 * scaled points r_i Krs_i, r_i sum_k C_ik, r_i pok_i, (r_i c_i^k) C_ik.  This call computes them once, keeps their products and sums over
 * the nodes of a tree of fan-in 8 (node (l, j) covers the proofs [j 8^l, min(n, (j + 1) 8^l)); the root covers the batch), tests the
 * root, descends only into nodes that fail, and hands the proofs still under suspicion to the per-proof body of mi_groth16_verify_batch.
 * A node's test is the combined test restricted to the well-formed proofs of the node; the root's is mi_groth16_verify_combined over the
 * well-formed proofs of the batch.
 *
 * verdicts[i] is what mi_groth16_verify_batch would write for proof i (MI_VERIFY_* of mi355x_groth16_verify.h), up to the soundness
 * claim under GUARANTEES.
 *
 * MALFORMED PROOFS are decided first, per proof, by the rules of mi_groth16_verify (in the bytes twin also a count or a point that does
 * not decode).  Each gets verdict 3 and takes no further part: no word of a malformed proof reaches an MSM, the group law or a Miller
 * loop.  Unlike in mi_groth16_verify_combined, malformed proofs do not end the batch: the others are still judged.
 *
 * COEFFICIENTS.  They are the combined verifier's, unchanged: r_i is the little-endian integer of the first 16 bytes of
 *     SHA-256("mi355x-g16-combine" | seed (32 bytes) | le64(n) | le64(i))
 * with the FULL n of the batch and the ORIGINAL index i, whichever node the proof is tested in; a malformed proof's coefficient counts
 * as 0.  seed == NULL: the library draws the 32 bytes from the operating system (getrandom); if that fails the call returns MI_ENODEV
 * and writes nothing.
 * THE SOUNDNESS CLAIM BELOW HOLDS ONLY FOR A SEED THE MAKER OF THE PROOFS CANNOT PREDICT: whoever knows the seed before choosing the
 * proofs knows every r_i and can make defects cancel inside a node.  A fixed seed is for tests and for reproducing a verdict, never for
 * judging proofs from someone else.
 *
 * GUARANTEES.
 *   - A proof reported 1 or 2 is rejected with that verdict by mi_groth16_verify, with certainty: such verdicts come only from the
 *     per-proof body, never from a node test.  A node test only ever decides "accepted".
 *   - A proof reported 0 that mi_groth16_verify would reject has slipped through a node test whose weighted defects summed to zero:
 *     probability about 2^-128 per node test, and a union over at most 8n/7 nodes, for a seed the maker of the proofs cannot predict.
 *   - A batch in which mi_groth16_verify accepts every well-formed proof costs ONE node test, the root's.
 *
 * THE DESCENT.  A round is a set of nodes on one level, tested in one batched pass.  Round 0 is the root.  From the failing nodes F of a
 * round (on level l, with u well-formed proofs under them) the next round takes the lowest level l' with 1 <= l' < l that has at most
 * MI_LOCATE_ROUND_NODES (64, chosen by measurement: DESIGN.md 4d) nodes under F, or l' = l - 1 when there is none; it stops when
 * l == 1 or when u <= 2 x that number of nodes (a round would buy less than a halving), and the u proofs go to the per-proof body in
 * one call.  Should every child of a failing node pass, all of them stay under suspicion.
 *
 * mi_verify_locate_stats (may be NULL) says what the call did.
 *
 * RETURN VALUES.  MI_OK whenever the verdicts were written; n == 0 gives MI_OK and zeroed stats.  MI_EINVAL, before any device work and
 * with nothing written: ctx or vk null, in or verdicts null with n > 0, n above 2^24, n * n_commitments above MI_MSM_MAX_PAIRS, or a
 * missing array the key's counts call for (the refusals of mi_groth16_verify_combined).  MI_ENODEV when seed == NULL and the operating
 * system gives no randomness.  Same library and conventions otherwise: HOST pointers, mi_last_error, a workspace that belongs to the
 * context and only grows.
 */
#ifndef MI355X_GROTH16_VERIFY_LOCATE_H
#define MI355X_GROTH16_VERIFY_LOCATE_H
#include "mi355x_groth16_verify_combined.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    uint32_t rounds;         /* node-test rounds run, the root's included; 0 when nothing was left to test */
    uint64_t nodes_tested;   /* subsets judged by a combined test, the root included */
    uint64_t judged_alone;   /* proofs handed to the per-proof body */
    uint64_t malformed, rejected;   /* proofs with verdict 3; with verdict 1 or 2 */
} mi_verify_locate_stats;

/* One verdict per proof: verdicts[0 .. n). */
int32_t mi_groth16_verify_locate(mi_ctx *ctx, const mi_vk *vk, const mi_verify_input *in, size_t n, const uint8_t seed[32] /* may be NULL */,
                                 uint8_t *verdicts /* n bytes */, mi_verify_locate_stats *stats /* may be NULL */);
/* The same from the bytes of the proofs: decodes and hashes exactly as mi_groth16_verify_bytes_batch does (its MI_EINVAL cases too),
 * then the body above over the decoded proofs; a proof that does not decode gets 3. */
int32_t mi_groth16_verify_bytes_locate(mi_ctx *ctx, const mi_vk *vk, const mi_verify_bytes_input *in, size_t n, const uint8_t seed[32] /* may be NULL */,
                                       uint8_t *verdicts /* n bytes */, mi_verify_locate_stats *stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif

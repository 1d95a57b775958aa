/* mi355x_groth16_verify_wave.h -- groth16.Verify on the device for ONE proof, or a few: the verifier of mi355x_groth16_verify.h with one
 * wave of 64 lanes per pairing instead of one lane.
 *
 * WHAT THE CALLS ARE FOR.  mi_groth16_verify[_batch] runs every Miller loop, every final exponentiation and the check of Bs as a chain
 * of tens of thousands of dependent field products in ONE lane: a batch of thousands fills the device, one proof waits for the chain.
 * The calls below spread the 36 Fp2 products of every Fp12 product (18 of a line product, 9 of a cyclotomic squaring) and the products
 * of every point step over the lanes of a wave, run one wave per (proof, pair) and one per (proof, equation), and check Bs by the 63-bit
 * endomorphism test the key loaders use, beside the Miller waves.  They are the calls for the single proof the reference verifies
 * (mt.go:497) and for small batches.
 *
 * THE VERDICTS ARE THOSE OF mi_groth16_verify_batch / mi_groth16_verify_bytes_batch, byte for byte: the same host half decides what is
 * malformed (ONE ENCODING and the curve checks of mi355x_groth16_verify.h; no word of a malformed proof reaches an MSM, the group law
 * or a Miller loop), the same two equations are compared after the same final exponentiation, and every field element here is fully
 * reduced, so another order of evaluation gives the same words.  Bs outside the r-torsion of the twist is malformed, as there.
 *
 * WHEN TO USE WHICH.  Measured against mi_groth16_verify_batch on the same inputs, the two calls alternating on one context
 * (profiles/verify.txt, a key with one commitment: 5 pairs per proof, whole calls, medians): n = 1: 5.2 ms against 40.6 ms; n = 8: 8.1
 * against 39.0; n = 64: 30.0 against 59.7; n = 512: 209.5 against 235.5; n = 4096: 1644.6 against 1620.1 -- the batch call takes the
 * lead somewhere between n = 512 and n = 4096 (not measured in between).  Both calls run one synchronous MSM per proof from the host;
 * at n = 1 that host stage is 0.39 ms of the 5.2, so by that figure it is most of either call from n = 64 on.  So: these calls for one
 * proof up to a few hundred.  (Those figures are from before mi355x_groth16_verify_ksum.h, which took that MSM out of both calls for
 * batches of 8 proofs and more; in the later block of profiles/verify.txt, same key: n = 64: 5.9 ms against 35.4; n = 512: 10.3
 * against 36.1; n = 4096: 64.5 against 40.4 -- the same advice, at other prices.)
 * Above that, mi_groth16_verify_batch names every rejected proof at a lower price per proof, mi_groth16_verify_combined
 * (mi355x_groth16_verify_combined.h) gives one verdict for the batch at a fraction of it, and mi_groth16_verify_locate
 * (mi355x_groth16_verify_locate.h) one verdict per proof at the combined test's price when the batch is good: they remain the tools for
 * large batches.
 *
 * RETURN VALUES.  MI_OK whenever the verdicts were written (MI_VERIFY_* of mi355x_groth16_verify.h); n == 0 gives MI_OK.  MI_EINVAL,
 * before any device work and with nothing written: the cases of mi_groth16_verify_batch and mi_groth16_verify_bytes_batch, unchanged
 * (null pointers, n above 2^24, a missing array the key's counts call for, a proof_len that is not the key's); mi_last_error says which,
 * under the prefix "verify wave: " (the decoding of the bytes twin keeps "verify bytes: ").  Same library and conventions otherwise: HOST
 * pointers, a workspace that belongs to the context and only grows -- the one mi_groth16_verify_batch uses, so the two may alternate on
 * one context.
 */
#ifndef MI355X_GROTH16_VERIFY_WAVE_H
#define MI355X_GROTH16_VERIFY_WAVE_H
#include "mi355x_groth16_verify.h"
#include "mi355x_groth16_verify_bytes.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One verdict per proof: verdicts[0 .. n), exactly mi_groth16_verify_batch's. */
int32_t mi_groth16_verify_wave(mi_ctx *ctx, const mi_vk *vk, const mi_verify_input *in, size_t n, uint8_t *verdicts /* n bytes */);
/* The same from the bytes of the proofs: decodes and hashes exactly as mi_groth16_verify_bytes_batch does (its MI_EINVAL cases too),
 * then the body above over the decoded proofs; a proof that does not decode gets 3. */
int32_t mi_groth16_verify_bytes_wave(mi_ctx *ctx, const mi_vk *vk, const mi_verify_bytes_input *in, size_t n, uint8_t *verdicts /* n bytes */);

#ifdef __cplusplus
}
#endif
#endif

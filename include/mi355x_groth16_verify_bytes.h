/* mi355x_groth16_verify_bytes.h -- groth16.Verify from the bytes of a proof: decode and hash on the device, then the pairing check of
 * mi355x_groth16_verify.h.
 *
 * mi_groth16_verify[_batch] takes a proof that someone has already taken apart: affine Montgomery points, and the two BSB22 hashes
 * (commitment_values, fold_challenge) computed by the caller.  The entry points here take what Proof.WriteTo wrote -- what
 * mi_proof_write of mi355x_groth16.h emits -- and do that work themselves:
 *     Ar (32) | Bs (64) | Krs (32) | u32 big-endian count | count x 32 commitments | pok (32)              164 + 32 count bytes
 * One lane per point decompresses it (an Fp or Fp2 square root by fixed exponentiations, csrc/decode_ops.cuh), one lane per proof
 * computes the hashes (SHA-256, expand_message_xmd, csrc/sha256_h2f.cuh), and the decoded proof goes through the same body as
 * mi_groth16_verify_batch.  THE CONTRACT: the verdict equals what mi_groth16_verify says for the decoded proof with these hashes.
 *
 * POINT ENCODING (gnark-crypto's, the inverse of mi_g1_compress / mi_g2_compress).  X is 32 bytes big-endian canonical (G2: 64 bytes,
 * X.A1 then X.A0); the top two bits of byte 0 are flags: 10 = y is the smaller of (y, p - y), 11 = the larger, 01 = infinity, 00 =
 * uncompressed.  "Larger" on G2 is decided on y.A1, or on y.A0 when y.A1 = 0.  ONE ENCODING, as everywhere in the verifier: a string is
 * MALFORMED when X (either component on G2) is not below p, when the flag is 00, when the flag is 01 and any other bit is set, or when X
 * has no y on the curve.
 *
 * HASHES, as gnark's verify.go states them (go/mi355x/verify.go spells the same thing with gnark-crypto's calls):
 *     commitment_values[i] = H_"bsb22-commitment"(uncompressed C_i | full[j - 1] as 32 bytes big-endian canonical, j in committed_i)
 *     full                 = public_inputs | commitment_values[0] | ... | commitment_values[i - 1]
 *     fold_challenge       = H_"G16-BSB22"(commitment_values[0] | ... as 32 bytes big-endian canonical)
 * H_dst(msg) = expand_message_xmd(SHA-256, msg, dst, 48) of RFC 9380 5.3.1, read big-endian, reduced mod r.  An uncompressed point is
 * 64 bytes, X | Y big-endian canonical; INFINITY IS 64 ZERO BYTES.  committed_i is the key's PublicAndCommitmentCommitted[i]
 * (mi_vk_set_public_committed).  Value i multiplies K[nb_public + i], as in mi_verify_input.
 *
 * NOT PINNED TO gnark's SOURCE: no gnark and no Go toolchain were at hand.  SHA-256 and expand_message_xmd are pinned by their
 * standards (and tested against an independent implementation); the two DST strings, the 64 zero bytes of an uncompressed infinity and
 * gnark-crypto's strictness on the infinity encoding (stray bits refused here) are written down from gnark's behaviour as documented,
 * not checked against it.  Before relying on this against proofs from gnark itself, verify one gnark proof first.
 *
 * Same library and conventions as mi355x_groth16_verify.h: int32 status codes, HOST pointers, mi_last_error; the library keeps no caller
 * pointer after return.  The workspace belongs to the context and only grows.
 */
#ifndef MI355X_GROTH16_VERIFY_BYTES_H
#define MI355X_GROTH16_VERIFY_BYTES_H
#include "mi355x_groth16_verify.h"

#ifdef __cplusplus
extern "C" {
#endif

/* gnark's vk.PublicAndCommitmentCommitted in CSR form: commitment i hashes, after its own point, full[j - 1] for j = indices[offsets[i]
 * .. offsets[i + 1]).  offsets has n_commitments + 1 entries, offsets[0] = 0, ascending.  A key starts with empty lists; indices may be
 * NULL when offsets[n_commitments] == 0.  MI_EINVAL (mi_last_error names the entry) for offsets that do not ascend from 0, or an index
 * outside 1 .. nb_public - 1 + i for commitment i: the public wires (1-based, the ONE wire is 0 and is never committed) and the values
 * of EARLIER commitments are all there is to commit to.  The lists are copied. */
int32_t mi_vk_set_public_committed(mi_ctx *ctx, mi_vk *vk, const uint32_t *offsets, const uint32_t *indices);

typedef struct mi_verify_bytes_input {
    const uint8_t *proof;            /* Proof.WriteTo's bytes */
    size_t proof_len;                /* must be 164 + 32 n_commitments of the key */
    const mi_fr *public_inputs;      /* nb_public - 1 Montgomery values, as mi_verify_input (may be NULL when nb_public == 1) */
} mi_verify_bytes_input;

/* Both return MI_OK whenever a verdict was reached (MI_VERIFY_* of mi355x_groth16_verify.h).  MI_EINVAL, before any device work: a null
 * pointer where one is required, or proof_len != 164 + 32 n_commitments -- the caller's framing error, not a property of the proof.
 * MI_VERIFY_MALFORMED: the count inside the proof differs from the key's, a point does not decode, or anything mi_groth16_verify calls
 * malformed.  A batch judges every proof on its own: verdicts[i] is exactly what mi_groth16_verify_bytes says for in[i]. */
int32_t mi_groth16_verify_bytes(mi_ctx *ctx, const mi_vk *vk, const uint8_t *proof, size_t proof_len, const mi_fr *public_inputs, uint8_t *verdict);
int32_t mi_groth16_verify_bytes_batch(mi_ctx *ctx, const mi_vk *vk, const mi_verify_bytes_input *in, size_t n, uint8_t *verdicts);

/* Host only: the inverse of mi_proof_write.  bytes[len] with len == 164 + 32 n_commitments and the same count inside -> proof, the
 * n_commitments points of commitments (may be NULL when n_commitments == 0) and pok.  MI_OK, or MI_EINVAL for a null pointer, another
 * length, another count or a point that does not decode (the outputs are then all infinity). */
int32_t mi_proof_read(const uint8_t *bytes, size_t len, uint32_t n_commitments, mi_proof_out *proof, mi_g1_affine *commitments, mi_g1_affine *pok);

/* Host only: H_dst(msg) above, one element of Fr in Montgomery form -- gnark-crypto's fr.Hash(msg, dst, 1)[0].  The prover side's
 * callers need it too: the challenge of mi_prover_submit_bsb22 and the commitment wires' values are these hashes.  MI_EINVAL for a null
 * pointer with a non-zero length, a null out, or dst_len outside 1 .. 255. */
int32_t mi_hash_to_field(const uint8_t *dst, size_t dst_len, const uint8_t *msg, size_t msg_len, mi_fr *out);

#ifdef __cplusplus
}
#endif
#endif

/* mi355x_groth16_vkfile.h -- verify from files: a verifying key and a public witness as the bytes gnark writes, decoded on the device.
 *
 * A verifier holds three files: vk.WriteTo's stream, proof.WriteTo's 164 + 32 k bytes and publicWitness.WriteTo's bytes.
 * mi355x_groth16_verify_bytes.h takes the second; this header takes the other two.  mi_vk_write writes a key, mi_vk_load_stream loads one
 * in any later process, and mi_groth16_verify_files* take (proof bytes, witness bytes) and give the verdicts of the
 * mi_groth16_verify_bytes* call of the same suffix.  The public inputs go up as bytes, become Montgomery words on the device (one value
 * per lane, csrc/witness_ops.cuh) and stay there: the host neither converts them nor sees them again.
 *
 * Same library and conventions as mi355x_groth16.h (int32 status codes, HOST pointers unless a name ends in _dev, mi_last_error,
 * nothing kept after return).
 *
 * KEY STREAM LAYOUT (VerifyingKey.WriteTo / WriteRawTo).  A point is encoded exactly as in mi355x_groth16_keyfile.h (MI_KEYFILE_RAW /
 * MI_KEYFILE_COMPRESSED), and malformed where that header calls it malformed:
 *     G1.Alpha | G1.Beta | G2.Beta | G2.Gamma | G1.Delta | G2.Delta
 *     u32-BE n_k | n_k x G1                                  (vk.G1.K)
 *     u32-BE n_lists | per list: u32-BE len | len x u64-BE   (PublicAndCommitmentCommitted)
 *     u32-BE n_commitment_keys | per key: G | GSigmaNeg      (two G2 points each)
 * Compressed, one commitment, an empty list and n_k = 4: 560 bytes; the same key raw: 1104.  The u64 values are the indices of
 * mi_vk_set_public_committed, by its rule and its range (list i: 1 .. nb_public - 1 + i).
 *
 * WITNESS LAYOUT (witness.WriteTo):
 *     u32-BE nbPublic | u32-BE nbSecret | u32-BE n (= nbPublic + nbSecret) | n x 32 bytes, big-endian canonical
 * The ONE wire is not in it: a key with nb_public wants nbPublic == nb_public - 1.  A full witness (nbSecret > 0) is accepted; its
 * public part is its first nbPublic values and the rest is not read.
 *
 * EXPERIMENTAL, as mi_pk_load_raw: BOTH LAYOUTS ARE RECALLED, NOT PINNED TO gnark (no gnark on the machines this was written on); the
 * caveat of mi355x_groth16_keyfile.h carries over unchanged.  tests/golden/vk_toy_c1.compressed.bin and vk_toy_c1.witness.bin are what
 * this library and its Python reference write: diff them against gnark's before relying on either layout. */
#ifndef MI355X_GROTH16_VKFILE_H
#define MI355X_GROTH16_VKFILE_H
#include "mi355x_groth16_keyfile.h"
#include "mi355x_groth16_verify_bytes.h"
#include "mi355x_groth16_verify_combined.h"
#include "mi355x_groth16_verify_locate.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- 1. the key's stream */
typedef struct mi_vk_stream_info {
    uint64_t n_k;                                   /* points of G1.K */
    uint32_t nb_public;                             /* n_k - n_commitment_keys: includes the ONE wire */
    uint32_t n_commitment_keys;
    uint64_t off_alpha1, off_beta1, off_beta2, off_gamma2, off_delta1, off_delta2;
    uint64_t off_k;                                 /* of K[0] (its count sits in the four bytes before) */
    uint64_t off_lists;                             /* of the u32 n_lists */
    uint64_t list_len[MI_PK_RAW_MAX_COMMITMENTS];   /* entries of list i */
    uint64_t off_list[MI_PK_RAW_MAX_COMMITMENTS];   /* of the first u64 of list i (its length sits in the four bytes before) */
    uint64_t off_commitment_keys;                   /* of the u32 n_commitment_keys */
    uint64_t off_ped[MI_PK_RAW_MAX_COMMITMENTS];    /* of G of key k; GSigmaNeg follows it */
    char refused[96];                               /* after MI_EINVAL: which field the stream was refused for (of the encoding whose
                                                       walk got furthest); empty after MI_OK */
} mi_vk_stream_info;
/* Host only, no device needed; the strictness of mi_pk_stream_inspect: every count cross-checked, the stream's length exact.  The
 * encoding is the one whose walk ends exactly at len, confirmed by the flag bits of G1.Alpha.  MI_EINVAL, info->refused naming the field:
 * n_lists != n_commitment_keys, n_k < 1 + n_commitment_keys, n_commitment_keys above MI_PK_RAW_MAX_COMMITMENTS, an index outside
 * mi_vk_set_public_committed's range or not below 2^32, or any length that does not add up. */
int32_t mi_vk_stream_inspect(const uint8_t *buf, size_t len, mi_vk_stream_info *info, uint32_t *encoding);

/* What a key file holds: mi_vk_desc's fields plus the two G1 points a verifier never uses (gnark writes them; so does this) and the
 * lists in the CSR form of mi_vk_set_public_committed.  Every pointer is a HOST pointer. */
typedef struct mi_vk_file_desc {
    mi_g1_affine alpha1, beta1, delta1;
    mi_g2_affine beta2, gamma2, delta2;
    const mi_g1_affine *k;
    uint64_t n_k;                    /* must equal nb_public + n_commitments */
    uint32_t nb_public;              /* includes the ONE wire */
    uint32_t n_commitments;          /* 0 .. MI_PK_RAW_MAX_COMMITMENTS */
    const mi_pedersen_vk *ped;       /* n_commitments entries; may be NULL when n_commitments == 0 */
    const uint32_t *pc_offsets;      /* n_commitments + 1 entries, or NULL: every list empty */
    const uint32_t *pc_indices;      /* may be NULL when pc_offsets[n_commitments] == 0 */
} mi_vk_file_desc;
/* Bytes of this key's stream in this encoding (the counts and pc_offsets alone are read). */
int32_t mi_vk_stream_size(const mi_vk_file_desc *desc, uint32_t encoding, size_t *len);
/* Writes the stream: K through the bulk encoders of mi_g1_compress_dev, the rest on the host.  Points are taken as given (on their
 * curve, reduced).  *len (may be NULL) = the stream's size.  cap too small: MI_EINVAL with *len set.  Whatever the error, nothing is
 * written to out_host: the device step comes first, into a buffer of its own. */
int32_t mi_vk_write(mi_ctx *ctx, const mi_vk_file_desc *desc, uint32_t encoding, uint8_t *out_host, size_t cap, size_t *len);

/* flags: MI_KEYFILE_NO_SUBGROUP_CHECK, MI_KEYFILE_SUBGROUP_BY_R.  Inspect, one upload, every point decoded on the device by the
 * decoders of mi_pk_load_stream (G1: on the curve; G2: on the twist and, unless told otherwise, in the r-torsion), one wait; then the
 * conditions mi_vk_load puts on a key (gamma2, delta2 and G not at infinity; all Pedersen keys share one G; K[i] at infinity is valid),
 * e(alpha, beta) and the lists.  G1.Beta and G1.Delta are decoded and checked like any G1 point and used for nothing else.
 * THE CONTRACT: the handle is indistinguishable from mi_vk_load + mi_vk_set_public_committed over the decoded points; free it with
 * mi_vk_free.  A refusal is MI_EINVAL, mi_last_error names the field (G1.Alpha, G1.Beta, G2.Beta, G2.Gamma, G1.Delta, G2.Delta, G1.K,
 * CommitmentKeys[k].G, CommitmentKeys[k].GSigmaNeg) and, for K, the lowest bad index; nothing is left allocated. */
int32_t mi_vk_load_stream(mi_ctx *ctx, const uint8_t *buf, size_t len, uint32_t flags, mi_vk **out);

/* mi_groth16_setup_to_stream plus the verifying key's stream, with an out / cap / len triple of its own: beta1, delta1 and the Pedersen
 * verifying keys (what mi_pedersen_vk_make computes from the trapdoor's sigma) are taken where Setup has them; the lists are empty, as
 * a key from Setup starts.  Both capacities are checked as soon as the counts are known, before any point is computed: MI_EINVAL with
 * both *len and *vk_len set, and no key either. */
int32_t mi_groth16_setup_to_streams(mi_ctx *ctx, const mi_r1cs_desc *r1cs, const mi_trapdoor *trapdoor, uint32_t encoding, uint8_t *out_host,
                                    size_t cap, size_t *len, uint8_t *vk_out_host, size_t vk_cap, size_t *vk_len, mi_pk **pk_out,
                                    mi_pedersen_pk **ped_out, mi_vk_out *vk_out);

/* ---- 2. the public witness.  Host only.
 * write: n Montgomery values -> 12 + 32 n bytes with header (n, 0, n).  cap too small: MI_EINVAL with *len set and nothing written.
 * read: the first nbPublic values of the witness, Montgomery; *n_out (may be NULL) = nbPublic.  MI_EINVAL for a null pointer, a header
 * that disagrees with itself or with len, cap < nbPublic (*n_out is set), or a value that is not below r. */
int32_t mi_public_witness_write(const mi_fr *values, size_t n, uint8_t *out, size_t cap, size_t *len);
int32_t mi_public_witness_read(const uint8_t *bytes, size_t len, mi_fr *out, size_t cap, size_t *n_out);

/* ---- 3. verifying from the two byte strings */
typedef struct mi_verify_files_input {
    const uint8_t *proof;            /* Proof.WriteTo's bytes */
    size_t proof_len;                /* must be 164 + 32 n_commitments of the key */
    const uint8_t *witness;          /* witness.WriteTo's bytes */
    size_t witness_len;              /* must be 12 + 32 n, n the third count of the witness's own header */
} mi_verify_files_input;
/* The arguments other than `in` are those of the mi_groth16_verify_bytes* call of the same suffix.  THE CONTRACT, exact: the
 * verdict(s), first_malformed and the locate stats equal what that call returns for the same proofs with public_inputs = the decoded
 * values.  MI_EINVAL, before any device work: a null pointer, proof_len wrong, witness_len != 12 + 32 n.  MI_VERIFY_MALFORMED for that
 * proof alone: nbPublic of the header differs from the key's nb_public - 1 (or the header's three counts do not add up), or a value is
 * not below r (ONE ENCODING of mi355x_groth16_verify.h). */
int32_t mi_groth16_verify_files(mi_ctx *ctx, const mi_vk *vk, const uint8_t *proof, size_t proof_len, const uint8_t *witness, size_t witness_len,
                                uint8_t *verdict);
int32_t mi_groth16_verify_files_batch(mi_ctx *ctx, const mi_vk *vk, const mi_verify_files_input *in, size_t n, uint8_t *verdicts);
int32_t mi_groth16_verify_files_combined(mi_ctx *ctx, const mi_vk *vk, const mi_verify_files_input *in, size_t n, const uint8_t *seed,
                                         uint8_t *verdict, uint64_t *first_malformed);
int32_t mi_groth16_verify_files_locate(mi_ctx *ctx, const mi_vk *vk, const mi_verify_files_input *in, size_t n, const uint8_t *seed,
                                       uint8_t *verdicts, mi_verify_locate_stats *stats);

#ifdef __cplusplus
}
#endif
#endif

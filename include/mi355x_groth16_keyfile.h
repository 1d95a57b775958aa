/* mi355x_groth16_keyfile.h -- proving keys as files: write a key from the device, load gnark's raw or compressed stream.
 *
 * mi_groth16_setup builds a key in HBM and a trapdoor must be forgotten, so that key has to leave the process that made it; and the
 * file most gnark users hold is the COMPRESSED one of pk.WriteTo(f), half the size of pk.WriteRawTo's.  Decoding it is one square
 * root per point (in Fp for G1, in Fp2 for G2) plus a membership test of the r-torsion per G2 point: data-parallel work that runs
 * here on the device, one point per lane.  This header closes the loop  Setup once -> write -> load in any later process -> prove.
 *
 * Same library and conventions as mi355x_groth16.h (status codes, Montgomery words on the ABI, mi_last_error).
 *
 * STREAM LAYOUT.  Both encodings have the layout of oracle/pk_raw.py field for field -- Domain block, G1.Alpha/Beta/Delta, the counted
 * sections G1.A, G1.B, G1.Z, G1.K, G2.Beta/Delta, counted G2.B, nbWires and the two infinity counts, the two bit-packed masks, the
 * Pedersen keys -- and differ in the size of a point alone:
 *     MI_KEYFILE_RAW          G1 64 bytes X | Y, G2 128 bytes X.A1 | X.A0 | Y.A1 | Y.A0; flag 00 (a point) or 01 (infinity)
 *     MI_KEYFILE_COMPRESSED   G1 32 bytes X, G2 64 bytes X.A1 | X.A0; flag 10 / 11 for the smaller / larger y, 01 for infinity
 * (the flag is the two top bits of byte 0; "larger" as mi_g1_compress / mi_g2_compress decide it; infinity is 40 00 ... 00).  A string
 * is MALFORMED where mi_groth16_verify_bytes.h calls a compressed point malformed -- a coordinate not below p, a flag of the other
 * encoding, an infinity with a stray bit, an X with no y -- and, raw, where (X, Y) is not on its curve.
 * EXPERIMENTAL, as mi_pk_load_raw: THE LAYOUT IS RECALLED, NOT PINNED TO gnark (no gnark on the machines this was written on); the
 * caveat of oracle/pk_raw.py and csrc/pk_raw.hip about the bit order of the masks carries over unchanged.
 *
 * A VERIFYING key as bytes (and the public witness as bytes) is mi355x_groth16_vkfile.h: mi_vk_load_stream, mi_vk_write. */
#ifndef MI355X_GROTH16_KEYFILE_H
#define MI355X_GROTH16_KEYFILE_H
#include "mi355x_groth16.h"
#include "mi355x_groth16_setup.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI_KEYFILE_RAW 0u
#define MI_KEYFILE_COMPRESSED 1u
/* flags of the decoders */
#define MI_KEYFILE_NO_SUBGROUP_CHECK 1u /* gnark's UnsafeReadFrom: G2 points are not tested for membership of the r-torsion */
#define MI_KEYFILE_SUBGROUP_BY_R 2u     /* measurement: that test by [r] Q (254 doublings) instead of the endomorphism (63) */

/* ---- 1. bulk point codecs: n points, one per lane; every pointer but first_bad is a DEVICE pointer, of any alignment.
 * Decoders: out_dev[i] = the point, (0, 0) for infinity and for a malformed string.  *first_bad (host, may be NULL) = the LOWEST
 * index whose string is malformed or (G2, unless MI_KEYFILE_NO_SUBGROUP_CHECK) whose point is not in the r-torsion, UINT64_MAX when
 * there is none; with one the call returns MI_EINVAL.  The calls return when the work is done. */
int32_t mi_g1_decompress_dev(mi_ctx *ctx, const uint8_t *bytes_dev, size_t n, mi_g1_affine *out_dev, uint64_t *first_bad);
int32_t mi_g2_decompress_dev(mi_ctx *ctx, const uint8_t *bytes_dev, size_t n, uint32_t flags, mi_g2_affine *out_dev, uint64_t *first_bad);
/* Encoders: encoding = MI_KEYFILE_RAW (64 / 128 bytes a point) or MI_KEYFILE_COMPRESSED (32 / 64).  Points are taken as given
 * (on their curve, reduced): these are the library's own arrays. */
int32_t mi_g1_compress_dev(mi_ctx *ctx, const mi_g1_affine *pts_dev, size_t n, uint32_t encoding, uint8_t *bytes_dev);
int32_t mi_g2_compress_dev(mi_ctx *ctx, const mi_g2_affine *pts_dev, size_t n, uint32_t encoding, uint8_t *bytes_dev);

/* ---- 2. loading either stream.
 * mi_pk_stream_inspect (host only, no device needed) has the strictness of mi_pk_raw_inspect -- every count cross-checked, the
 * stream length exact -- for both encodings: the encoding is the one whose section sizes add up to len, confirmed by the flag bits
 * of the first point.  On a raw stream it returns exactly what mi_pk_raw_inspect returns. */
int32_t mi_pk_stream_inspect(const uint8_t *buf, size_t len, mi_pk_raw_info *info, uint32_t *encoding);
/* mi_pk_load_raw's arguments plus flags (MI_KEYFILE_NO_SUBGROUP_CHECK, MI_KEYFILE_SUBGROUP_BY_R).  The stream is uploaded once and
 * decoded section by section straight into the arrays the key adopts.  It checks what gnark's ReadFrom checks, ON RAW STREAMS TOO
 * (mi_pk_load_raw checks neither): every G1 point on the curve (cofactor 1: nothing more to ask), every G2 point on the twist and in
 * the r-torsion.  A refusal is MI_EINVAL, mi_last_error names the section (G1.AlphaBetaDelta, G1.A, G1.B, G1.Z, G1.K, G2.BetaDelta,
 * G2.B, Basis[k], BasisExpSigma[k]) and the lowest bad index in it, and nothing is left allocated.
 * PEAK DEVICE MEMORY: the stream (len bytes) plus the decoded arrays (64 bytes a G1 point, 128 a G2 point: twice the compressed
 * stream's point bytes, or the raw stream's), held together until the last section is decoded; then the stream goes and the key is
 * built as by mi_pk_load_dev over arrays it owns.  The upload is not chunked. */
int32_t mi_pk_load_stream(mi_ctx *ctx, const uint8_t *buf, size_t len, uint32_t flags, uint32_t nb_public, const uint32_t *committed_wires,
                          size_t n_committed, mi_pk **out, mi_pedersen_pk **ped_out, uint32_t *n_ped_out);
/* Host-clock times of the last mi_pk_load_stream / mi_pk_write_dev on ctx, each span ending in a device synchronise.  load: upload
 * (host to device copy of the stream), decode (every section but the membership tests), subgroup (those), build (mi_pk_load_dev's
 * work and the Pedersen keys).  write: decode = the encode kernels, upload = the copies back to the host. */
typedef struct mi_keyfile_stats {
    float upload_ms, decode_ms, subgroup_ms, build_ms, total_ms;
} mi_keyfile_stats;
int32_t mi_keyfile_get_stats(mi_ctx *ctx, mi_keyfile_stats *out);

/* ---- 3. writing.  The writer takes plain arrays, not an mi_pk: a loaded key holds its points only as per-wire expanded copies and
 * fixed-base tables, and does not remember which private wires were cut from K. */
typedef struct mi_pedersen_arrays {
    const mi_g1_affine *basis_dev, *basis_exp_sigma_dev;   /* device pointers, n points each */
    uint64_t n;
} mi_pedersen_arrays;
/* Bytes of the stream of this key in this encoding (the counts of desc and ped alone are read). */
int32_t mi_pk_stream_size(const mi_pk_desc *desc, const mi_pedersen_arrays *ped, uint32_t n_ped, uint32_t encoding, size_t *len);
/* desc as for mi_pk_load_dev: the five point arrays are DEVICE pointers, the masks host pointers; nb_public, committed_wires and
 * n_committed are not part of a key file and are not read.  out_host receives the stream; *len (may be NULL) its size.  cap too
 * small: MI_EINVAL with *len set to the size needed and nothing written. */
int32_t mi_pk_write_dev(mi_ctx *ctx, const mi_pk_desc *desc, const mi_pedersen_arrays *ped, uint32_t n_ped, uint32_t encoding,
                        uint8_t *out_host, size_t cap, size_t *len);
/* mi_groth16_setup with the key's stream written at the one place where the plain arrays exist: before the key takes them.  pk_out
 * may be NULL (write only: no key is built and ped_out is not written); everything else is mi_groth16_setup's, refusals included.
 * cap too small: MI_EINVAL with *len set, and no key either. */
int32_t mi_groth16_setup_to_stream(mi_ctx *ctx, const mi_r1cs_desc *r1cs, const mi_trapdoor *trapdoor, uint32_t encoding, uint8_t *out_host,
                                   size_t cap, size_t *len, mi_pk **pk_out, mi_pedersen_pk **ped_out, mi_vk_out *vk_out);

#ifdef __cplusplus
}
#endif
#endif

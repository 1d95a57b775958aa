/* mi355x_groth16_phase2_check.h -- what makes a phase-2 ceremony (mi355x_groth16_phase2.h) checkable by someone other than its
 * coordinator: the pairing check that an SRS holds consistent powers, contributions that carry a proof of knowledge, and the
 * verification of a contributor's claimed state before it is taken over.
 *
 * Both checks come down to one primitive, the SAME-RATIO TEST.  For G1 arrays P, Q and G2 points s, t it decides
 *     e(sum_k r_k P_k, s) = e(sum_k r_k Q_k, t)
 * with coefficients r_k below 2^128 that the maker of the data could not predict: two MSMs, two Miller loops and one final
 * exponentiation, whatever the length of the arrays.  (Where the array is on the G2 side, the MSM is a G2 one.)
 *
 * COEFFICIENTS.  r_k is the little-endian integer of the first 16 bytes of
 *     SHA-256("mi355x-ceremony-coeff" | seed (32 bytes) | le64(k))
 * computed on the device, one lane per k.  One stream of coefficients serves every relation of a call: each relation is judged by its own
 * pairing product, so each keeps its own bound.  seed == NULL: the library draws the 32 bytes from the operating system (getrandom); if
 * that fails the call returns MI_ENODEV and no verdict.
 * THE SOUNDNESS CLAIM BELOW HOLDS ONLY FOR A SEED THE MAKER OF THE DATA CANNOT PREDICT: whoever knows the seed before choosing the points
 * knows every r_k and can make defects cancel.  A fixed seed is for tests and for reproducing a verdict, never for judging an SRS or a
 * state from someone else.
 *
 * GUARANTEES.  Rows and states that are what they should be pass every relation for every seed.  After the point checks every point lies
 * in a group of prime order r, so a relation reads sum_k r_k d_k = 0 mod r with d_k the defects in the exponent, and a non-zero d_k leaves
 * one value of r_k (of 2^128) that satisfies it: a relation that should fail passes with probability at most about 2^-128 over the seed.
 *
 * Same library and conventions as mi355x_groth16_phase2.h: status codes, Montgomery mi_fr, affine points with (0, 0) = infinity,
 * mi_last_error names the field, HOST pointers none of which the library keeps, nothing left allocated after a refusal.
 *
 * THE RECORDS OF CONTRIBUTIONS ARE THIS PROJECT'S OWN FORMAT.  gnark's mpcsetup layouts are not available to this project (see
 * mi355x_groth16_phase2.h); a transcript written here is read here.
 *
 * SIGMA HAS A CHAIN OF ITS OWN.  mi_phase2_contribute_proved leaves sigma / BasisExpSigma alone and mi_phase2_verify_adopt takes none from
 * outside; the re-randomisation of the commitment keys is proved, chained and adopted by the calls of the last section below
 * (mi_phase2_contribute_sigma_proved, mi_phase2_sigma_records_verify, mi_phase2_verify_adopt_sigma).  The state holds [-sigma_k]2 as a
 * point, so no party -- this library included -- needs the scalar after mi_phase2_init, which a ceremony calls with sigma = 1.
 *
 * NOT COVERED:
 *   - gnark's Phase1 / Phase2 file formats.
 * That BasisExpSigma IS sigma Basis for the sigma of the verifying key, and every other array the key of its circuit under its SRS, is
 * what mi355x_groth16_keyaudit.h checks without the derivation; who contributed to sigma is what the sigma chain says.
 * mi_srs_check_powers says that the rows ARE powers of one (tau, alpha, beta), not who contributed to them: that is what a phase-1 transcript
 * says, and mi355x_groth16_phase1.h makes and verifies one (its mi_phase1_verify_adopt and mi_phase1_check run the relations below over
 * rows that are on the device already).
 */
#ifndef MI355X_GROTH16_PHASE2_CHECK_H
#define MI355X_GROTH16_PHASE2_CHECK_H
#include "mi355x_groth16_phase2.h"
#include "mi355x_groth16_verify.h"   /* mi_pedersen_vk */

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- the SRS rows are consistent powers
 * the bits of *failed: the relation that does NOT hold (g1, g2: the generators) */
#define MI_SRS_BAD_GENERATORS 1u   /* tau_g1[0] != g1 or tau_g2[0] != g2 (compared as affine words) */
#define MI_SRS_BAD_TAU_G1     2u   /* e(sum_{k<2N-1} r_k tau_g1[k+1], g2) != e(sum r_k tau_g1[k], tau_g2[1]) */
#define MI_SRS_BAD_ALPHA_G1   4u   /* the same over alpha_tau_g1, k < N-1 */
#define MI_SRS_BAD_BETA_G1    8u   /* the same over beta_tau_g1,  k < N-1 */
#define MI_SRS_BAD_TAU_G2    16u   /* e(sum_{k<N} r_k tau_g1[k], g2) != e(g1, sum r_k tau_g2[k])   (a G2 MSM) */
#define MI_SRS_BAD_BETA_G2   32u   /* e(beta_tau_g1[0], g2) != e(g1, beta_g2) */

/* Times of the last mi_srs_check_powers on ctx by phase, in milliseconds of the host's clock around work that is waited for (the phases
 * run one after the other): upload: the rows to the device; point_check: the point checks mi_phase2_init makes; coeff: the coefficient
 * kernel; msm_g1 / msm_g2: the seven G1 MSMs / the G2 one; pairing: ten Miller loops, five final exponentiations and the verdicts.
 * peak_bytes: the most device memory the call's own allocations held at once (one row, the coefficients and a few points; the MSM's
 * workspaces belong to the context and are mi_get_mem_ledger's). */
typedef struct mi_srs_check_stats {
    float upload_ms, point_check_ms, coeff_ms, msm_g1_ms, msm_g2_ms, pairing_ms, total_ms;
    uint64_t peak_bytes;
} mi_srs_check_stats;

/* Reads exactly what mi_phase2_init reads for a circuit of domain size n_domain = N (a power of two >= 2): 2 N points of tau_g1, N of
 * each other row.  First the point checks of mi_phase2_init with its refusals: MI_EINVAL for a point off its curve, a G2 point outside
 * the r-torsion or a point at infinity, mi_last_error naming the row and the lowest bad index.  flags: 0 or
 * MI_KEYFILE_NO_SUBGROUP_CHECK, as there (WITHOUT the r-torsion test the soundness claim does not cover the G2 rows).  MI_EINVAL before
 * any device work: ctx, srs or failed null, a null or short row, n_domain not a power of two >= 2 or above 2^MI_SETUP_MAX_LOG_N, an
 * unknown flag.  MI_ENODEV: seed == NULL and no randomness.
 * Otherwise MI_OK and *failed = the mask of relations that do not hold; 0: the rows are [tau^k]1, [alpha tau^k]1, [beta tau^k]1, [tau^k]2,
 * [beta]2 for one (tau, alpha, beta).  Every relation is evaluated whatever the others say. */
int32_t mi_srs_check_powers(mi_ctx *ctx, const mi_srs_desc *srs, uint64_t n_domain, const uint8_t seed[32] /* may be NULL */, uint32_t flags,
                            uint32_t *failed);
int32_t mi_srs_check_get_stats(mi_ctx *ctx, mi_srs_check_stats *out);

/* ---------------------------------------------------------------- contributions with a proof of knowledge of delta (a Schnorr proof) */
typedef struct mi_phase2_record {
    mi_g1_affine delta1;     /* [delta]1 AFTER this contribution */
    mi_g1_affine commit;     /* T = [k] delta1_before */
    mi_fr        response;   /* z = k + c d mod r (Montgomery) */
    uint8_t      hash[32];   /* chain value after this record */
} mi_phase2_record;
/* hash_i = SHA-256("mi355x-phase2-record" | hash_(i-1) | le64(i) | compress(delta1_before) | compress(delta1) | compress(T))
 * c_i    = le integer of the first 16 bytes of SHA-256("mi355x-phase2-challenge" | hash_i);   accept iff [z] delta1_before = T + [c] delta1
 * compress = mi_g1_compress; hash_(-1) = the state's transcript id (32 zero bytes unless set) */

/* The id the first record's hash continues, of the delta chain and of the sigma chain alike.  Only before the first record of either
 * chain of the state: else MI_EINVAL. */
int32_t mi_phase2_set_transcript_id(mi_ctx *ctx, mi_phase2 *st, const uint8_t id[32]);
/* Does to the arrays exactly what mi_phase2_contribute(st, delta, NULL) does, then writes the record of that step and advances the
 * state's chain (its record count and chain hash).  nonce: the Schnorr nonce k, which must be secret, fresh and uniform -- NULL: drawn
 * from getrandom (MI_ENODEV when that fails); a given nonce is for tests.  delta = 0 or nonce = 0: MI_EINVAL, the state untouched.
 * A state on which plain mi_phase2_contribute is called does NOT advance its chain: its delta1 moves without a record, and such a state
 * will not verify for anyone else. */
int32_t mi_phase2_contribute_proved(mi_ctx *ctx, mi_phase2 *st, const mi_fr *delta, const mi_fr *nonce /* NULL: getrandom */, mi_phase2_record *out);
/* Host only, no context: the Schnorr chain of m records continuing (delta1_start, start_hash, first_index).  MI_OK with *first_bad = the
 * index in rec of the first record that does not hold, m when all hold.  A record whose points are off the curve or at infinity, or
 * whose response is not below r, does not hold.  MI_EINVAL: a null pointer (rec may be null with m = 0), or delta1_start off the curve or
 * at infinity. */
int32_t mi_phase2_records_verify(const mi_g1_affine *delta1_start, const uint8_t start_hash[32], uint64_t first_index,
                                 const mi_phase2_record *rec, size_t m, uint64_t *first_bad /* = m when all hold */);

/* ---------------------------------------------------------------- check a claimed state, then take it
 * The verifier derives its own state from the public SRS and R1CS (mi_phase2_init is deterministic) and brings it to where the
 * contributor started.  Only what depends on delta comes from outside; everything else (A, B, G2.B, vk.K, Basis, alpha, beta) stays the
 * verifier's own and needs no check. */
typedef struct mi_phase2_claim {          /* HOST pointers, layouts of mi_phase2_get_array */
    const mi_g1_affine *g1_z; uint64_t n_z;    /* MI_PHASE2_G1_Z */
    const mi_g1_affine *g1_k; uint64_t n_k;    /* MI_PHASE2_G1_K */
    mi_g1_affine delta1; mi_g2_affine delta2;
} mi_phase2_claim;
#define MI_PHASE2_BAD_RECORD 1u  /* mi_phase2_records_verify from the state's (delta1, chain, n_records) fails; *first_bad_record says where */
#define MI_PHASE2_BAD_DELTA  2u  /* claim.delta1 != rec[m-1].delta1, or e(delta1, g2) != e(g1, delta2) */
#define MI_PHASE2_BAD_Z      4u  /* e(sum r_i Z'_i, delta2') != e(sum r_i Z_i, delta2 of the state) */
#define MI_PHASE2_BAD_K      8u  /* the same over the private wires' K */
/* MI_EINVAL, the state untouched: a null argument (g1_k may be null with n_k = 0), m = 0, counts that differ from the state's, a claimed
 * point off its curve, delta2 off the twist or outside the r-torsion, a delta at infinity.  (0, 0) is allowed inside Z and K, where the
 * state's own arrays may hold it.  MI_ENODEV: seed == NULL and no randomness.
 * Otherwise MI_OK and *failed = the mask; every relation is evaluated whatever the others say.  *first_bad_record = m unless
 * MI_PHASE2_BAD_RECORD is set.  With mask 0, and only then, Z, K, delta1 and delta2 are copied into the state and its chain advances by
 * the m records; otherwise the state is bit for bit as it was. */
int32_t mi_phase2_verify_adopt(mi_ctx *ctx, mi_phase2 *st, const mi_phase2_claim *claim, const mi_phase2_record *rec, size_t m /* >= 1 */,
                               const uint8_t seed[32] /* may be NULL */, uint32_t *failed, uint64_t *first_bad_record /* may be NULL */);
/* Times of the last mi_phase2_verify_adopt on ctx, as mi_srs_check_stats (msm_g1: four MSMs; msm_g2_ms stays 0; pairing: six Miller loops
 * and three final exponentiations; point_check: the claimed arrays on the curve). */
int32_t mi_phase2_verify_get_stats(mi_ctx *ctx, mi_srs_check_stats *out);

/* ---------------------------------------------------------------- sigma: the state's points, proved contributions, a claimed state
 * Per commitment k the state holds g_sigma_neg_k = [-sigma_k]2 beside Basis_k and BasisExpSigma_k = sigma_k Basis_k: mi_phase2_init makes
 * the point as mi_pedersen_vk_make does, mi_phase2_contribute with a sigma_factor multiplies it, and everything that writes the verifying
 * half of the commitment keys (mi_phase2_to_streams, mi_key_claim_from_phase2) reads the state's points.  out[k] = {g2, g_sigma_neg_k}:
 * what a caller of mi_phase2_seal puts into mi_vk_desc.ped.  MI_EINVAL: a null argument (out may be null for a state without commitments). */
int32_t mi_phase2_get_pedersen_vk(mi_ctx *ctx, const mi_phase2 *st, mi_pedersen_vk *out /* n_commitments */);

/* One contribution step re-randomises ALL commitments of the state under one challenge (a Schnorr proof per commitment over the twist) */
typedef struct mi_phase2_sigma_proof {   /* one per commitment */
    mi_g2_affine g_sigma_neg;            /* AFTER this step: [s_k] before_k */
    mi_g2_affine commit;                 /* T_k = [n_k] before_k */
    mi_fr        response;               /* z_k = n_k + c s_k mod r (Montgomery) */
} mi_phase2_sigma_proof;
/* hash_i = SHA-256("mi355x-phase2-sigma-record" | hash_(i-1) | le64(i) | le32(n_commitments) |
 *                  for k: compress2(before_k) | compress2(after_k) | compress2(T_k))
 * c_i    = le integer of the first 16 bytes of SHA-256("mi355x-phase2-sigma-challenge" | hash_i)
 * accept iff the hash matches and [z_k] before_k = T_k + [c_i] after_k for every k
 * compress2 = mi_g2_compress.  The chain is the state's SECOND one: its own record count and its own 32-byte chain value, which starts
 * from the same transcript id as the delta chain.  The delta chain above does not change by a byte. */

/* Does to BasisExpSigma_k and g_sigma_neg_k exactly what mi_phase2_contribute(st, 1, sigma_factor) does and touches nothing that depends
 * on delta, then writes the step (n_commitments proofs and the chain value after it) and advances the sigma chain.  nonce: as
 * mi_phase2_contribute_proved's, one per commitment.  MI_EINVAL, the state bit for bit as it was: a null argument, a state without
 * commitments, a factor or nonce that is 0 or not below r.  MI_ENODEV: nonce == NULL and no randomness. */
int32_t mi_phase2_contribute_sigma_proved(mi_ctx *ctx, mi_phase2 *st, const mi_fr *sigma_factor /* [n_commitments] */,
                                          const mi_fr *nonce /* [n_commitments] or NULL: getrandom */,
                                          mi_phase2_sigma_proof *out /* [n_commitments] */, uint8_t hash_out[32]);
/* Host only, no context: the chain of m steps of nc commitments continuing (start, start_hash, first_index).  MI_OK with *first_bad = the
 * index of the first step that does not hold, m when all hold.  A step one of whose points is off the twist or at infinity, or one of whose
 * responses is not below r, does not hold.  MI_EINVAL: a null pointer (proofs and hashes may be null with m = 0), nc = 0, a start point
 * off the twist or at infinity. */
int32_t mi_phase2_sigma_records_verify(const mi_g2_affine *start /* [nc] */, uint32_t nc, const uint8_t start_hash[32], uint64_t first_index,
                                       const mi_phase2_sigma_proof *proofs /* [m * nc] */, const uint8_t (*hashes)[32] /* [m] */, size_t m,
                                       uint64_t *first_bad /* = m when all hold */);
/* Where the two chains of a state stand: what a verifier keeps books with (the points of sigma: mi_phase2_get_pedersen_vk) */
typedef struct mi_phase2_chain_info {
    uint32_t n_commitments, pad_;
    uint64_t n_records;        /* records of the delta chain so far */
    uint8_t  chain[32];        /* the value its next record continues: the transcript id until there is a record */
    uint64_t n_sigma_records;  /* steps of the sigma chain so far */
    uint8_t  sigma_chain[32];  /* the value its next step continues: the transcript id until there is a step */
} mi_phase2_chain_info;
int32_t mi_phase2_get_chain_info(mi_ctx *ctx, const mi_phase2 *st, mi_phase2_chain_info *out);

/* Check a claimed sigma state, then take it.  Basis_k and the generator are the verifier's own; only BasisExpSigma_k and g_sigma_neg_k
 * come from outside.  The coefficients r_i are those of the top of this file with i the index within the commitment. */
typedef struct mi_phase2_sigma_claim {          /* HOST pointers */
    const mi_g1_affine *const *basis_exp_sigma; /* [nc] arrays, layout of mi_phase2_get_array(MI_PHASE2_BASIS + 2k + 1) */
    const uint64_t *n;                          /* [nc] */
    const mi_g2_affine *g_sigma_neg;            /* [nc] */
} mi_phase2_sigma_claim;
#define MI_PHASE2_BAD_SIGMA_RECORD 16u  /* the sigma chain from the state's (g_sigma_neg, chain, count) fails; *first_bad_record says where */
#define MI_PHASE2_BAD_SIGMA_LINK   32u  /* some claim.g_sigma_neg[k] is not the last step's */
#define MI_PHASE2_BAD_BES          64u  /* some k: e(sum_i r_i Basis_k[i], g_sigma_neg'_k) . e(sum_i r_i BES'_k[i], g2) != 1; *bad_commitments bit k */
/* MI_EINVAL, the state untouched: a null argument, m = 0, a state without commitments (or with more than 64), a count that differs from
 * the state's, a claimed BasisExpSigma point off its curve ((0, 0) is allowed, where a basis point may be infinity), a claimed g_sigma_neg
 * off the twist, outside the r-torsion or at infinity.  MI_ENODEV: seed == NULL and no randomness (the rule of the seed is the one at the
 * top of this file).  Otherwise MI_OK, *failed = the mask and *bad_commitments = the commitments whose MI_PHASE2_BAD_BES relation fails;
 * every relation is evaluated whatever the others say.  *first_bad_record = m unless MI_PHASE2_BAD_SIGMA_RECORD is set.  With mask 0, and
 * only then, BasisExpSigma_k and g_sigma_neg_k are replaced and the sigma chain advances by the m steps; otherwise the state is bit for bit
 * as it was.  The delta chain and everything that depends on delta are not touched either way.  mi_phase2_verify_get_stats reports this
 * call's times too (msm_g1: two MSMs per commitment; pairing: two Miller loops and one final exponentiation per commitment). */
int32_t mi_phase2_verify_adopt_sigma(mi_ctx *ctx, mi_phase2 *st, const mi_phase2_sigma_claim *claim, const mi_phase2_sigma_proof *proofs,
                                     const uint8_t (*hashes)[32], size_t m /* >= 1 */, const uint8_t seed[32] /* may be NULL */, uint32_t *failed,
                                     uint64_t *bad_commitments, uint64_t *first_bad_record /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif

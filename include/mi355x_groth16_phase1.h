/* mi355x_groth16_phase1.h -- the powers-of-tau SRS itself, made on the device (BN254): a phase-1 ceremony that feeds
 * mi355x_groth16_phase2.h.
 *
 * mi_phase2_init derives a circuit's keys from an SRS whose tau, alpha, beta nobody knows.  This header is how such an SRS comes to be: a
 * state holds the rows of mi_srs_desc for a domain N = 2^log_n, contributors re-randomise tau, alpha, beta one after the other and leave
 * chained Schnorr records, a verifier checks a contributor's claimed rows before taking them over, and the rows go on to phase 2 without
 * leaving the device.  The hot path is csrc/scale_powers.cuh: every point of every row times its own full-width scalar c t^k, the same
 * instruction sequence in every lane (signed fixed-window digits over a per-lane table), row by row in chunks (csrc/phase1.hip).
 *
 * Same library and conventions as mi355x_groth16_phase2.h: status codes, Montgomery mi_fr, affine points with (0, 0) = infinity,
 * mi_last_error names the field, HOST pointers none of which the library keeps, nothing left allocated after a refusal, and a refused
 * call leaves the state bit for bit as it was.
 *
 * THE RECORDS OF CONTRIBUTIONS ARE THIS PROJECT'S OWN FORMAT, like the phase-2 ones.  gnark's mpcsetup layouts are not available to this
 * project (see mi355x_groth16_phase2.h); a transcript written here is read here.
 *
 * THE SAME-RATIO TESTS of mi_phase1_verify_adopt and mi_phase1_check are mi_srs_check_powers' (mi355x_groth16_phase2_check.h), over rows
 * that are already on the device, with its coefficients r_k = 128 bits of SHA-256("mi355x-ceremony-coeff" | seed | le64(k)).
 * THE SOUNDNESS CLAIM OF THAT HEADER HOLDS ONLY FOR A SEED THE MAKER OF THE DATA CANNOT PREDICT: whoever knows the seed before choosing the
 * points knows every r_k and can make defects cancel.  seed == NULL draws it from the operating system (MI_ENODEV if that fails); a fixed
 * seed is for tests and for reproducing a verdict, never for judging rows from someone else.
 *
 * NOT DONE HERE: gnark's Phase1 file format; a random beacon applied at the end of a ceremony (the last contribution is an ordinary one).
 */
#ifndef MI355X_GROTH16_PHASE1_H
#define MI355X_GROTH16_PHASE1_H
#include "mi355x_groth16_phase2.h"
#include "mi355x_groth16_phase2_check.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi_phase1 mi_phase1;   /* device-resident: tau_g1[2 N], alpha_tau_g1[N], beta_tau_g1[N], tau_g2[N], beta_g2, a record count and a
                                       * 32-byte chain value (the transcript id until there is a record) */

/* The last contribution on ctx (mi_phase1_contribute / _proved; mi_debug_scale_powers_dev fills row 0): per row -- 0: tau_g1, 1: alpha_tau_g1,
 * 2: beta_tau_g1, 3: tau_g2 -- the device time of the scalar multiplications (table and ladder) and of the conversions to affine (HIP
 * events on the context's stream); total_ms: the host's clock around the whole call; peak_bytes: the most device memory the call's own
 * allocations held at once (the table, the XYZZ results and the inversion scratch of one chunk; the rows are the state's). */
typedef struct mi_phase1_stats {
    float scalar_mul_ms[4], affine_ms[4], total_ms;
    uint32_t window, chunk;        /* what ran: 0 = the bit-by-bit yardstick, 2..5 = the window width; lanes per chunk */
    uint64_t peak_bytes;
} mi_phase1_stats;

/* Every row the generator: tau = alpha = beta = 1.  1 <= log_n <= MI_SETUP_MAX_LOG_N, else MI_EINVAL. */
int32_t mi_phase1_init(mi_ctx *ctx, uint32_t log_n, mi_phase1 **out);
/* An existing SRS taken in: 2 N / N points of its rows for n_domain = N (a power of two from 2 to 2^MI_SETUP_MAX_LOG_N), with
 * mi_phase2_init's point checks and refusals and the same texts ("phase2: srs.<row>[<index>] ...").  flags: 0 or
 * MI_KEYFILE_NO_SUBGROUP_CHECK.  The rows are NOT tested for being powers: mi_phase1_check does that. */
int32_t mi_phase1_from_srs(mi_ctx *ctx, const mi_srs_desc *srs, uint64_t n_domain, uint32_t flags, mi_phase1 **out);
/* The id the first record's hash continues.  Only before the first record of the state: else MI_EINVAL. */
int32_t mi_phase1_set_transcript_id(mi_ctx *ctx, mi_phase1 *st, const uint8_t id[32]);
/* tau_g1[k] <- [t^k] tau_g1[k], alpha_tau_g1[k] <- [a t^k] alpha_tau_g1[k], beta_tau_g1[k] <- [b t^k] beta_tau_g1[k],
 * tau_g2[k] <- [t^k] tau_g2[k], beta_g2 <- [b] beta_g2, with t = *tau, a = *alpha, b = *beta.  Any of the three 0 or not below r:
 * MI_EINVAL.  The new rows are built beside the old ones and swapped in at the end: a call that fails leaves the state as it was.
 * A state on which this plain form is called does not advance its chain and will not verify for anyone else. */
int32_t mi_phase1_contribute(mi_ctx *ctx, mi_phase1 *st, const mi_fr *tau, const mi_fr *alpha, const mi_fr *beta);

typedef struct mi_phase1_record {
    mi_g1_affine tau1, alpha1, beta1;   /* tau_g1[1], alpha_tau_g1[0], beta_tau_g1[0] AFTER this contribution */
    mi_g1_affine commit[3];             /* T_x = [k_x] before_x, x = 0: tau, 1: alpha, 2: beta */
    mi_fr        response[3];           /* z_x = k_x + c d_x mod r (Montgomery), d = (t, a, b) */
    uint8_t      hash[32];              /* chain value after this record */
} mi_phase1_record;
/* hash_i = SHA-256("mi355x-phase1-record" | hash_(i-1) | le64(i) | compress(before_x) x3 | compress(after_x) x3 | compress(T_x) x3)
 * c_i    = le integer of the first 16 bytes of SHA-256("mi355x-phase1-challenge" | hash_i): ONE challenge for the three proofs
 * accept iff the hash matches and [z_x] before_x = T_x + [c_i] after_x for x = 0, 1, 2
 * compress = mi_g1_compress; hash_(-1) = the state's transcript id (32 zero bytes unless set) */

/* mi_phase1_contribute, then the record of that step; the chain advances.  nonce: three Schnorr nonces, secret, fresh and uniform --
 * NULL: drawn from getrandom (MI_ENODEV when that fails); given nonces are for tests.  A nonce of 0 or not below r: MI_EINVAL. */
int32_t mi_phase1_contribute_proved(mi_ctx *ctx, mi_phase1 *st, const mi_fr *tau, const mi_fr *alpha, const mi_fr *beta,
                                    const mi_fr *nonce /* [3], or NULL: getrandom */, mi_phase1_record *out);
/* Host only, no context: the chain of m records continuing (start[3] = tau_g1[1], alpha_tau_g1[0], beta_tau_g1[0] before the first of
 * them; start_hash; first_index).  MI_OK with *first_bad = the index in rec of the first record that does not hold, m when all hold.  A
 * record with words off the curve, a point at infinity or a response that is not below r does not hold.  MI_EINVAL: a null pointer (rec
 * may be null with m = 0), or a start point off the curve or at infinity. */
int32_t mi_phase1_records_verify(const mi_g1_affine start[3], const uint8_t start_hash[32], uint64_t first_index, const mi_phase1_record *rec,
                                 size_t m, uint64_t *first_bad /* = m when all hold */);

/* ---------------------------------------------------------------- check claimed rows, then take them
 * The verifier's state stands where the contributor started.  2 N / N points of the claim are read. */
#define MI_PHASE1_BAD_RECORD  64u   /* mi_phase1_records_verify from the state's three points, chain value and record count fails */
#define MI_PHASE1_BAD_LINK   128u   /* claim.tau_g1[1], alpha_tau_g1[0] or beta_tau_g1[0] is not the last record's point */
/* First the point checks of mi_phase2_init over the claim, with its MI_EINVALs (and: a null argument, m = 0, a null or short row).
 * Otherwise MI_OK and *failed = the MI_SRS_BAD_* bits, with exactly mi_srs_check_powers' meaning over the claim, | MI_PHASE1_BAD_RECORD |
 * MI_PHASE1_BAD_LINK; every relation is evaluated whatever the others say.  *first_bad_record = m unless MI_PHASE1_BAD_RECORD is set.
 * With mask 0, and only then, the rows are copied into the state and its chain advances by the m records; otherwise the state is bit
 * for bit as it was.  MI_ENODEV: seed == NULL and no randomness. */
int32_t mi_phase1_verify_adopt(mi_ctx *ctx, mi_phase1 *st, const mi_srs_desc *claim, const mi_phase1_record *rec, size_t m /* >= 1 */,
                               const uint8_t seed[32] /* may be NULL */, uint32_t *failed, uint64_t *first_bad_record /* may be NULL */);
/* mi_srs_check_powers over the state's own rows, where they are: *failed = the MI_SRS_BAD_* mask. */
int32_t mi_phase1_check(mi_ctx *ctx, const mi_phase1 *st, const uint8_t seed[32] /* may be NULL */, uint32_t *failed);

/* What the state holds, without its rows: for a verifier's bookkeeping and mi_phase1_records_verify. */
typedef struct mi_phase1_info {
    uint32_t log_n, pad_;
    uint64_t n_records;
    uint8_t  chain[32];
    mi_g1_affine tau1, alpha1, beta1;    /* tau_g1[1], alpha_tau_g1[0], beta_tau_g1[0] */
} mi_phase1_info;
int32_t mi_phase1_get_info(mi_ctx *ctx, const mi_phase1 *st, mi_phase1_info *out);
/* The rows to host arrays of cap_* points (2 N, N, N, N are written).  A NULL row is not written; n[4] (never NULL) takes the counts
 * 2 N, N, N, N; beta_g2 may be NULL.  A non-NULL row whose cap is too small: MI_EINVAL, nothing written. */
int32_t mi_phase1_export(mi_ctx *ctx, const mi_phase1 *st, mi_g1_affine *tau_g1, mi_g1_affine *alpha_tau_g1, mi_g1_affine *beta_tau_g1,
                         mi_g2_affine *tau_g2, mi_g2_affine *beta_g2, uint64_t cap_tau_g1, uint64_t cap_alpha_tau_g1, uint64_t cap_beta_tau_g1,
                         uint64_t cap_tau_g2, uint64_t n[4]);
int32_t mi_phase1_free(mi_ctx *ctx, mi_phase1 *st);
int32_t mi_phase1_get_stats(mi_ctx *ctx, mi_phase1_stats *out);

/* ---------------------------------------------------------------- the handover
 * mi_phase2_init reading the SRS rows from the state's device arrays instead of uploading them (the state is not changed; the rows'
 * points were checked when they entered it, and are checked again as mi_phase2_init checks them).  Everything mi_phase2_init refuses
 * about the R1CS, sigma and flags; a circuit whose domain is above the state's N: MI_EINVAL. */
int32_t mi_phase2_init_from_phase1(mi_ctx *ctx, const mi_r1cs_desc *r1cs, const mi_phase1 *p1, const mi_fr *sigma, uint32_t flags, mi_phase2 **out);

#ifdef __cplusplus
}
#endif
#endif

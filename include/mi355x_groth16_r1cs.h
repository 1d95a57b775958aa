/* mi355x_groth16_r1cs.h -- a device-resident compiled R1CS: a = A W, b = B W, c = C W on the device, a constraint check, and
 * Groth16 proofs from the wire vector alone (BN254).
 *
 * Replaces the three arguments a, b, c of the call at mt.go:494-496 of the reference: the solver's wire vector W is all that crosses
 * PCIe per proof.  a and b are linear images of W under matrices the device can hold once per circuit, as it holds a proving key; c is
 * a o b (as mi_groth16_prove forms it when c is NULL) or C W on request.  The handle also gives a caller what the library could not
 * offer before: a device-side check that a wire vector satisfies the constraints.
 *
 * Same library and conventions as mi355x_groth16.h (status codes, Montgomery mi_fr, mi_last_error).  The descriptor is
 * mi355x_groth16_setup.h's mi_r1cs_desc, with the same rules: mi_r1cs_load refuses what mi_groth16_setup refuses of it (MI_EINVAL on the
 * host, before anything is allocated; mi_last_error names the field).  Its commitment fields are validated and not otherwise used.
 *
 * On the device, per matrix: n_constraints + 1 row offsets of 32 bits, one 8-byte (wire, coefficient) entry per non-zero, and the plan
 * of its long rows; the coefficient table once.  mi_r1cs_bytes reports the sum (about 8 B per entry + 4 B per row per matrix).
 * A handle is read-only after load: every context of the device it was loaded on -- all contexts of a prover pool -- may use it at the
 * same time, as they share a key.  Free it when no call that uses it is running or queued.
 */
#ifndef MI355X_GROTH16_R1CS_H
#define MI355X_GROTH16_R1CS_H
#include "mi355x_groth16_setup.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi_r1cs mi_r1cs;

int32_t mi_r1cs_load(mi_ctx *ctx, const mi_r1cs_desc *r1cs, mi_r1cs **out);   /* host CSR in; device-resident, read-only afterwards */
int32_t mi_r1cs_free(mi_ctx *ctx, mi_r1cs *r1cs);
int32_t mi_r1cs_bytes(const mi_r1cs *r1cs, uint64_t *out);                    /* device bytes held (not part of mi_mem_ledger) */

#define MI_R1CS_A 1u
#define MI_R1CS_B 2u
#define MI_R1CS_C 4u
/* The requested products (`which`: any of MI_R1CS_A | _B | _C; the pointer of a matrix that is not requested is not read).  Each
 * output has n_constraints rows in natural order, Montgomery form: what mi_compute_h takes.  A row without entries gives 0;
 * duplicate columns inside a row add up.  W has nb_wires values.  _dev: device pointers, the work is enqueued on the context's stream
 * and the call does not wait for it. */
int32_t mi_r1cs_eval_dev(mi_ctx *ctx, const mi_r1cs *r1cs, const mi_fr *W_dev, uint32_t which, mi_fr *a_dev, mi_fr *b_dev, mi_fr *c_dev);
int32_t mi_r1cs_eval(mi_ctx *ctx, const mi_r1cs *r1cs, const mi_fr *W, uint32_t which, mi_fr *a, mi_fr *b, mi_fr *c);
/* *n_bad = rows with (A W)(B W) != C W, *first_bad = the lowest such row (UINT64_MAX if none).  Synchronous; nothing is written but
 * the two counters. */
int32_t mi_r1cs_check_dev(mi_ctx *ctx, const mi_r1cs *r1cs, const mi_fr *W_dev, uint64_t *n_bad, uint64_t *first_bad);

/* The last evaluation (mi_r1cs_eval*, mi_r1cs_check_dev, or the one inside a mi_groth16_prove_w* / pool job) on ctx: device time of
 * its launches, the entries of the matrices it ran over, and how many of their rows were split over waves, into how many pieces. */
typedef struct mi_r1cs_stats {
    float eval_ms;
    uint32_t matrices;
    uint64_t entries, long_rows, pieces;
} mi_r1cs_stats;
int32_t mi_r1cs_get_stats(mi_ctx *ctx, mi_r1cs_stats *out);

/* mi_groth16_prove / _dev from W alone: a = A W and b = B W are evaluated on the device into the context's workspace.  Same proof
 * bytes as mi_groth16_prove(pk, W, A W, B W, NULL, r, s); with MI_PROVE_W_EVAL_C the same as with c = C W passed.
 * MI_EINVAL: n_wires differs from the key's or the R1CS's wire count, the key's log_n is not the domain of the R1CS's n_constraints,
 * the key is one part of a sharded key. */
#define MI_PROVE_W_EVAL_C 1u   /* c = C W evaluated on the device and passed to computeH's general path; default: c = a o b */
int32_t mi_groth16_prove_w(mi_ctx *ctx, mi_pk *pk, const mi_r1cs *r1cs, const mi_fr *W, size_t n_wires, uint32_t flags,
                           const mi_fr *r, const mi_fr *s, mi_proof_out *out, mi_stats *stats);
int32_t mi_groth16_prove_w_dev(mi_ctx *ctx, mi_pk *pk, const mi_r1cs *r1cs, const mi_fr *W_dev, size_t n_wires, uint32_t flags,
                               const mi_fr *r, const mi_fr *s, mi_proof_out *out, mi_stats *stats);
/* The prover pool's submit calls from W alone (mi_prover_wait, tickets and lifetimes as in mi355x_groth16.h).  The upload stage moves
 * W only; the worker evaluates.  stats->h2d_ms of a host job covers W alone. */
int32_t mi_prover_submit_w(mi_prover *p, mi_pk *pk, const mi_r1cs *r1cs, const mi_fr *W, size_t n_wires, uint32_t flags,
                           const mi_fr *r, const mi_fr *s, mi_proof_out *out, mi_stats *stats, uint64_t *ticket);
int32_t mi_prover_submit_w_dev(mi_prover *p, mi_pk *pk, const mi_r1cs *r1cs, const mi_fr *W_dev, size_t n_wires, uint32_t flags,
                               const mi_fr *r, const mi_fr *s, mi_proof_out *out, mi_stats *stats, uint64_t *ticket);
int32_t mi_prover_submit_w_bsb22(mi_prover *p, mi_pk *pk, const mi_r1cs *r1cs, const mi_fr *W, size_t n_wires, uint32_t flags,
                                 const mi_fr *r, const mi_fr *s, const mi_bsb22_input *commitments, uint32_t n_commitments,
                                 const mi_fr *challenge, mi_proof_out *out, mi_g1_affine *pok_out, mi_stats *stats, uint64_t *ticket);

#ifdef __cplusplus
}
#endif
#endif

/* mi355x_groth16_verify_ksum.h -- the public-input sums of a whole batch under one resident verifying key, in a number of kernel
 * launches that does not depend on the size of the batch.
 *
 * WHAT THE CALLS ARE FOR.  groth16.Verify (mt.go:497 of the reference) starts from kSum = K[0] + sum_j x_j K[1 + j] + sum_k C_k.  All
 * proofs of a batch share the bases K[1..] of their key, so the scalar part of a batch is a matrix of scalars times ONE vector of fixed
 * points.  A key keeps a window table of its bases,
 *     T[j][w][d] = d 2^(c w) K[1 + j],   c = 8, 4 or 2 bits,   ceil(254 / c) windows,   affine,
 * and the sum of a row is then additions of table entries alone: no doubling, no sorting, nothing per proof on the host.  A zero digit
 * costs nothing, so a byte-valued public input costs one addition at c = 8 and two at c = 4.  One launch adds the entries of slices of
 * every row's terms, a second adds each row's partial sums, a third goes back to affine with one inversion per 16 results.
 *
 * The verdict-per-proof verifiers (mi_groth16_verify_batch, mi_groth16_verify_wave, the bytes and files calls over them and the proofs
 * mi_groth16_verify_locate judges alone) stage their batches this way once the key has a table: the sums here, then the pairs of every
 * proof laid out by one more launch, where they ran one synchronous MSM per proof and the group law on the host before.  THE VERDICTS DO
 * NOT CHANGE, and neither does any word on the way: every coordinate is fully reduced, so a sum has one encoding, and the points below
 * are word for word what mi_msm_g1_dev gives for the row.
 *
 * THE TABLE.  Per base it takes ceil(254 / c) (2^c - 1) 64 bytes: about 522 KB at c = 8, 61 KB at c = 4, 24 KB at c = 2.  c is the
 * largest width whose table fits a byte budget.  The budget is MI_KSUM_DEFAULT_TABLE_BYTES = 64 MiB unless mi_vk_ksum_prepare names
 * another: c = 8 up to 128 bases, c = 4 up to 1092, c = 2 up to 2752.  A table is built once per key, on the device, by the first
 * verdict-per-proof call on the key that takes it (8 proofs or more, below) or by mi_vk_ksum_prepare, and mi_vk_free frees it.  The table belongs to the KEY: it is a device
 * allocation of its own beside the key's bases, which mi_vk_ksum_get_info reports (mi_get_mem_ledger takes a proving key and counts
 * no array of a verifying key).
 * Batches below 8 proofs keep the older stage as well: for one proof three launches and a gather are not faster than one MSM
 * (profiles/verify.txt), so such a call neither builds nor uses the table.  mi_vk_ksum_batch[_dev] use it at every n.
 * A key with no table stays on the older stage, one MSM per proof: when not even c = 2 fits the budget, when the device has not the
 * memory for the table or for building it, and when the key has no base (nb_public + n_commitments == 1).  mi_vk_ksum_get_info says
 * which.  A verify call never fails because of the table.
 *
 * RETURN VALUES.  MI_OK, or MI_EINVAL before any device work with mi_last_error naming the argument ("ksum: ..."): a null context (no
 * message), a null key, a null pointer where n > 0, n above 2^24, a key without bases where n > 0, and for the two batch calls a key
 * that has no table (call mi_vk_ksum_prepare first and read its info).  MI_ENOMEM / MI_EHIP as everywhere.  n == 0 gives MI_OK.
 * Same library and conventions as mi355x_groth16_verify.h; the workspace is the context's, the one the verifiers use, and only grows.
 */
#ifndef MI355X_GROTH16_VERIFY_KSUM_H
#define MI355X_GROTH16_VERIFY_KSUM_H
#include "mi355x_groth16_verify.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI_KSUM_DEFAULT_TABLE_BYTES ((uint64_t)64 << 20)

/* why a key has, or has not, a table */
#define MI_KSUM_NOT_BUILT 0   /* no call has asked for one yet */
#define MI_KSUM_READY 1
#define MI_KSUM_OVER_BUDGET 2 /* not even 2-bit windows fit the budget */
#define MI_KSUM_NO_MEMORY 3   /* the device had not the memory for the table, or for building it */
#define MI_KSUM_NO_BASES 4    /* the key has K[0] alone: there is nothing to sum */

typedef struct mi_vk_ksum_info {
    uint32_t window_bits;     /* c: 8, 4 or 2; 0 = the key has no table */
    uint32_t windows;         /* ceil(254 / c), 0 without a table */
    uint64_t table_bytes;     /* device bytes the table holds, 0 without */
    uint64_t bases;           /* nb_public - 1 + n_commitments: the scalars of one row */
    uint64_t budget_bytes;    /* the budget of the last build (the default before any) */
    uint32_t state;           /* MI_KSUM_* */
    float build_ms;           /* the last build, wall clock with its synchronisation */
} mi_vk_ksum_info;

/* Builds the key's table now under max_table_bytes (0 = MI_KSUM_DEFAULT_TABLE_BYTES), or builds it again when the key already has
 * one under another budget; the same budget again is no work.  MI_OK also when the key ends without a table (over budget, no memory,
 * no base): mi_vk_ksum_get_info says so, and the verifiers keep their older stage for the key.  The context must be idle on this key. */
int32_t mi_vk_ksum_prepare(mi_ctx *ctx, mi_vk *vk, uint64_t max_table_bytes);
int32_t mi_vk_ksum_get_info(mi_ctx *ctx, const mi_vk *vk, mi_vk_ksum_info *out);
/* out_dev[i] = sum_j scalars_dev[i * bases + j] K[1 + j] for i < n: affine, (0, 0) = infinity.  scalars_dev: n x bases Montgomery values
 * below r, row-major; skip_dev (may be null): n bytes, a non-zero byte leaves row i unread and out_dev[i] = infinity.  DEVICE pointers;
 * the launches go to the context's stream (mi_dev_sync before reading).  The key must have a table. */
int32_t mi_vk_ksum_batch_dev(mi_ctx *ctx, const mi_vk *vk, const mi_fr *scalars_dev, const uint8_t *skip_dev, size_t n, mi_g1_affine *out_dev);
/* The same over HOST pointers: upload, the launches, the points back, synchronised.  The public-input sums of n statements under a
 * resident key, with no pairing attached. */
int32_t mi_vk_ksum_batch(mi_ctx *ctx, const mi_vk *vk, const mi_fr *scalars, const uint8_t *skip, size_t n, mi_g1_affine *out);

#ifdef __cplusplus
}
#endif
#endif

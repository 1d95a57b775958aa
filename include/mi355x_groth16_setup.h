/* mi355x_groth16_setup.h -- groth16.Setup on the device (BN254): compiled R1CS and trapdoor in, device-resident proving key out.
 *
 * Replaces the call
 *     pk, vk, _ := groth16.Setup(ccs)
 * at mt.go:448 of the reference, which the reference pays on every run (it never stores a key).  The circuit, frontend.Compile and
 * the solver stay gnark's; Setup is pure arithmetic over the compiled R1CS and runs here: the Lagrange basis at tau, the transposed
 * sparse products sum_i M[i][j] L_i(tau) for M = A, B, C (csrc/setup.hip), the element-wise key exponents, and the points through the
 * same fixed-base kernels as mi_batch_scalar_mul_g1/g2_dev.  The key never crosses PCIe: only the R1CS goes up, and the two infinity
 * masks, the counts and the verifying key come down.
 *
 * Same library and conventions as mi355x_groth16.h (status codes, Montgomery mi_fr, mi_last_error).  All R1CS pointers are HOST
 * pointers (gnark's R1CS lives in host memory); the library keeps none of them after return.  The trapdoor is passed in, as r and s are
 * for mi_groth16_prove: the caller samples it (and must forget it), and a test can repeat a run.
 *
 * Definitions (w = the domain generator of fft.NewDomain(n_constraints), N = the domain size, oracle/pyref.py:toy_setup for the part
 * it covers):
 *     L_i(tau) = (tau^N - 1) / N * w^i / (tau - w^i)
 *     A_j = sum_i A[i][j] L_i(tau), likewise B_j, C_j        (rows >= n_constraints do not exist)
 *     t_j = beta A_j + alpha B_j + C_j
 *     infinity_a[j] = (A_j == 0), infinity_b[j] = (B_j == 0)
 *     pk.G1.A / pk.G1.B / pk.G2.B   A_j g1 / B_j g1 / B_j g2 for the wires not at infinity, in wire order
 *     pk.G1.K                       (t_j / delta) g1 for private wires that are neither committed nor a commitment wire, in wire order
 *                                   (a private wire in no constraint keeps its slot, with the point at infinity)
 *     pk.G1.Z                       N points, exponent tau^i (tau^N - 1) / delta, stored bit-reversed
 *     vk.G1.K                       (t_j / gamma) g1 for public wires and commitment wires, ascending wire index
 *     commitment k                  Basis[i] = (t_j / gamma) g1 for j = committed[k][i]; BasisExpSigma[i] = sigma_k Basis[i]
 * The Pedersen bases are what the verification equation forces (the commitment point is added to the public-input sum, which is over
 * gamma).  NOT PINNED TO gnark's SOURCE, which is not available to this project: before relying on commitments made with these keys
 * against a gnark verifier, compare one key with gnark's own Setup on the same trapdoor.
 */
#ifndef MI355X_GROTH16_SETUP_H
#define MI355X_GROTH16_SETUP_H
#include "mi355x_groth16.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI_SETUP_MAX_LOG_N 27        /* one device: the key's Z MSM takes at most MI_MSM_MAX_PAIRS pairs */

typedef struct mi_r1cs_matrix {      /* CSR: row = constraint, column = wire */
    const uint64_t *row_ptr;         /* n_constraints + 1 entries, row_ptr[0] = 0, non-decreasing; nnz = row_ptr[n_constraints] */
    const uint32_t *col;             /* nnz wire indices, each < nb_wires; duplicates inside a row are legal and add up */
    const uint32_t *coeff;           /* nnz indices into coeffs */
} mi_r1cs_matrix;

typedef struct mi_r1cs_desc {
    uint64_t n_constraints;          /* domain = next power of two >= n_constraints (fft.NewDomain), log_n <= MI_SETUP_MAX_LOG_N */
    uint64_t nb_wires;               /* as mi_pk_desc, at most MI_MSM_MAX_PAIRS */
    uint32_t nb_public;              /* as mi_pk_desc: includes the ONE wire, so >= 1 */
    mi_r1cs_matrix A, B, C;          /* nnz of each < 2^32 */
    const mi_fr *coeffs;             /* the interned coefficient table (gnark cs.Coefficients; the reference's Interner) */
    uint64_t n_coeffs;
    /* BSB22: commitment k commits to the private wires committed[k][0 .. n_committed[k]) and owns the wire commitment_wire[k] */
    uint32_t n_commitments;          /* 0 .. MI_PK_RAW_MAX_COMMITMENTS */
    const uint32_t *const *committed;
    const uint64_t *n_committed;
    const uint32_t *commitment_wire;
} mi_r1cs_desc;

typedef struct mi_trapdoor {
    mi_fr tau, alpha, beta, gamma, delta;
    mi_fr sigma[MI_PK_RAW_MAX_COMMITMENTS];   /* sigma[k] for k < n_commitments; the rest is not read */
} mi_trapdoor;

/* The verifying key's points (groth16 bn254 VerifyingKey.G1.Alpha, G2.Beta / Gamma / Delta, G1.K), host memory. */
typedef struct mi_vk_out {
    mi_g1_affine alpha1;
    mi_g2_affine beta2, gamma2, delta2;
    mi_g1_affine *k;                 /* caller's array of k_cap points; receives nb_public + n_commitments of them */
    uint64_t k_cap;
    uint64_t n_k;                    /* out: points written */
} mi_vk_out;

/* The Fr half of Setup, to host arrays.  Every pointer may be NULL (that array is not fetched). */
typedef struct mi_setup_exponents {
    mi_fr *a, *b, *c;                /* nb_wires each: A_j, B_j, C_j */
    mi_fr *k;                        /* nb_wires: t_j / delta for EVERY wire (pk.G1.K takes the rows named above) */
    mi_fr *k_gamma;                  /* nb_wires: t_j / gamma for every wire (vk.G1.K and the Pedersen bases take their rows from it) */
    mi_fr *z;                        /* N: the pk.G1.Z exponents in the stored, bit-reversed order */
    uint8_t *infinity_a, *infinity_b;/* nb_wires bytes each, 0 or 1 */
} mi_setup_exponents;

/* Device times of the last mi_groth16_setup / mi_groth16_setup_exponents call on ctx, by phase (HIP events on the context's stream;
 * the phases run one after the other, so they add up to total_ms but for the host work between them).  entries = nnz(A) + nnz(B) +
 * nnz(C); long_columns / chunks = columns whose entry lists were split over waves, and the pieces they were split into. */
typedef struct mi_setup_stats {
    float upload_ms, lagrange_ms, sparse_ms, elementwise_ms, points_ms, handover_ms, total_ms;
    float sparse_sort_ms, sparse_sum_ms;   /* the two halves of sparse_ms: counting sort by column, segmented sum */
    uint64_t entries, long_columns, chunks;
} mi_setup_stats;

/* groth16.Setup.  *pk_out is a device-resident mi_pk that owns its arrays and behaves in every later call exactly like one from
 * mi_pk_load (fixed-base tables, mi_pk_table_plan, mi_get_mem_ledger, mi_pk_free, the prover pool).  ped_out (room for n_commitments
 * handles; may be NULL when n_commitments == 0) receives the commitments' Pedersen keys; free them with mi_pedersen_pk_free.
 * MI_EINVAL, before any device work and with nothing allocated: a null pointer, row_ptr not starting at 0 or decreasing, nnz >= 2^32,
 * a col >= nb_wires, a coeff >= n_coeffs, log_n > MI_SETUP_MAX_LOG_N, nb_public of 0 or above nb_wires, a committed or commitment wire
 * that is public or listed twice, delta, gamma or a used sigma equal to 0, tau^N = 1 (tau on the domain), vk_out->k_cap too small.
 * mi_last_error names the field. */
int32_t mi_groth16_setup(mi_ctx *ctx, const mi_r1cs_desc *r1cs, const mi_trapdoor *trapdoor, mi_pk **pk_out,
                         mi_pedersen_pk **ped_out, mi_vk_out *vk_out);
/* The Fr half alone (the same device code mi_groth16_setup runs), results to host arrays: what a maintainer dumps when a key is in
 * doubt.  Same refusals. */
int32_t mi_groth16_setup_exponents(mi_ctx *ctx, const mi_r1cs_desc *r1cs, const mi_trapdoor *trapdoor, mi_setup_exponents *out);
int32_t mi_groth16_setup_get_stats(mi_ctx *ctx, mi_setup_stats *out);

#ifdef __cplusplus
}
#endif
#endif

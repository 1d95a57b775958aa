// What phase2.hip shares with phase2_check.hip (not part of the C-ABI): the ceremony state, the host checks of an SRS descriptor and
// the point checks of its rows on the device.
#pragma once
#include "ctx.h"
#include "fp12.cuh"
#include "dev_arena.h"
#include "abi_glue.h"
#include "../../include/mi355x_groth16_phase2_check.h"
#include <vector>

struct mi_phase2 {
    u32 log_n = 0, nb_public = 0, n_commitments = 0;
    u64 N = 0, nb_wires = 0;
    std::vector<u32> removed;             // committed + commitment wires: the private wires without a pk.G1.K point
    std::vector<uint8_t> inf_a, inf_b;
    // device arrays, affine
    void *g1_a = nullptr, *g1_b = nullptr, *g2_b = nullptr, *g1_k = nullptr, *g1_z = nullptr, *vk_k = nullptr;
    u64 n_a = 0, n_b = 0, n_k = 0, n_vk = 0;
    // g_sigma_neg = [-sigma]2 is what the library's outputs are made from; the scalar is a convenience that holds only while sigma_known
    // (until the state adopts points from outside), and nothing is computed from it after mi_phase2_init
    struct Ped { void *basis = nullptr, *bes = nullptr; u64 n = 0; Fr sigma; bool sigma_known = true; G2Aff g_sigma_neg; };
    std::vector<Ped> ped;
    G1Aff alpha1, beta1, delta1;
    G2Aff beta2, gamma2, delta2;
    // the chain of proved contributions (include/mi355x_groth16_phase2_check.h): records so far, and the hash the next one continues
    // (the transcript id until there is one)
    u64 n_records = 0;
    uint8_t chain[32] = {0};
    // the chain of proved contributions to sigma: a second one, which starts from the same transcript id
    u64 n_sigma_records = 0;
    uint8_t sigma_chain[32] = {0};
};

// null rows and rows shorter than the circuit needs (tau_g1: 2 N, the others: N)
int32_t mi_phase2_srs_host_check(mi_ctx *ctx, const mi_srs_desc *srs, u64 N);
// One row of an SRS on the device.  mi_phase2_check_points over n_rows of them: every point on its curve and not at infinity
// (point_check.cuh's POINT_RULE_SRS_ROW) -- the rows in the order given, the lowest bad index of the first bad row named -- then, unless flags holds MI_KEYFILE_NO_SUBGROUP_CHECK, every
// point of the G2 rows in the r-torsion, the same way.  MI_EINVAL with "phase2: srs.<name>[<index>] ..." in mi_last_error.  The stream
// is idle on return.  At most 8 rows.
struct Phase2Row { const char *name; bool g2; const void *pts; u64 n; };
int32_t mi_phase2_check_points(mi_ctx *ctx, Arena &ar, const Phase2Row *rows, int n_rows, uint32_t flags);
// mi_srs_check_powers' relations (phase2_check.hip) over rows that are ON THE DEVICE and have passed mi_phase2_check_points: the four row
// pointers of rows_dev are device pointers to 2 N / N points, beta_g2 sits in the descriptor.  seed may be null (getrandom; MI_ENODEV
// names `who`).  No row is copied; stats takes the times.
int32_t mi_srs_check_rows_dev(mi_ctx *ctx, const char *who, const mi_srs_desc *rows_dev, u64 N, const uint8_t *seed, mi_srs_check_stats &stats, uint32_t *failed);
// mi_phase2_init, or with on_device the same reading the SRS rows from device arrays (phase1.hip's handover: rows as above, the counts
// the arrays' own, so that a circuit they are too short for is refused as a short row is)
int32_t mi_phase2_init_rows(mi_ctx *ctx, const mi_r1cs_desc *r1cs, const mi_srs_desc *rows, bool on_device, const mi_fr *sigma, uint32_t flags, mi_phase2 **out);
// BasisExpSigma_k and g_sigma_neg_k times sf[k] for every commitment (k_phase2_scale_g1 / _g2): the sigma half of mi_phase2_contribute, and
// all of mi_phase2_contribute_sigma_proved's device work.  The stream is idle on return
int32_t mi_phase2_scale_sigma(mi_ctx *ctx, mi_phase2 *S, const Fr *sf);
// the Pedersen verifying pairs {g2, g_sigma_neg_k} of the state's points
void mi_phase2_pedersen_vk_of(const mi_phase2 *S, mi_pedersen_vk *out);

// ---------------------------------------------------------------------------------------------------- shared with keyaudit.hip
// The steps of a same-ratio test as phase2_check.hip runs them, for the audit of a key (include/mi355x_groth16_keyaudit.h).
// seed, or 32 bytes of the operating system's into own (MI_ENODEV names `who`)
int32_t mi_ceremony_seed_or_random(mi_ctx *ctx, const char *who, const uint8_t *&seed, uint8_t own[32]);
// out_dev[k] = r_k for k < n (k_ceremony_coeffs), Montgomery, enqueued on ctx->stream
int32_t mi_ceremony_coeffs_enqueue(mi_ctx *ctx, const uint8_t seed[32], u64 n, Fr *out_dev);
// sum_k scalars[k] bases[k] over device arrays of affine points (G1Aff / G2Aff), (0, 0) = infinity; Montgomery scalars.  The result is on
// the host on return.  A sum over no pair is infinity, whatever the pointers, and launches nothing
int32_t mi_ceremony_msm_g1(mi_ctx *ctx, const void *bases, const Fr *scalars, u64 n, G1Aff *out);
int32_t mi_ceremony_msm_g2(mi_ctx *ctx, const void *bases, const Fr *scalars, u64 n, G2Aff *out);
// The relations of one call: relation i is e(p[2 i], q[2 i]) = e(pb, q[2 i + 1]), with p[2 i + 1] = -pb
struct CeremonyRelations {
    std::vector<G1Aff> p;
    std::vector<G2Aff> q;
    void add(const G1Aff &pa, const G2Aff &qa, const G1Aff &pb, const G2Aff &qb);
    u32 count() const { return (u32)(p.size() / 2); }
};
// bad[i] = relation i does not hold: every pair through ONE launch of the Miller loop, a product and a final exponentiation per
// relation, k_ceremony_judge.  The stream is idle on return
int32_t mi_ceremony_judge(mi_ctx *ctx, Arena &ar, const CeremonyRelations &rel, std::vector<uint8_t> &bad);
// the four rows of a phase-1 state where they lie on the device, as a descriptor with the rows' own counts (phase1.hip)
struct mi_phase1;
mi_srs_desc mi_phase1_rows_desc(const mi_phase1 *p1);

// Internals of the prove path shared by prove.hip (one device) and group.hip (point-sharded over several devices).
#pragma once
#include "ctx.h"
#include "curve.cuh"
#include "msm_curve_ops.h"
#include "key_plan.h"
#include "abi_glue.h"   // fr_of: a scalar of the C-ABI (Montgomery words) as the library's Fr
#include <functional>
#include <future>
#include <cstring>

// The MSMs of a proof that share one sort of their scalars, as the key serves them.
struct KeyGroup {
    u32 c = 0;       // window width of the fixed-base tables; 0 = the generic path on the plain bases
    u32 gen_c = 0;   // generic-path window bits the parts of a sharded key agree on (0 = from n); stays 0 where there are tables
    u64 n = 0;       // pairs of each MSM of the group
    // per MSM: the device array its level-1 accumulation gathers from (fixed-base window copies 2^(c*w) * P of the bases, msm2_core.cuh,
    // or the plain bases) and the pair count it reports (mi_msm_enqueue's stat_pairs: 0 = n)
    struct { void *pts = nullptr; u64 stat_pairs = 0; } bases[2];
};
// The groups, in the order of FixedBasePlan::c and ctx->fixed_knob: A + K over all wires (pk.G1.A and pk.G1.K re-expanded to one slot per
// wire, zero = infinity where the wire has no point: both are multiplied by W itself, so ONE sort of W serves both and neither needs a
// gather), B1 + B2 over the gathered B wires, Z over h.
enum { KEY_AK, KEY_B, KEY_Z };
static constexpr int KEY_GROUP_MSMS[3] = {2, 2, 1}, KEY_GROUP_CURVE[3][2] = {{1, 1}, {1, 2}, {1, 1}};
enum { KEY_MEM_BASES, KEY_MEM_TABLES, KEY_MEM_INDICES };   // mi_mem_ledger's key_bases, key_tables, key_indices

struct mi_pk {
    u32 log_n = 0, nb_public = 0;
    u64 nb_wires = 0;
    KeyGroup group[3];
    const u32 *idx_b = nullptr;   // wire index of every B point (the gather of wireValuesB)
    // The arrays of every group hold both coordinates times 2^5: the R' = 2^261 packed form of the 9 x 29-bit kernel
    // (msm_curve_ops.h).  Arrays of the caller (mi_pk_load_dev) are never rewritten: the key points at converted copies of its own then.
    bool rprime = false;
    G1Aff alpha1, beta1, delta1;
    G2Aff beta2, delta2;
    // A part of a point-sharded key (group.hip) covers wires [wire_lo, wire_lo + nb_wires) and the Z pairs
    // [z_lo, z_lo + n_z_msm) of the 2^log_n - 1; a whole key has wire_lo = z_lo = 0 and n_z_msm = 2^log_n - 1.
    u64 wire_lo = 0, z_lo = 0, n_z_msm = 0;
    // Every device allocation the key frees, and their bytes by KEY_MEM_* as they come and go.  Arrays of the caller are not among them.
    struct Alloc { void *p; u64 bytes; int kind; };
    std::vector<Alloc> owned;
    u64 mem[3] = {0, 0, 0};
    void own(void *p, u64 bytes, int kind) { owned.push_back({p, bytes, kind}); mem[kind] += bytes; }
    void drop(void *p) { for (Alloc &a : owned) if (p && a.p == p) { (void)hipFree(p); mem[a.kind] -= a.bytes; a.p = nullptr; } }   // frees one of them now
};

struct ShardRange { u64 w_lo, w_hi, z_lo, z_hi; };   // wires [w_lo, w_hi), Z pairs [z_lo, z_hi)
// mi_pk_load / mi_pk_load_dev (sr == nullptr) or one part of a sharded key (host arrays only)
// sr with device_points: the arrays are this part's slices on ctx's device (mi_pk_load_sharded_dev).
// forced (null: the key plans for itself): the table plan of a sharded key's parts; a knob the caller set on the context wins for its group
// adopt (device_points only): the key takes ownership of the five arrays; *took_arrays = true once it has (then they are released by
// the key on success and by this function on failure -- the caller must not free them again).
int32_t mi_pk_load_range(mi_ctx *ctx, const mi_pk_desc *d, mi_pk **out, bool device_points, const ShardRange *sr, const FixedBasePlan *forced = nullptr,
                         bool adopt = false, bool *took_arrays = nullptr);
// a Pedersen key over device arrays the key takes ownership of (mi_pk_load_raw)
extern "C" int32_t mi_pedersen_pk_adopt(mi_ctx *ctx, void *basis_dev, void *basis_exp_sigma_dev, size_t n, mi_pedersen_pk **out);
// ProveKnowledge of one BSB22 commitment in two halves on MSM_SLOT_POK of ctx (beside a proof's five MSMs): host values in, affine point out
int32_t mi_pedersen_pok_enqueue(mi_ctx *ctx, mi_pedersen_pk *pk, const mi_fr *values, size_t n);
int32_t mi_pedersen_pok_collect(mi_ctx *ctx, mi_g1_affine *pok_or_null);
// The wire MSMs (MSM_SLOT_A, _B1, _B2, _K) over W_dev = this key's wire range, ordered after ev_w; the Z MSM (MSM_SLOT_Z) over
// h_dev = this key's first h coefficient, ordered after ev_h.  defer_reduce: stop each MSM at its bucket sums (group.hip
// exchanges them between devices before the reduce, SURVEY 8e option ii).
// The wire MSMs are two independent groups, each with one sort and one host-side wait for that sort's count pass: B1 + B2 and A + K
// (own slots, own buffers: safe to enqueue from two threads at once).  start() hands each group to a helper thread and returns at
// once; join() waits for both and returns the first failure.  A group for which no thread can be had is enqueued by start() on the
// calling thread, without the gate (the caller would wait for itself); no exception crosses either call.
// accum_gate (may be null): MsmSlot::accum_gate for the four slots -- the sorts are enqueued at once, the bucket accumulations
// behind the event it returns.
struct WireMsms {
    std::future<int32_t> f_b, f_ak;
    int32_t rc_inline = MI_OK;
    void start(mi_ctx *ctx, mi_pk *pk, const mi_fr *W_dev, hipEvent_t ev_w, bool defer_reduce, const std::function<hipEvent_t()> *accum_gate);
    int32_t join();
};
// start() and join() in one call
int32_t mi_prove_enqueue_wire_msms(mi_ctx *ctx, mi_pk *pk, const mi_fr *W_dev, hipEvent_t ev_w, bool defer_reduce = false);
int32_t mi_prove_enqueue_z_msm(mi_ctx *ctx, mi_pk *pk, const mi_fr *h_dev, hipEvent_t ev_h, bool defer_reduce = false);

// mi_groth16_prove_dev over inputs that are still arriving in HBM (the prover pool's upload stage): the one schedule of prove_common
// (prove.hip) with W resident when the call is made -- the wire MSMs are enqueued at once, with nothing to wait for -- and
// abc_ready(k), k = 1, 2, 3, asked right before computeH's part for a, b, c is enqueued: it must block until k of a, b, c (in that
// order) are resident (false = their upload failed; k = 3 is never asked for when c is null).  abc_arrived: they all were when the job
// was picked up (the steady state): only then may the wire MSMs' accumulations be held back for computeH.  Same proof bytes.
int32_t mi_groth16_prove_dev_gated(mi_ctx *ctx, mi_pk *pk, const mi_fr *W_dev, size_t n_wires, const mi_fr *a_dev, const mi_fr *b_dev, const mi_fr *c_dev,
                                   size_t n_constraints, const mi_fr *r, const mi_fr *s, mi_proof_out *out, mi_stats *stats,
                                   const std::function<bool(int)> &abc_ready, bool abc_arrived);

// Blinding and assembly of Ar, Bs, Krs from the five MSM sums, exactly as gnark's prove.go composes them (row a9); host
// code over O(1) points.  start() launches the multiples of delta on host threads while the GPU works; have_a_b1() needs
// only the A and B1 sums and starts s*Ar, r*Bs1; finish() takes the rest.
struct ProofAssembler {
    const mi_pk *pk = nullptr;
    Fr rc, sc, krc;
    std::future<G1X> f_r, f_s, f_kr, f_sar;
    G2X s_delta2;
    G1X r_delta, s_delta, kr_delta, r_bs1;
    G1Aff ar_aff, bs1_aff;
    void start(const mi_pk *pk_, const mi_fr *r_m, const mi_fr *s_m);
    void have_a_b1(const G1X &msm_a, const G1X &msm_b1);
    void finish(const G1X &msm_k, const G2X &msm_b2, const G1X &msm_z, mi_proof_out *out);
};

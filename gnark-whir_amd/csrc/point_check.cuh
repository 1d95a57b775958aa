// "Is this array made of points?" -- the one predicate, the one kernel pair and the one launcher behind every bulk check of points that
// come from outside as plain affine words: an SRS row (phase2.hip's mi_phase2_check_points), a claimed state of a ceremony
// (phase2_check.hip) and the arrays of mi_key_claim_from_arrays (keyaudit.hip).  The predicate is MI_HD: the host build of the tests
// (tests/cpp/keyaudit_host.cpp) runs the same text.  Points that arrive as a stream's bytes are judged by their decoders (keyfile.hip).
//
// The curve equation is always asked.  What else is asked differs by caller, and the differences are as they were found, not designed:
// pairing.cuh ("the checks a verifier makes on points it did not compute") says why a verifier wants exactly one encoding of a point, and
// an SRS row is not asked for it.
#pragma once
#include "pairing.cuh"

constexpr u32 POINT_ALLOW_INF = 1;      // (0, 0), the point at infinity, passes
constexpr u32 POINT_NEED_REDUCED = 2;   // every coordinate word, read as a 256-bit integer, is below the modulus (else x and x + p both pass)
constexpr u32 POINT_RULE_SRS_ROW = 0;                                      // an SRS row: no infinity; words that are NOT reduced pass
constexpr u32 POINT_RULE_CLAIM = POINT_ALLOW_INF | POINT_NEED_REDUCED;     // a claimed Z, K or BasisExpSigma of a ceremony
constexpr u32 POINT_RULE_AUDIT = POINT_NEED_REDUCED;                       // an array of a key claim, | POINT_ALLOW_INF where the array may hold it
constexpr u32 point_rule_audit(bool allow_inf) { return POINT_RULE_AUDIT | (allow_inf ? POINT_ALLOW_INF : 0); }

MI_HD bool point_ok(const G1Aff &p, u32 rule) {
    if ((rule & POINT_NEED_REDUCED) && !g1_reduced(p)) return false;
    if (p.is_inf()) return (rule & POINT_ALLOW_INF) != 0;
    return fe_sqr(p.y) == fe_sqr(p.x) * p.x + curve_b((const Fp *)0);
}
MI_HD bool point_ok(const G2Aff &q, u32 rule) {
    if ((rule & POINT_NEED_REDUCED) && !g2_reduced(q)) return false;
    if (q.is_inf()) return (rule & POINT_ALLOW_INF) != 0;
    return g2_on_twist(q);
}

#if defined(__HIPCC__)
#include "ctx.h"
// *first_bad (a device word that starts at UINT64_MAX: BadSlots, dev_arena.h) takes the lowest index whose point does not pass.  Static, as
// scan_u32.cuh's kernels are: a translation unit that includes this header carries its own copy.  Plain names, no template: a
// template's name carries its signature into every trace (keyfile.hip)
static __global__ void __launch_bounds__(256) k_points_check_g1(const G1Aff *pts, u64 n, u32 rule, unsigned long long *first_bad) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && !point_ok(pts[i], rule)) atomicMin(first_bad, (unsigned long long)i);
}
static __global__ void __launch_bounds__(256) k_points_check_g2(const G2Aff *pts, u64 n, u32 rule, unsigned long long *first_bad) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && !point_ok(pts[i], rule)) atomicMin(first_bad, (unsigned long long)i);
}
// n points of G1, or with g2 of the twist, on ctx->stream; no point, no launch
static inline int32_t mi_points_check_enqueue(mi_ctx *ctx, bool g2, const void *pts, u64 n, u32 rule, unsigned long long *first_bad) {
    if (!n) return MI_OK;
    if (g2) hipLaunchKernelGGL(k_points_check_g2, dim3(mi_blocks_of(n, 256)), dim3(256), 0, ctx->stream, (const G2Aff *)pts, n, rule, first_bad);
    else hipLaunchKernelGGL(k_points_check_g1, dim3(mi_blocks_of(n, 256)), dim3(256), 0, ctx->stream, (const G1Aff *)pts, n, rule, first_bad);
    MI_CHECK_HIP(ctx, hipGetLastError());
    return MI_OK;
}
#endif

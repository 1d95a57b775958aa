// The chain of a phase-1 ceremony's contribution records on the host (include/mi355x_groth16_phase1.h): mi_phase1_records_verify.  This
// file holds no HIP call: the arithmetic is phase1_ops.cuh's text over ceremony_ops.cuh's helpers, and tests/cpp/phase1_host.cpp builds
// it as plain C++ under the sanitizers (make sanitize-phase1).
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>   // the qualifiers of MI_HD alone; nothing here calls the runtime
#endif
#include "../../include/mi355x_groth16_phase1.h"
#include "phase1_ops.cuh"
#include <cstring>

static_assert(sizeof(mi_phase1_record) == sizeof(Phase1Record) && sizeof(mi_phase1_record) == 512 && offsetof(mi_phase1_record, alpha1) == 64 &&
              offsetof(mi_phase1_record, beta1) == 128 && offsetof(mi_phase1_record, commit) == 192 && offsetof(mi_phase1_record, response) == 384 &&
              offsetof(mi_phase1_record, hash) == 480, "phase1_ops.cuh reads the header's record as a Phase1Record");
static_assert(offsetof(mi_phase1_info, alpha1) == offsetof(mi_phase1_info, tau1) + 64 && offsetof(mi_phase1_info, beta1) == offsetof(mi_phase1_info, tau1) + 128,
              "the three watched points of mi_phase1_info lie one after the other");

extern "C" int32_t mi_phase1_records_verify(const mi_g1_affine start[3], const uint8_t start_hash[32], uint64_t first_index, const mi_phase1_record *rec, size_t m,
                                            uint64_t *first_bad) {
    if (!start || !start_hash || !first_bad || (!rec && m)) return MI_EINVAL;
    G1Aff s[3];
    std::memcpy(s, start, sizeof(s));
    for (int x = 0; x < 3; x++)
        if (!g1_on_curve(s[x]) || s[x].is_inf()) return MI_EINVAL;
    *first_bad = phase1_records_first_bad(s, start_hash, first_index, (const Phase1Record *)rec, m);
    return MI_OK;
}

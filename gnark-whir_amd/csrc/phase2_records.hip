// The chain of a ceremony's contribution records on the host (include/mi355x_groth16_phase2_check.h): mi_phase2_records_verify.  This
// file holds no HIP call: the arithmetic is ceremony_ops.cuh's MI_HD text, and tests/cpp/phase2_check_host.cpp builds it as plain C++
// under the sanitizers (make sanitize-phase2-check).
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>   // the qualifiers of MI_HD alone; nothing here calls the runtime
#endif
#include "../../include/mi355x_groth16_phase2_check.h"
#include "ceremony_ops.cuh"
#include <cstring>

static_assert(sizeof(mi_phase2_record) == sizeof(CeremonyRecord) && sizeof(mi_phase2_record) == 192 && offsetof(mi_phase2_record, response) == 128 &&
              offsetof(mi_phase2_record, hash) == 160, "ceremony_ops.cuh reads the header's record as a CeremonyRecord");

extern "C" int32_t mi_phase2_records_verify(const mi_g1_affine *delta1_start, const uint8_t start_hash[32], uint64_t first_index, const mi_phase2_record *rec,
                                            size_t m, uint64_t *first_bad) {
    if (!delta1_start || !start_hash || !first_bad || (!rec && m)) return MI_EINVAL;
    G1Aff start;
    std::memcpy(&start, delta1_start, sizeof(start));
    if (!g1_on_curve(start) || start.is_inf()) return MI_EINVAL;
    *first_bad = ceremony_records_first_bad(start, start_hash, first_index, (const CeremonyRecord *)rec, m);
    return MI_OK;
}

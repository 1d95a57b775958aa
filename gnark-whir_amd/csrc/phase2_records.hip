// The chains of a ceremony's contribution records on the host (include/mi355x_groth16_phase2_check.h): mi_phase2_records_verify for delta
// over G1, mi_phase2_sigma_records_verify for sigma over the twist.  This
// file holds no HIP call: the arithmetic is ceremony_ops.cuh's MI_HD text, and tests/cpp/phase2_check_host.cpp and
// tests/cpp/phase2_sigma_host.cpp build it as plain C++ under the sanitizers (make sanitize-phase2-check, make sanitize-phase2-sigma).
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

static_assert(sizeof(mi_phase2_sigma_proof) == sizeof(CeremonySigmaProof) && sizeof(mi_phase2_sigma_proof) == 288 && offsetof(mi_phase2_sigma_proof, commit) == 128 &&
              offsetof(mi_phase2_sigma_proof, response) == 256, "ceremony_ops.cuh reads the header's sigma proof as a CeremonySigmaProof");

extern "C" int32_t mi_phase2_sigma_records_verify(const mi_g2_affine *start, uint32_t nc, const uint8_t start_hash[32], uint64_t first_index,
                                                  const mi_phase2_sigma_proof *proofs, const uint8_t (*hashes)[32], size_t m, uint64_t *first_bad) {
    if (!start || !nc || !start_hash || !first_bad || ((!proofs || !hashes) && m)) return MI_EINVAL;
    std::vector<G2Aff> st(nc);
    std::memcpy(st.data(), start, (size_t)nc * sizeof(G2Aff));
    for (uint32_t k = 0; k < nc; k++) if (!ceremony_sigma_point_ok(st[k])) return MI_EINVAL;
    *first_bad = ceremony_sigma_first_bad(st.data(), nc, start_hash, first_index, (const CeremonySigmaProof *)proofs, hashes, m);
    return MI_OK;
}

// The host-only entry points of include/mi355x_groth16_verify_bytes.h: mi_proof_read (the inverse of mi_proof_write, api.hip) and
// mi_hash_to_field.  They run the bodies the kernels of verify_bytes.hip run (decode_ops.cuh, sha256_h2f.cuh).  No HIP call in this file: it
// also builds as plain C++ with the sanitizers (Makefile `sanitize`, tests/cpp/decode_fuzz.cpp), since it reads bytes from outside.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>   // the qualifiers of MI_HD alone; nothing here calls the runtime
#endif
#include "../../include/mi355x_groth16_verify_bytes.h"
#include "sha256_h2f.cuh"
#include <cstring>

static_assert(sizeof(mi_g1_affine) == sizeof(G1Aff) && sizeof(mi_g2_affine) == sizeof(G2Aff) && sizeof(mi_fr) == sizeof(Fr),
              "decode_ops.cuh writes the header's records as G1Aff / G2Aff / Fr");

extern "C" {

int32_t mi_proof_read(const uint8_t *bytes, size_t len, uint32_t n_commitments, mi_proof_out *proof, mi_g1_affine *commitments, mi_g1_affine *pok) {
    if (!bytes || !proof || !pok || (!commitments && n_commitments)) return MI_EINVAL;
    std::memset(proof, 0, sizeof(*proof));
    std::memset(pok, 0, sizeof(*pok));
    if (n_commitments && n_commitments <= MI_PK_RAW_MAX_COMMITMENTS) std::memset(commitments, 0, (size_t)n_commitments * sizeof(mi_g1_affine));
    if (n_commitments > MI_PK_RAW_MAX_COMMITMENTS || len != proof_bytes_len(n_commitments) || proof_bytes_count(bytes) != n_commitments) return MI_EINVAL;
    G1Aff ar, krs, pk, cm[MI_PK_RAW_MAX_COMMITMENTS];
    G2Aff bs;
    bool ok = g1_decode(&ar, bytes);
    ok = g2_decode(&bs, bytes + MI_PROOF_OFF_BS) && ok;
    ok = g1_decode(&krs, bytes + MI_PROOF_OFF_KRS) && ok;
    for (uint32_t k = 0; k < n_commitments; k++) ok = g1_decode(&cm[k], bytes + proof_g1_slot_offset(2 + k)) && ok;
    ok = g1_decode(&pk, bytes + proof_g1_slot_offset(2 + n_commitments)) && ok;
    if (!ok) return MI_EINVAL;
    std::memcpy(&proof->ar, &ar, sizeof(ar));
    std::memcpy(&proof->bs, &bs, sizeof(bs));
    std::memcpy(&proof->krs, &krs, sizeof(krs));
    if (n_commitments) std::memcpy(commitments, cm, (size_t)n_commitments * sizeof(G1Aff));
    std::memcpy(pok, &pk, sizeof(pk));
    return MI_OK;
}

int32_t mi_hash_to_field(const uint8_t *dst, size_t dst_len, const uint8_t *msg, size_t msg_len, mi_fr *out) {
    if (!dst || !out || (!msg && msg_len) || dst_len == 0 || dst_len > 255) return MI_EINVAL;
    const Fr v = hash_to_field(dst, (u32)dst_len, msg, msg_len);
    std::memcpy(out, &v, sizeof(v));
    return MI_OK;
}

}   // extern "C"

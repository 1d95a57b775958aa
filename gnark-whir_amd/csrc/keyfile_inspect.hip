// The host-only half of the key-file entry points (include/mi355x_groth16_keyfile.h): which encoding a stream has and where its sections
// lie, and the size of the stream a key would have.  No HIP in this file: mi_pk_stream_inspect reads bytes an outside party wrote, and
// the CPU build with -fsanitize=address,undefined (make sanitize-keyfile; tests/test_keyfile_cpu.py) compiles it with its driver
// tests/cpp/keyfile_fuzz.cpp.
#include "../../include/mi355x_groth16_keyfile.h"
#include "pk_stream_walk.h"

extern "C" {

// The counts of a stream are the same in both encodings and the bytes of a point are not, so at most one walk ends exactly at len
// (a key has five points outside the counted sections: the two sizes always differ).  The flag bits of the first point then have to
// be ones that encoding writes.
int32_t mi_pk_stream_inspect(const uint8_t *buf, size_t len, mi_pk_raw_info *info, uint32_t *encoding) {
    if (!buf || !info || !encoding) return MI_EINVAL;
    *encoding = MI_KEYFILE_RAW;
    if (pk_stream_walk(buf, len, info, 64, 128) == MI_OK) return buf[info->off_alpha1] >> 6 <= 1 ? MI_OK : MI_EINVAL;
    *encoding = MI_KEYFILE_COMPRESSED;
    if (pk_stream_walk(buf, len, info, 32, 64) == MI_OK) return buf[info->off_alpha1] >> 6 >= 1 ? MI_OK : MI_EINVAL;
    return MI_EINVAL;
}

int32_t mi_pk_stream_size(const mi_pk_desc *desc, const mi_pedersen_arrays *ped, uint32_t n_ped, uint32_t encoding, size_t *len) {
    if (!desc || !len || (!ped && n_ped) || n_ped > MI_PK_RAW_MAX_COMMITMENTS || encoding > MI_KEYFILE_COMPRESSED) return MI_EINVAL;
    const size_t g1 = encoding == MI_KEYFILE_COMPRESSED ? 32 : 64, g2 = 2 * g1, mask = (size_t)((desc->nb_wires + 7) / 8);
    size_t n = 8 + 5 * 32 + 1 + 3 * g1 + 2 * g2 + 5 * 4 + 3 * 8 + 2 * (4 + mask) + 4;
    n += (size_t)(desc->n_g1_a + desc->n_g1_b + desc->n_g1_z + desc->n_g1_k) * g1 + (size_t)desc->n_g2_b * g2;
    for (uint32_t k = 0; k < n_ped; k++) n += 2 * (4 + (size_t)ped[k].n * g1);
    *len = n;
    return MI_OK;
}

}  // extern "C"

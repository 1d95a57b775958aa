// The host-only half of include/mi355x_groth16_vkfile.h: which encoding a verifying key's stream has and where its fields lie, the size
// of the stream a key would have, and the public witness's bytes to and from Montgomery words (the body k_witness_decode runs,
// witness_ops.cuh).  No HIP call in this file: it reads bytes an outside party wrote, and the CPU build with
// -fsanitize=address,undefined (make sanitize-vkfile; tests/test_vkfile_cpu.py) compiles it with its driver tests/cpp/vkfile_fuzz.cpp.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>   // the qualifiers of MI_HD alone; nothing here calls the runtime
#endif
#include "../../include/mi355x_groth16_vkfile.h"
#include "vk_stream_walk.h"
#include "witness_ops.cuh"

static_assert(sizeof(mi_fr) == sizeof(Fr), "witness_ops.cuh writes the header's records as Fr");

extern "C" {

// The counts of a stream are the same in both encodings and the bytes of a point are not, so at most one walk ends exactly at len
// (a key has six points outside the counted section: the two sizes always differ).  The flag bits of G1.Alpha then have to be ones
// that encoding writes.
int32_t mi_vk_stream_inspect(const uint8_t *buf, size_t len, mi_vk_stream_info *info, uint32_t *encoding) {
    if (!buf || !info || !encoding) return MI_EINVAL;
    mi_vk_stream_info raw;
    size_t reached_raw = 0, reached = 0;
    *encoding = MI_KEYFILE_RAW;
    if (vk_stream_walk(buf, len, &raw, 64, 128, &reached_raw) == MI_OK) {
        *info = raw;
        if (buf[0] >> 6 <= 1) return MI_OK;
        std::snprintf(info->refused, sizeof(info->refused), "the lengths are a raw stream's, the flag bits of G1.Alpha a compressed point's");
        return MI_EINVAL;
    }
    *encoding = MI_KEYFILE_COMPRESSED;
    if (vk_stream_walk(buf, len, info, 32, 64, &reached) == MI_OK) {
        if (buf[0] >> 6 >= 1) return MI_OK;
        std::snprintf(info->refused, sizeof(info->refused), "the lengths are a compressed stream's, the flag bits of G1.Alpha a raw point's");
        return MI_EINVAL;
    }
    if (reached_raw > reached) { *info = raw; *encoding = MI_KEYFILE_RAW; }
    return MI_EINVAL;
}

int32_t mi_vk_stream_size(const mi_vk_file_desc *d, uint32_t encoding, size_t *len) {
    if (!d || !len || d->n_commitments > MI_PK_RAW_MAX_COMMITMENTS || encoding > MI_KEYFILE_COMPRESSED) return MI_EINVAL;
    const size_t g1 = encoding == MI_KEYFILE_COMPRESSED ? 32 : 64, g2 = 2 * g1;
    const size_t n_idx = d->pc_offsets ? d->pc_offsets[d->n_commitments] : 0;
    *len = 3 * g1 + 3 * g2 + 4 + (size_t)d->n_k * g1 + 4 + 4 * (size_t)d->n_commitments + 8 * n_idx + 4 + 2 * g2 * (size_t)d->n_commitments;
    return MI_OK;
}

int32_t mi_public_witness_write(const mi_fr *values, size_t n, uint8_t *out, size_t cap, size_t *len) {
    if ((!values && n) || n > 0xffffffffu) return MI_EINVAL;
    const size_t need = MI_WITNESS_HEADER_BYTES + 32 * n;
    if (len) *len = need;
    if (!out || cap < need) return MI_EINVAL;
    const uint32_t head[3] = {(uint32_t)n, 0, (uint32_t)n};
    for (int h = 0; h < 3; h++)
        for (int s = 0; s < 4; s++) out[4 * h + s] = (uint8_t)(head[h] >> (24 - 8 * s));
    for (size_t i = 0; i < n; i++) {
        Fr v;
        std::memcpy(&v, &values[i], sizeof(v));
        fe_to_be32(out + MI_WITNESS_HEADER_BYTES + 32 * i, v);
    }
    return MI_OK;
}

int32_t mi_public_witness_read(const uint8_t *bytes, size_t len, mi_fr *out, size_t cap, size_t *n_out) {
    if (n_out) *n_out = 0;
    if (!bytes || len < MI_WITNESS_HEADER_BYTES) return MI_EINVAL;
    const uint64_t n_pub = witness_be32(bytes), n_sec = witness_be32(bytes + 4), n = witness_be32(bytes + 8);
    if (n_pub + n_sec != n || (len - MI_WITNESS_HEADER_BYTES) / 32 != n || (len - MI_WITNESS_HEADER_BYTES) % 32) return MI_EINVAL;
    if (n_out) *n_out = (size_t)n_pub;
    if (cap < n_pub || (!out && n_pub)) return MI_EINVAL;
    bool ok = true;
    for (uint64_t i = 0; i < n_pub; i++) {
        Fr v;
        ok = fr_from_be32(&v, bytes + MI_WITNESS_HEADER_BYTES + 32 * i) && ok;
        std::memcpy(&out[i], &v, sizeof(v));
    }
    return ok ? MI_OK : MI_EINVAL;
}

}  // extern "C"

// keyfile.hip's bulk point kernels for vkfile.hip (not part of the C-ABI), enqueued on ctx->stream, one point per lane.  Strings are
// back to back in the given encoding, of any alignment; a decoder leaves (0, 0) for a refused string; *first_bad_dev (a device word the
// caller set to UINT64_MAX) takes the lowest refused index by atomic min.  Then the two host reads of a key's stream both loaders make.
#pragma once
#include "ctx.h"
#include "field.cuh"
#include <vector>
int32_t mi_keyfile_decode_enqueue(mi_ctx *ctx, bool g2, void *dst_dev, const uint8_t *src_dev, size_t n, bool compressed, unsigned long long *first_bad_dev);
int32_t mi_keyfile_subgroup_enqueue(mi_ctx *ctx, const void *g2_dev, size_t n, bool by_r, unsigned long long *first_bad_dev);
int32_t mi_keyfile_encode_enqueue(mi_ctx *ctx, bool g2, uint8_t *dst_dev, const void *src_dev, size_t n, bool compressed);
// one bit-packed []bool mask of an inspected stream (MSB first) -> one byte per wire
inline std::vector<uint8_t> mi_pk_stream_mask(const uint8_t *buf, uint64_t off, uint64_t nb_wires) {
    std::vector<uint8_t> m(nb_wires);
    for (uint64_t j = 0; j < nb_wires; j++) m[j] = (buf[off + j / 8] >> (7 - j % 8)) & 1;
    return m;
}
// Domain.Generator from the stream's head (after Cardinality and CardinalityInv: 32 bytes big-endian canonical) in Montgomery form
inline Fr mi_pk_stream_generator(const uint8_t *buf) {
    Fr c;
    for (int i = 0; i < 8; i++) { const uint8_t *q = buf + 8 + 32 + 28 - 4 * i; c.l[i] = ((u32)q[0] << 24) | ((u32)q[1] << 16) | ((u32)q[2] << 8) | q[3]; }
    return fe_to_mont(c);
}

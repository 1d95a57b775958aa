// keyfile.hip's bulk point kernels for vkfile.hip (not part of the C-ABI), enqueued on ctx->stream, one point per lane.  Strings are
// back to back in the given encoding, of any alignment; a decoder leaves (0, 0) for a refused string; *first_bad_dev (a device word the
// caller set to UINT64_MAX) takes the lowest refused index by atomic min.
#pragma once
#include "ctx.h"
int32_t mi_keyfile_decode_enqueue(mi_ctx *ctx, bool g2, void *dst_dev, const uint8_t *src_dev, size_t n, bool compressed, unsigned long long *first_bad_dev);
int32_t mi_keyfile_subgroup_enqueue(mi_ctx *ctx, const void *g2_dev, size_t n, bool by_r, unsigned long long *first_bad_dev);
int32_t mi_keyfile_encode_enqueue(mi_ctx *ctx, bool g2, uint8_t *dst_dev, const void *src_dev, size_t n, bool compressed);

// The host-only walk over a verifying key's stream (layout in include/mi355x_groth16_vkfile.h): offsets and counts of every field, every
// count cross-checked.  One walk for both encodings -- they differ in the bytes of a point alone -- behind mi_vk_stream_inspect
// (vkfile_inspect.hip).  No HIP here: it reads bytes an outside party wrote, and the CPU build with -fsanitize=address,undefined
// (make sanitize-vkfile) compiles it.
#pragma once
#include "../../include/mi355x_groth16_vkfile.h"
#include "pk_stream_walk.h"
#include <cstdio>

namespace {
// g1 / g2: bytes of one point.  *reached = how far the walk got (the inspector reports the refusal of the walk that got further).
inline int32_t vk_stream_walk(const uint8_t *buf, size_t len, mi_vk_stream_info *info, size_t g1, size_t g2, size_t *reached) {
    std::memset(info, 0, sizeof(*info));
    Cursor c{buf, len};
    auto refuse = [&](const char *why, uint64_t a = 0, uint64_t b = 0) {
        std::snprintf(info->refused, sizeof(info->refused), why, (unsigned long long)a, (unsigned long long)b);
        *reached = c.off;
        return MI_EINVAL;
    };
    info->off_alpha1 = c.off; c.take(g1);
    info->off_beta1 = c.off; c.take(g1);
    info->off_beta2 = c.off; c.take(g2);
    info->off_gamma2 = c.off; c.take(g2);
    info->off_delta1 = c.off; c.take(g1);
    info->off_delta2 = c.off; c.take(g2);
    if (!c.ok) return refuse("the six points of G1.Alpha .. G2.Delta do not fit");
    info->n_k = c.be(4);
    info->off_k = c.off;
    if (!c.ok || info->n_k > (len - c.off) / g1) return refuse("G1.K: n_k = %llu points do not fit", info->n_k);
    c.take((size_t)info->n_k * g1);
    info->off_lists = c.off;
    const uint64_t n_lists = c.be(4);
    if (!c.ok) return refuse("PublicAndCommitmentCommitted: the count does not fit");
    if (n_lists > MI_PK_RAW_MAX_COMMITMENTS) return refuse("PublicAndCommitmentCommitted: n_lists = %llu is above MI_PK_RAW_MAX_COMMITMENTS", n_lists);
    for (uint64_t i = 0; i < n_lists; i++) {
        info->list_len[i] = c.be(4);
        info->off_list[i] = c.off;
        if (!c.ok || info->list_len[i] > (len - c.off) / 8) return refuse("PublicAndCommitmentCommitted[%llu]: its %llu indices do not fit", i, info->list_len[i]);
        c.take((size_t)info->list_len[i] * 8);
    }
    info->off_commitment_keys = c.off;
    const uint64_t n_keys = c.be(4);
    if (!c.ok) return refuse("CommitmentKeys: the count does not fit");
    if (n_keys > MI_PK_RAW_MAX_COMMITMENTS) return refuse("CommitmentKeys: n_commitment_keys = %llu is above MI_PK_RAW_MAX_COMMITMENTS", n_keys);
    info->n_commitment_keys = (uint32_t)n_keys;
    for (uint64_t k = 0; k < n_keys; k++) {
        info->off_ped[k] = c.off;
        c.take(2 * g2);
    }
    if (!c.ok) return refuse("CommitmentKeys: %llu keys do not fit", n_keys);
    if (c.off != len) return refuse("%llu bytes follow the last field", len - c.off);   // trailing bytes = not the layout this parser knows
    // cross-checks that tie the fields together
    if (n_lists != n_keys) return refuse("n_lists = %llu is not n_commitment_keys = %llu", n_lists, n_keys);
    if (info->n_k < 1 + n_keys) return refuse("G1.K: n_k = %llu is below 1 + n_commitment_keys = %llu", info->n_k, 1 + n_keys);
    info->nb_public = (uint32_t)(info->n_k - n_keys);
    for (uint64_t i = 0; i < n_lists; i++)
        for (uint64_t t = 0; t < info->list_len[i]; t++) {
            const uint8_t *b = buf + info->off_list[i] + 8 * t;
            uint64_t v = 0;
            for (int s = 0; s < 8; s++) v = (v << 8) | b[s];
            if (v < 1 || v > (uint64_t)info->nb_public - 1 + i) {
                std::snprintf(info->refused, sizeof(info->refused), "PublicAndCommitmentCommitted[%llu][%llu] is outside 1 .. %llu", (unsigned long long)i,
                              (unsigned long long)t, (unsigned long long)(info->nb_public - 1 + i));
                *reached = c.off;
                return MI_EINVAL;
            }
        }
    *reached = c.off;
    return MI_OK;
}
}  // namespace

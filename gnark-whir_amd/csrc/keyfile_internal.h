// keyfile.hip's bulk point kernels for vkfile.hip (not part of the C-ABI), enqueued on ctx->stream, one point per lane.  Strings are
// back to back in the given encoding, of any alignment; a decoder leaves (0, 0) for a refused string; *first_bad_dev (a device word the
// caller set to UINT64_MAX) takes the lowest refused index by atomic min.  Then the two host reads of a key's stream both loaders make.
#pragma once
#include "ctx.h"
#include "field.cuh"
#include "../../include/mi355x_groth16_vkfile.h"
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
// What mi_pk_load_stream and the key audit's claim (keyaudit.hip) share: a stream in either encoding decoded into device arrays of this
// struct's own -- inspected on the host, uploaded once, every section through the decoders above, the two G2 sections through the
// membership test, ONE wait for all verdicts -- with the loader's refusals and texts.  What is still here when the struct goes is freed.
struct PkStreamDecoded {
    mi_pk_raw_info in;
    bool compressed = false;
    std::vector<uint8_t> inf_a, inf_b;                                // a byte per wire
    void *arr[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};    // mi_pk_desc's order: G1.A, G1.B, G1.K, G1.Z, G2.B
    mi_g1_affine small1[3];                                           // alpha, beta, delta
    mi_g2_affine small2[2];                                           // beta, delta
    std::vector<void *> ped;                                          // Basis, BasisExpSigma of every Pedersen key decoded
    double t0 = 0, t_up = 0, t_dec = 0, t_sub = 0;                    // the host's clock: at entry, after the upload, the decoders, the verdicts
    PkStreamDecoded() = default;
    PkStreamDecoded(const PkStreamDecoded &) = delete;
    ~PkStreamDecoded() {
        for (void *a : arr) if (a) (void)hipFree(a);
        for (void *a : ped) if (a) (void)hipFree(a);
    }
};
// with_ped: the Pedersen keys' sections are decoded too.  Resets ctx->keyfile_stats; the stream is idle on return
int32_t mi_pk_stream_decode(mi_ctx *ctx, const uint8_t *buf, size_t len, uint32_t flags, bool with_ped, PkStreamDecoded &out);
// The same for a verifying key's stream (vkfile.hip), with mi_vk_load_stream's refusals and texts, the conditions mi_vk_load puts on a
// key included.  g1 = Alpha, Beta, Delta, K[0]; g2 = Beta, Gamma, Delta, then G, GSigmaNeg of every Pedersen key; k = all of K on the
// host; k_dev = K[1 .. n_k) on the device in an allocation of (n_k - 1) * 64 + 64 bytes, freed with the struct unless taken out.
struct VkStreamDecoded {
    mi_vk_stream_info in;
    bool compressed = false;
    mi_g1_affine g1[4];
    std::vector<mi_g2_affine> g2;
    std::vector<mi_g1_affine> k;
    void *k_dev = nullptr;
    VkStreamDecoded() = default;
    VkStreamDecoded(const VkStreamDecoded &) = delete;
    ~VkStreamDecoded() { if (k_dev) (void)hipFree(k_dev); }
};
int32_t mi_vk_stream_decode(mi_ctx *ctx, const uint8_t *buf, size_t len, uint32_t flags, VkStreamDecoded &out);
// Domain.Generator from the stream's head (after Cardinality and CardinalityInv: 32 bytes big-endian canonical) in Montgomery form
inline Fr mi_pk_stream_generator(const uint8_t *buf) {
    Fr c;
    for (int i = 0; i < 8; i++) { const uint8_t *q = buf + 8 + 32 + 28 - 4 * i; c.l[i] = ((u32)q[0] << 24) | ((u32)q[1] << 16) | ((u32)q[2] << 8) | q[3]; }
    return fe_to_mont(c);
}

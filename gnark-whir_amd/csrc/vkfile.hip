// Verifying keys as files (include/mi355x_groth16_vkfile.h): the loader of gnark's raw or compressed stream and the writer of both.  The
// host-only half (which encoding, where the fields lie, the witness's bytes) is vkfile_inspect.hip; the verifier's entry points over
// witness bytes are in verify_bytes.hip, beside the decode step they extend.
//
// mi_vk_stream_decode + mi_vk_load_stream: inspect on the host, upload once, every point through the bulk decoders of keyfile.hip (keyfile_internal.h; one
// launch per run of points the stream holds back to back), every G2 point through its membership test, ONE wait for all verdicts; then
// the conditions mi_vk_load puts on a key and its own build of the resident key (mi_vk_build, verify.hip), which adopts K[1..] where the
// decoder left it.  mi_vk_write: K through the bulk encoders, the single points and the lists on the host.
#include "verify_internal.h"
#include "../../include/mi355x_groth16_vkfile.h"
#include "keyfile_ops.cuh"
#include "keyfile_internal.h"
#include "dev_arena.h"
#include <cstring>
#include <string>
#include <vector>

namespace {

void put_be(uint8_t *&p, uint64_t v, int bytes) {
    for (int i = bytes - 1; i >= 0; i--) *p++ = (uint8_t)(v >> (8 * i));
}
std::string ped_name(size_t j) { return "CommitmentKeys[" + std::to_string(j / 2) + "]." + (j % 2 ? "GSigmaNeg" : "G"); }

}  // namespace

// keyfile_internal.h: what mi_vk_load_stream and the key audit's claim (keyaudit.hip) share
int32_t mi_vk_stream_decode(mi_ctx *ctx, const uint8_t *buf, size_t len, uint32_t flags, VkStreamDecoded &out) {
    if (flags & ~(MI_KEYFILE_NO_SUBGROUP_CHECK | MI_KEYFILE_SUBGROUP_BY_R)) MI_FAIL(ctx, MI_EINVAL, "vkfile: unknown flag");
    mi_vk_stream_info &in = out.in;
    uint32_t encoding = 0;
    if (mi_vk_stream_inspect(buf, len, &in, &encoding) != MI_OK)
        MI_FAIL(ctx, MI_EINVAL, std::string("vkfile: the stream has neither the layout of VerifyingKey.WriteRawTo nor of VerifyingKey.WriteTo: ") + in.refused);
    const bool compressed = out.compressed = encoding == MI_KEYFILE_COMPRESSED;
    const uint32_t nck = in.n_commitment_keys;
    const size_t n_k = (size_t)in.n_k, n_g2 = 3 + 2 * (size_t)nck;
    // where the decoded points go: g1 = Alpha, Beta, Delta, K[0]; g2 = Beta, Gamma, Delta, then G, GSigmaNeg of every key; k = K[1..]
    G1Aff *d_g1 = nullptr;
    G2Aff *d_g2 = nullptr;
    uint8_t *raw = nullptr;
    enum { S_ALPHA_BETA1, S_BETA_GAMMA2, S_DELTA1, S_DELTA2, S_K0, S_K, S_PED, S_SUBGROUP, S_END };
    auto body = [&]() -> int32_t {
        MI_CHECK_HIP(ctx, hipMalloc((void **)&d_g1, 4 * sizeof(G1Aff)));
        MI_CHECK_HIP(ctx, hipMalloc((void **)&d_g2, n_g2 * sizeof(G2Aff)));
        MI_CHECK_HIP(ctx, hipMalloc(&out.k_dev, (n_k - 1) * sizeof(G1Aff) + 64));
        BadSlots slots;   // one word per run of points the stream holds back to back, then the membership test
        MI_TRY(slots.init(ctx, S_END));
        unsigned long long *const d_bad = slots.dev;
        const std::vector<unsigned long long> &bad = slots.host;
        MI_CHECK_HIP(ctx, hipMalloc((void **)&raw, len));
        MI_CHECK_HIP(ctx, hipMemcpyAsync(raw, buf, len, hipMemcpyHostToDevice, ctx->stream));
        const size_t g1b = MI_KEYFILE_G1_BYTES(compressed);
        G1Aff *const d_k = (G1Aff *)out.k_dev;
        MI_TRY(mi_keyfile_decode_enqueue(ctx, false, d_g1, raw + in.off_alpha1, 2, compressed, d_bad + S_ALPHA_BETA1));
        MI_TRY(mi_keyfile_decode_enqueue(ctx, true, d_g2, raw + in.off_beta2, 2, compressed, d_bad + S_BETA_GAMMA2));
        MI_TRY(mi_keyfile_decode_enqueue(ctx, false, d_g1 + 2, raw + in.off_delta1, 1, compressed, d_bad + S_DELTA1));
        MI_TRY(mi_keyfile_decode_enqueue(ctx, true, d_g2 + 2, raw + in.off_delta2, 1, compressed, d_bad + S_DELTA2));
        MI_TRY(mi_keyfile_decode_enqueue(ctx, false, d_g1 + 3, raw + in.off_k, 1, compressed, d_bad + S_K0));
        MI_TRY(mi_keyfile_decode_enqueue(ctx, false, d_k, raw + in.off_k + g1b, n_k - 1, compressed, d_bad + S_K));
        if (nck) MI_TRY(mi_keyfile_decode_enqueue(ctx, true, d_g2 + 3, raw + in.off_ped[0], 2 * (size_t)nck, compressed, d_bad + S_PED));
        if (!(flags & MI_KEYFILE_NO_SUBGROUP_CHECK))
            MI_TRY(mi_keyfile_subgroup_enqueue(ctx, d_g2, n_g2, (flags & MI_KEYFILE_SUBGROUP_BY_R) != 0, d_bad + S_SUBGROUP));
        out.g2.resize(n_g2);
        out.k.resize(n_k);
        std::vector<G2Aff> g2(n_g2);
        MI_CHECK_HIP(ctx, hipMemcpyAsync(out.g1, d_g1, sizeof(out.g1), hipMemcpyDeviceToHost, ctx->stream));
        MI_CHECK_HIP(ctx, hipMemcpyAsync(g2.data(), d_g2, n_g2 * sizeof(G2Aff), hipMemcpyDeviceToHost, ctx->stream));
        if (n_k > 1) MI_CHECK_HIP(ctx, hipMemcpyAsync(out.k.data() + 1, d_k, (n_k - 1) * sizeof(G1Aff), hipMemcpyDeviceToHost, ctx->stream));
        MI_TRY(slots.fetch(ctx));   // the one wait
        out.k[0] = out.g1[3];
        std::memcpy(out.g2.data(), g2.data(), n_g2 * sizeof(G2Aff));
        // ---- the decoders' verdicts, in stream order
        const std::string no_point = std::string(" is malformed: no point of the curve has this ") + (compressed ? "compressed" : "raw") + " encoding";
        const char *const g2_names[3] = {"G2.Beta", "G2.Gamma", "G2.Delta"};
        if (bad[S_ALPHA_BETA1] != ~0ull) MI_FAIL(ctx, MI_EINVAL, std::string("vkfile: ") + (bad[S_ALPHA_BETA1] ? "G1.Beta" : "G1.Alpha") + no_point);
        if (bad[S_BETA_GAMMA2] != ~0ull) MI_FAIL(ctx, MI_EINVAL, std::string("vkfile: ") + g2_names[bad[S_BETA_GAMMA2]] + no_point);
        if (bad[S_DELTA1] != ~0ull) MI_FAIL(ctx, MI_EINVAL, "vkfile: G1.Delta" + no_point);
        if (bad[S_DELTA2] != ~0ull) MI_FAIL(ctx, MI_EINVAL, "vkfile: G2.Delta" + no_point);
        if (bad[S_K0] != ~0ull) MI_FAIL(ctx, MI_EINVAL, "vkfile: G1.K[0]" + no_point);
        if (bad[S_K] != ~0ull) MI_FAIL(ctx, MI_EINVAL, "vkfile: G1.K[" + std::to_string(bad[S_K] + 1) + "]" + no_point);
        if (bad[S_PED] != ~0ull) MI_FAIL(ctx, MI_EINVAL, "vkfile: " + ped_name((size_t)bad[S_PED]) + no_point);
        if (bad[S_SUBGROUP] != ~0ull)
            MI_FAIL(ctx, MI_EINVAL, "vkfile: " + (bad[S_SUBGROUP] < 3 ? std::string(g2_names[bad[S_SUBGROUP]]) : ped_name((size_t)bad[S_SUBGROUP] - 3)) +
                                        " is on the twist but not in the r-torsion");
        // ---- the conditions mi_vk_load puts on a key beyond its points' membership
        if (g2[1].is_inf()) MI_FAIL(ctx, MI_EINVAL, "vkfile: G2.Gamma is infinity");
        if (g2[2].is_inf()) MI_FAIL(ctx, MI_EINVAL, "vkfile: G2.Delta is infinity");
        for (uint32_t c = 0; c < nck; c++) {
            if (std::memcmp(&g2[3 + 2 * c], &g2[3], sizeof(G2Aff)) != 0) MI_FAIL(ctx, MI_EINVAL, "vkfile: the Pedersen keys do not share one G (" + ped_name(2 * c) + ")");
            if (g2[3 + 2 * c].is_inf()) MI_FAIL(ctx, MI_EINVAL, "vkfile: " + ped_name(2 * c) + " is infinity");
        }
        return MI_OK;
    };
    const int32_t rc = body();
    (void)hipStreamSynchronize(ctx->stream);
    for (void *a : {(void *)d_g1, (void *)d_g2, (void *)raw})
        if (a) (void)hipFree(a);
    return rc;
}

extern "C" {

int32_t mi_vk_load_stream(mi_ctx *ctx, const uint8_t *buf, size_t len, uint32_t flags, mi_vk **out) {
    if (!ctx) return MI_EINVAL;
    if (!buf || !out) MI_FAIL(ctx, MI_EINVAL, "vkfile: null stream or output pointer");
    *out = nullptr;
    VkStreamDecoded dec;
    auto body = [&]() -> int32_t {
        MI_TRY(mi_vk_stream_decode(ctx, buf, len, flags, dec));
        const mi_vk_stream_info &in = dec.in;
        const uint32_t nck = in.n_commitment_keys;
        // ---- the resident key, as mi_vk_load builds it, and the lists
        mi_vk_desc d;
        std::memset(&d, 0, sizeof(d));
        d.alpha1 = dec.g1[0];
        d.beta2 = dec.g2[0]; d.gamma2 = dec.g2[1]; d.delta2 = dec.g2[2];
        d.k = dec.k.data(); d.n_k = in.n_k; d.nb_public = in.nb_public; d.n_commitments = nck;
        d.ped = nck ? (const mi_pedersen_vk *)&dec.g2[3] : nullptr;
        G1Aff *adopt = (G1Aff *)dec.k_dev;
        dec.k_dev = nullptr;   // the key owns it from here, whatever mi_vk_build returns
        MI_TRY(mi_vk_build(ctx, &d, adopt, out));
        std::vector<uint32_t> off(nck + 1, 0), idx;
        for (uint32_t c = 0; c < nck; c++) {
            off[c + 1] = off[c] + (uint32_t)in.list_len[c];
            for (uint64_t t = 0; t < in.list_len[c]; t++) {
                const uint8_t *b = buf + in.off_list[c] + 8 * t + 4;   // below 2^32: the inspector has seen to it
                idx.push_back(((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | b[3]);
            }
        }
        return mi_vk_set_public_committed(ctx, *out, off.data(), idx.data());
    };
    const int32_t rc = body();
    (void)hipStreamSynchronize(ctx->stream);
    if (rc != MI_OK && *out) { (void)mi_vk_free(ctx, *out); *out = nullptr; }
    return rc;
}

int32_t mi_vk_write(mi_ctx *ctx, const mi_vk_file_desc *d, uint32_t encoding, uint8_t *out_host, size_t cap, size_t *len) {
    if (!ctx) return MI_EINVAL;
    size_t need = 0;
    if (mi_vk_stream_size(d, encoding, &need) != MI_OK) MI_FAIL(ctx, MI_EINVAL, "vkfile: write: null desc, more than MI_PK_RAW_MAX_COMMITMENTS Pedersen keys, or an unknown encoding");
    if (len) *len = need;
    if (!out_host || cap < need) MI_FAIL(ctx, MI_EINVAL, "vkfile: write: the stream takes " + std::to_string(need) + " bytes, out_host has room for " + std::to_string(out_host ? cap : 0));
    const uint32_t nc = d->n_commitments;
    if (!d->k || d->nb_public == 0 || d->n_k != (uint64_t)d->nb_public + nc || d->n_k > 0xffffffffu) MI_FAIL(ctx, MI_EINVAL, "vkfile: write: k is null, nb_public is 0 or n_k is not nb_public + n_commitments");
    if (nc && !d->ped) MI_FAIL(ctx, MI_EINVAL, "vkfile: write: ped is null");
    const uint32_t zero_off[MI_PK_RAW_MAX_COMMITMENTS + 1] = {0};
    const uint32_t *off = d->pc_offsets ? d->pc_offsets : zero_off;
    if (off[0] != 0 || (off[nc] && !d->pc_indices)) MI_FAIL(ctx, MI_EINVAL, "vkfile: write: pc_offsets[0] is not 0, or pc_indices is null");
    for (uint32_t i = 0; i < nc; i++) {
        if (off[i + 1] < off[i]) MI_FAIL(ctx, MI_EINVAL, "vkfile: write: pc_offsets do not ascend");
        for (uint32_t t = off[i]; t < off[i + 1]; t++)
            if (d->pc_indices[t] < 1 || d->pc_indices[t] > d->nb_public - 1 + i)
                MI_FAIL(ctx, MI_EINVAL, "vkfile: write: pc_indices[" + std::to_string(t) + "] of commitment " + std::to_string(i) + " is outside 1 .. " + std::to_string(d->nb_public - 1 + i));
    }
    const bool compressed = encoding == MI_KEYFILE_COMPRESSED;
    const size_t g1b = MI_KEYFILE_G1_BYTES(compressed), g2b = MI_KEYFILE_G2_BYTES(compressed), n_k = (size_t)d->n_k;
    // K first: up, through the bulk encoder, back to the host.  Only this step can fail, and out_host is not touched before it has passed.
    std::vector<uint8_t> k_enc(n_k * g1b);
    G1Aff *d_k = nullptr;
    uint8_t *d_enc = nullptr;
    auto body = [&]() -> int32_t {
        MI_CHECK_HIP(ctx, hipMalloc((void **)&d_k, n_k * sizeof(G1Aff)));
        MI_CHECK_HIP(ctx, hipMalloc((void **)&d_enc, n_k * g1b));
        MI_CHECK_HIP(ctx, hipMemcpyAsync(d_k, d->k, n_k * sizeof(G1Aff), hipMemcpyHostToDevice, ctx->stream));
        MI_TRY(mi_keyfile_encode_enqueue(ctx, false, d_enc, d_k, n_k, compressed));
        MI_CHECK_HIP(ctx, hipMemcpyAsync(k_enc.data(), d_enc, n_k * g1b, hipMemcpyDeviceToHost, ctx->stream));
        MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return MI_OK;
    };
    const int32_t rc = body();
    (void)hipStreamSynchronize(ctx->stream);
    if (d_k) (void)hipFree(d_k);
    if (d_enc) (void)hipFree(d_enc);
    MI_TRY(rc);
    uint8_t *p = out_host;
    auto g1 = [&](const mi_g1_affine &q) { G1Aff a; std::memcpy(&a, &q, sizeof(a)); g1_encode_stream(p, a, compressed); p += g1b; };
    auto g2 = [&](const mi_g2_affine &q) { G2Aff a; std::memcpy(&a, &q, sizeof(a)); g2_encode_stream(p, a, compressed); p += g2b; };
    g1(d->alpha1); g1(d->beta1); g2(d->beta2); g2(d->gamma2); g1(d->delta1); g2(d->delta2);
    put_be(p, n_k, 4);
    std::memcpy(p, k_enc.data(), k_enc.size());
    p += k_enc.size();
    put_be(p, nc, 4);
    for (uint32_t i = 0; i < nc; i++) {
        put_be(p, off[i + 1] - off[i], 4);
        for (uint32_t t = off[i]; t < off[i + 1]; t++) put_be(p, d->pc_indices[t], 8);
    }
    put_be(p, nc, 4);
    for (uint32_t c = 0; c < nc; c++) { g2(d->ped[c].g); g2(d->ped[c].g_sigma_neg); }
    if ((size_t)(p - out_host) != need) MI_FAIL(ctx, MI_EHIP, "vkfile: write: the stream written does not have the size computed for it");
    return MI_OK;
}

}  // extern "C"

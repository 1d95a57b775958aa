// Proving keys as files (include/mi355x_groth16_keyfile.h): the bulk point codecs, the loader of gnark's raw or compressed stream and the
// writer of both.  The host-only half (which encoding, where the sections lie, how long a stream is) is keyfile_inspect.hip.
//
// One lane handles one point and runs the text of keyfile_ops.cuh:
//   k_keyfile_decode_g1 / _g2 _compressed / _raw   a section's strings -> affine Montgomery points; a refused string leaves (0, 0) and its
//                                           index in *first_bad by atomic min, so the LOWEST bad index of a section comes back
//   k_keyfile_subgroup_psi / _by_r          decoded G2 points -> the same for membership of the r-torsion (the endomorphism test; by_r:
//                                           g2_in_subgroup's [r] Q, kept for the measurement in profiles/keyfile.txt)
//   k_keyfile_encode_g1 / _g2 _compressed / _raw   the way back
// The membership test is a kernel of its own rather than the tail of the G2 decoder: its 63-step scalar multiple holds a G2 point in
// extended coordinates where the decoder holds its table of fifteen powers, and apart each is timed (mi_keyfile_stats).
//
// mi_pk_stream_decode (keyfile_internal.h): inspect on the host, upload once, decode every section straight into the array the key will
// own, ONE wait for all verdicts.  mi_pk_load_stream: that, then the handover of key_handover.h (mi_pk_load_range / mi_pedersen_pk_adopt);
// the key audit's claim (keyaudit.hip) stops before the handover.  mi_pk_write_dev: the sections are encoded
// on the device and copied into place; the Domain block, the counts and the masks are host code and follow oracle/pk_raw.py.
#include "prove_internal.h"
#include "keyfile_ops.cuh"
#include "keyfile_internal.h"
#include "key_handover.h"   // dev_arena.h: BadSlots
#include <cstring>
#include <string>
#include <vector>

namespace {

typedef unsigned long long ull;
constexpr unsigned KF_BLOCK = 128;

// one lane of each kernel; the kernels below are these bodies under plain names (a template's name carries its whole signature into
// every trace and resource table)
template <bool COMPRESSED>
MI_D void lane_decode_g1(G1Aff *dst, const uint8_t *src, size_t n, ull *first_bad) {
    const size_t i = (size_t)blockIdx.x * KF_BLOCK + threadIdx.x;
    if (i >= n) return;
    G1Aff p;
    const bool ok = g1_decode_stream(&p, src + (size_t)MI_KEYFILE_G1_BYTES(COMPRESSED) * i, COMPRESSED);
    dst[i] = p;
    if (!ok) atomicMin(first_bad, (ull)i);
}
template <bool COMPRESSED>
MI_D void lane_decode_g2(G2Aff *dst, const uint8_t *src, size_t n, ull *first_bad) {
    const size_t i = (size_t)blockIdx.x * KF_BLOCK + threadIdx.x;
    if (i >= n) return;
    G2Aff q;
    const bool ok = g2_decode_stream(&q, src + (size_t)MI_KEYFILE_G2_BYTES(COMPRESSED) * i, COMPRESSED);
    dst[i] = q;
    if (!ok) atomicMin(first_bad, (ull)i);
}
// pts: points of the twist (what a decoder wrote)
template <bool BY_R>
MI_D void lane_subgroup(const G2Aff *pts, size_t n, ull *first_bad) {
    const size_t i = (size_t)blockIdx.x * KF_BLOCK + threadIdx.x;
    if (i >= n) return;
    const G2Aff q = pts[i];
    const bool ok = BY_R ? g2_in_subgroup(&q) : g2_in_subgroup_psi(&q);
    if (!ok) atomicMin(first_bad, (ull)i);
}
template <bool COMPRESSED>
MI_D void lane_encode_g1(uint8_t *dst, const G1Aff *src, size_t n) {
    const size_t i = (size_t)blockIdx.x * KF_BLOCK + threadIdx.x;
    if (i < n) g1_encode_stream(dst + (size_t)MI_KEYFILE_G1_BYTES(COMPRESSED) * i, src[i], COMPRESSED);
}
template <bool COMPRESSED>
MI_D void lane_encode_g2(uint8_t *dst, const G2Aff *src, size_t n) {
    const size_t i = (size_t)blockIdx.x * KF_BLOCK + threadIdx.x;
    if (i < n) g2_encode_stream(dst + (size_t)MI_KEYFILE_G2_BYTES(COMPRESSED) * i, src[i], COMPRESSED);
}
#define KF_KERNEL __global__ void __launch_bounds__(KF_BLOCK)
KF_KERNEL k_keyfile_decode_g1_compressed(G1Aff *dst, const uint8_t *src, size_t n, ull *first_bad) { lane_decode_g1<true>(dst, src, n, first_bad); }
KF_KERNEL k_keyfile_decode_g1_raw(G1Aff *dst, const uint8_t *src, size_t n, ull *first_bad) { lane_decode_g1<false>(dst, src, n, first_bad); }
KF_KERNEL k_keyfile_decode_g2_compressed(G2Aff *dst, const uint8_t *src, size_t n, ull *first_bad) { lane_decode_g2<true>(dst, src, n, first_bad); }
KF_KERNEL k_keyfile_decode_g2_raw(G2Aff *dst, const uint8_t *src, size_t n, ull *first_bad) { lane_decode_g2<false>(dst, src, n, first_bad); }
KF_KERNEL k_keyfile_subgroup_psi(const G2Aff *pts, size_t n, ull *first_bad) { lane_subgroup<false>(pts, n, first_bad); }
KF_KERNEL k_keyfile_subgroup_by_r(const G2Aff *pts, size_t n, ull *first_bad) { lane_subgroup<true>(pts, n, first_bad); }
KF_KERNEL k_keyfile_encode_g1_compressed(uint8_t *dst, const G1Aff *src, size_t n) { lane_encode_g1<true>(dst, src, n); }
KF_KERNEL k_keyfile_encode_g1_raw(uint8_t *dst, const G1Aff *src, size_t n) { lane_encode_g1<false>(dst, src, n); }
KF_KERNEL k_keyfile_encode_g2_compressed(uint8_t *dst, const G2Aff *src, size_t n) { lane_encode_g2<true>(dst, src, n); }
KF_KERNEL k_keyfile_encode_g2_raw(uint8_t *dst, const G2Aff *src, size_t n) { lane_encode_g2<false>(dst, src, n); }

#define KF_LAUNCH(ctx, kernel, n, ...)                                                                                        \
    do {                                                                                                                      \
        if (n) hipLaunchKernelGGL(kernel, dim3(mi_blocks_of((n), KF_BLOCK)), dim3(KF_BLOCK), 0, (ctx)->stream, __VA_ARGS__);  \
        MI_CHECK_HIP(ctx, hipGetLastError());                                                                                 \
    } while (0)

int32_t decode_g1(mi_ctx *ctx, void *dst, const uint8_t *src, size_t n, bool compressed, ull *bad) {
    if (compressed) KF_LAUNCH(ctx, k_keyfile_decode_g1_compressed, n, (G1Aff *)dst, src, n, bad);
    else KF_LAUNCH(ctx, k_keyfile_decode_g1_raw, n, (G1Aff *)dst, src, n, bad);
    return MI_OK;
}
int32_t decode_g2(mi_ctx *ctx, void *dst, const uint8_t *src, size_t n, bool compressed, ull *bad) {
    if (compressed) KF_LAUNCH(ctx, k_keyfile_decode_g2_compressed, n, (G2Aff *)dst, src, n, bad);
    else KF_LAUNCH(ctx, k_keyfile_decode_g2_raw, n, (G2Aff *)dst, src, n, bad);
    return MI_OK;
}
int32_t subgroup_g2(mi_ctx *ctx, const void *pts, size_t n, bool by_r, ull *bad) {
    if (by_r) KF_LAUNCH(ctx, k_keyfile_subgroup_by_r, n, (const G2Aff *)pts, n, bad);
    else KF_LAUNCH(ctx, k_keyfile_subgroup_psi, n, (const G2Aff *)pts, n, bad);
    return MI_OK;
}
int32_t encode_g1(mi_ctx *ctx, uint8_t *dst, const void *src, size_t n, bool compressed) {
    if (compressed) KF_LAUNCH(ctx, k_keyfile_encode_g1_compressed, n, dst, (const G1Aff *)src, n);
    else KF_LAUNCH(ctx, k_keyfile_encode_g1_raw, n, dst, (const G1Aff *)src, n);
    return MI_OK;
}
int32_t encode_g2(mi_ctx *ctx, uint8_t *dst, const void *src, size_t n, bool compressed) {
    if (compressed) KF_LAUNCH(ctx, k_keyfile_encode_g2_compressed, n, dst, (const G2Aff *)src, n);
    else KF_LAUNCH(ctx, k_keyfile_encode_g2_raw, n, dst, (const G2Aff *)src, n);
    return MI_OK;
}

// n strings of one group -> points, and the lowest refused index
int32_t decompress(mi_ctx *ctx, bool g2, const uint8_t *bytes_dev, size_t n, uint32_t flags, void *out_dev, uint64_t *first_bad) {
    if (!ctx) return MI_EINVAL;
    if (first_bad) *first_bad = UINT64_MAX;
    if ((!bytes_dev || !out_dev) && n) MI_FAIL(ctx, MI_EINVAL, "keyfile: decompress: null pointer");
    if (flags & ~(MI_KEYFILE_NO_SUBGROUP_CHECK | MI_KEYFILE_SUBGROUP_BY_R)) MI_FAIL(ctx, MI_EINVAL, "keyfile: decompress: unknown flag");
    BadSlots bad;
    MI_TRY(bad.init(ctx, 2));
    if (g2) {
        MI_TRY(decode_g2(ctx, out_dev, bytes_dev, n, true, bad.dev));
        if (!(flags & MI_KEYFILE_NO_SUBGROUP_CHECK)) MI_TRY(subgroup_g2(ctx, out_dev, n, (flags & MI_KEYFILE_SUBGROUP_BY_R) != 0, bad.dev + 1));
    } else MI_TRY(decode_g1(ctx, out_dev, bytes_dev, n, true, bad.dev));
    MI_TRY(bad.fetch(ctx));
    const ull lowest = bad.host[0] < bad.host[1] ? bad.host[0] : bad.host[1];
    if (first_bad) *first_bad = lowest;
    if (lowest == ~0ull) return MI_OK;
    MI_FAIL(ctx, MI_EINVAL, std::string("keyfile: ") + (g2 ? "G2" : "G1") + " point " + std::to_string(lowest) +
                                (bad.host[0] <= bad.host[1] ? " is malformed" : " is not in the r-torsion"));
}
int32_t compress(mi_ctx *ctx, bool g2, const void *pts_dev, size_t n, uint32_t encoding, uint8_t *bytes_dev) {
    if (!ctx) return MI_EINVAL;
    if ((!pts_dev || !bytes_dev) && n) MI_FAIL(ctx, MI_EINVAL, "keyfile: compress: null pointer");
    if (encoding > MI_KEYFILE_COMPRESSED) MI_FAIL(ctx, MI_EINVAL, "keyfile: compress: encoding is neither MI_KEYFILE_RAW nor MI_KEYFILE_COMPRESSED");
    MI_TRY(g2 ? encode_g2(ctx, bytes_dev, pts_dev, n, encoding == MI_KEYFILE_COMPRESSED) : encode_g1(ctx, bytes_dev, pts_dev, n, encoding == MI_KEYFILE_COMPRESSED));
    MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MI_OK;
}

// one Fr / one count of the host half of a stream
void put_be(uint8_t *&p, uint64_t v, int bytes) {
    for (int i = bytes - 1; i >= 0; i--) *p++ = (uint8_t)(v >> (8 * i));
}
void put_fr(uint8_t *&p, const Fr &mont) {
    fe_to_be32(p, mont);
    p += 32;
}

}  // namespace

// keyfile_internal.h: the same launches for the verifying key's stream (vkfile.hip)
int32_t mi_keyfile_decode_enqueue(mi_ctx *ctx, bool g2, void *dst_dev, const uint8_t *src_dev, size_t n, bool compressed, ull *first_bad_dev) {
    return g2 ? decode_g2(ctx, dst_dev, src_dev, n, compressed, first_bad_dev) : decode_g1(ctx, dst_dev, src_dev, n, compressed, first_bad_dev);
}
int32_t mi_keyfile_subgroup_enqueue(mi_ctx *ctx, const void *g2_dev, size_t n, bool by_r, ull *first_bad_dev) { return subgroup_g2(ctx, g2_dev, n, by_r, first_bad_dev); }
int32_t mi_keyfile_encode_enqueue(mi_ctx *ctx, bool g2, uint8_t *dst_dev, const void *src_dev, size_t n, bool compressed) {
    return g2 ? encode_g2(ctx, dst_dev, src_dev, n, compressed) : encode_g1(ctx, dst_dev, src_dev, n, compressed);
}

int32_t mi_pk_stream_decode(mi_ctx *ctx, const uint8_t *buf, size_t len, uint32_t flags, bool with_ped, PkStreamDecoded &out) {
    if (flags & ~(MI_KEYFILE_NO_SUBGROUP_CHECK | MI_KEYFILE_SUBGROUP_BY_R)) MI_FAIL(ctx, MI_EINVAL, "keyfile: unknown flag");
    mi_pk_raw_info &in = out.in;
    uint32_t encoding = 0;
    if (mi_pk_stream_inspect(buf, len, &in, &encoding) != MI_OK)
        MI_FAIL(ctx, MI_EINVAL, "keyfile: the stream has neither the layout of ProvingKey.WriteRawTo nor of ProvingKey.WriteTo (include/mi355x_groth16_keyfile.h)");
    const bool compressed = out.compressed = encoding == MI_KEYFILE_COMPRESSED;
    // the domain's generator must be the one fft.NewDomain derives for this size (a cheap canary for a shifted layout)
    if (mi_pk_stream_generator(buf) != fr_domain_generator(in.log_n)) MI_FAIL(ctx, MI_EINVAL, "keyfile: Domain.Generator is not fft.NewDomain's for this cardinality");
    ctx->keyfile_stats = mi_keyfile_stats{};
    out.t0 = now_ms();
    out.inf_a = mi_pk_stream_mask(buf, in.off_infinity_a, in.nb_wires);
    out.inf_b = mi_pk_stream_mask(buf, in.off_infinity_b, in.nb_wires);
    const uint32_t n_ped = with_ped ? in.n_commitment_keys : 0;
    out.ped.assign(2 * (size_t)n_ped, nullptr);
    // every section, in stream order: where it lies, where it goes
    struct Section { std::string name; bool g2; uint64_t off, n; void *dst; };
    void *d_small1 = nullptr, *d_small2 = nullptr, *raw = nullptr;
    auto body = [&]() -> int32_t {
        std::vector<Section> sec = {{"G1.AlphaBetaDelta", false, in.off_alpha1, 3, nullptr}, {"G1.A", false, in.off_g1_a, in.n_g1_a, nullptr},
                                    {"G1.B", false, in.off_g1_b, in.n_g1_b, nullptr},        {"G1.Z", false, in.off_g1_z, in.n_g1_z, nullptr},
                                    {"G1.K", false, in.off_g1_k, in.n_g1_k, nullptr},        {"G2.BetaDelta", true, in.off_beta2, 2, nullptr},
                                    {"G2.B", true, in.off_g2_b, in.n_g2_b, nullptr}};
        for (uint32_t k = 0; k < n_ped; k++) {
            sec.push_back({"Basis[" + std::to_string(k) + "]", false, in.off_basis[k], in.n_basis[k], nullptr});
            sec.push_back({"BasisExpSigma[" + std::to_string(k) + "]", false, in.off_basis_exp_sigma[k], in.n_basis[k], nullptr});
        }
        void **const home[7] = {&d_small1, &out.arr[0], &out.arr[1], &out.arr[3], &out.arr[2], &d_small2, &out.arr[4]};
        for (size_t s = 0; s < sec.size(); s++) {
            void **h = s < 7 ? home[s] : &out.ped[s - 7];
            const size_t bytes = (size_t)sec[s].n * (sec[s].g2 ? 128 : 64);
            MI_CHECK_HIP(ctx, hipMalloc(h, bytes ? bytes : 64));
            sec[s].dst = *h;
        }
        BadSlots bad;   // one word per section, then the membership tests of the two G2 sections
        MI_TRY(bad.init(ctx, sec.size() + 2));
        MI_CHECK_HIP(ctx, hipMalloc(&raw, len));
        MI_CHECK_HIP(ctx, hipMemcpyAsync(raw, buf, len, hipMemcpyHostToDevice, ctx->stream));
        MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        out.t_up = now_ms();
        for (size_t s = 0; s < sec.size(); s++) {
            const uint8_t *src = (const uint8_t *)raw + sec[s].off;
            MI_TRY(sec[s].g2 ? decode_g2(ctx, sec[s].dst, src, (size_t)sec[s].n, compressed, bad.dev + s) : decode_g1(ctx, sec[s].dst, src, (size_t)sec[s].n, compressed, bad.dev + s));
        }
        MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        out.t_dec = now_ms();
        if (!(flags & MI_KEYFILE_NO_SUBGROUP_CHECK))
            for (int k = 0; k < 2; k++) MI_TRY(subgroup_g2(ctx, sec[5 + k].dst, (size_t)sec[5 + k].n, (flags & MI_KEYFILE_SUBGROUP_BY_R) != 0, bad.dev + sec.size() + k));
        MI_CHECK_HIP(ctx, hipMemcpyAsync(out.small1, d_small1, 3 * sizeof(G1Aff), hipMemcpyDeviceToHost, ctx->stream));
        MI_CHECK_HIP(ctx, hipMemcpyAsync(out.small2, d_small2, 2 * sizeof(G2Aff), hipMemcpyDeviceToHost, ctx->stream));
        MI_TRY(bad.fetch(ctx));
        out.t_sub = now_ms();
        (void)hipFree(raw); raw = nullptr;   // the stream has been read
        for (size_t s = 0; s < sec.size(); s++)
            if (bad.host[s] != ~0ull) MI_FAIL(ctx, MI_EINVAL, "keyfile: " + sec[s].name + "[" + std::to_string(bad.host[s]) + "] is malformed: no point of the curve has this " + (compressed ? "compressed" : "raw") + " encoding");
        for (int k = 0; k < 2; k++)
            if (bad.host[sec.size() + k] != ~0ull) MI_FAIL(ctx, MI_EINVAL, "keyfile: " + sec[5 + k].name + "[" + std::to_string(bad.host[sec.size() + k]) + "] is on the twist but not in the r-torsion");
        ctx->keyfile_stats = mi_keyfile_stats{(float)(out.t_up - out.t0), (float)(out.t_dec - out.t_up), (float)(out.t_sub - out.t_dec), 0.f, (float)(out.t_sub - out.t0)};   // a loader adds its build
        return MI_OK;
    };
    const int32_t rc = body();
    (void)hipStreamSynchronize(ctx->stream);
    for (void *a : {raw, d_small1, d_small2}) if (a) (void)hipFree(a);
    return rc;
}

extern "C" {

int32_t mi_g1_decompress_dev(mi_ctx *ctx, const uint8_t *bytes_dev, size_t n, mi_g1_affine *out_dev, uint64_t *first_bad) {
    return decompress(ctx, false, bytes_dev, n, 0, out_dev, first_bad);
}
int32_t mi_g2_decompress_dev(mi_ctx *ctx, const uint8_t *bytes_dev, size_t n, uint32_t flags, mi_g2_affine *out_dev, uint64_t *first_bad) {
    return decompress(ctx, true, bytes_dev, n, flags, out_dev, first_bad);
}
int32_t mi_g1_compress_dev(mi_ctx *ctx, const mi_g1_affine *pts_dev, size_t n, uint32_t encoding, uint8_t *bytes_dev) {
    return compress(ctx, false, pts_dev, n, encoding, bytes_dev);
}
int32_t mi_g2_compress_dev(mi_ctx *ctx, const mi_g2_affine *pts_dev, size_t n, uint32_t encoding, uint8_t *bytes_dev) {
    return compress(ctx, true, pts_dev, n, encoding, bytes_dev);
}
int32_t mi_keyfile_get_stats(mi_ctx *ctx, mi_keyfile_stats *out) {
    if (!ctx || !out) return MI_EINVAL;
    *out = ctx->keyfile_stats;
    return MI_OK;
}

int32_t mi_pk_load_stream(mi_ctx *ctx, const uint8_t *buf, size_t len, uint32_t flags, uint32_t nb_public, const uint32_t *committed_wires,
                          size_t n_committed, mi_pk **out, mi_pedersen_pk **ped_out, uint32_t *n_ped_out) {
    if (!ctx || !buf || !out) return MI_EINVAL;
    *out = nullptr;
    if (n_ped_out) *n_ped_out = 0;
    PkStreamDecoded dec;
    KeyHandover hand(ctx, out, ped_out);
    uint32_t n_ped = 0;
    auto body = [&]() -> int32_t {
        MI_TRY(mi_pk_stream_decode(ctx, buf, len, flags, ped_out != nullptr, dec));
        const mi_pk_raw_info &in = dec.in;
        n_ped = (uint32_t)(dec.ped.size() / 2);
        KeyArrays ka(in.log_n, nb_public, in.nb_wires, dec.inf_a.data(), dec.inf_b.data(), committed_wires, n_committed);   // the arrays are this call's own until the key takes them
        ka.n[KEY_G1_A] = in.n_g1_a; ka.n[KEY_G1_B] = in.n_g1_b; ka.n[KEY_G1_K] = in.n_g1_k; ka.n[KEY_G1_Z] = in.n_g1_z; ka.n[KEY_G2_B] = in.n_g2_b;
        for (int i = 0; i < KEY_ARRAYS; i++) ka.arr[i] = dec.arr[i];
        std::memcpy(ka.small1, dec.small1, sizeof(dec.small1));
        std::memcpy(ka.small2, dec.small2, sizeof(dec.small2));
        const int32_t rc = hand.adopt_key(ka, nullptr);
        for (int i = 0; i < KEY_ARRAYS; i++) dec.arr[i] = ka.arr[i];   // what the key took is no longer this call's
        MI_TRY(rc);
        for (uint32_t k = 0; k < n_ped; k++) MI_TRY(hand.adopt_pedersen(&dec.ped[2 * k], &dec.ped[2 * k + 1], (size_t)in.n_basis[k], nullptr));
        MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        const double t_end = now_ms();
        ctx->keyfile_stats = mi_keyfile_stats{(float)(dec.t_up - dec.t0), (float)(dec.t_dec - dec.t_up), (float)(dec.t_sub - dec.t_dec), (float)(t_end - dec.t_sub), (float)(t_end - dec.t0)};
        return MI_OK;
    };
    const int32_t rc = body();
    (void)hipStreamSynchronize(ctx->stream);
    if (rc == MI_OK) {
        hand.dismiss();
        if (n_ped_out) *n_ped_out = n_ped;
    }
    return rc;
}

int32_t mi_pk_write_dev(mi_ctx *ctx, const mi_pk_desc *d, const mi_pedersen_arrays *ped, uint32_t n_ped, uint32_t encoding, uint8_t *out_host,
                        size_t cap, size_t *len) {
    if (!ctx) return MI_EINVAL;
    size_t need = 0;
    if (mi_pk_stream_size(d, ped, n_ped, encoding, &need) != MI_OK) MI_FAIL(ctx, MI_EINVAL, "keyfile: write: null desc, more than MI_PK_RAW_MAX_COMMITMENTS Pedersen keys, or an unknown encoding");
    if (len) *len = need;
    if (!out_host || cap < need) MI_FAIL(ctx, MI_EINVAL, "keyfile: write: the stream takes " + std::to_string(need) + " bytes, out_host has room for " + std::to_string(out_host ? cap : 0));
    if (d->log_n > 28 || (!d->infinity_a || !d->infinity_b) && d->nb_wires) MI_FAIL(ctx, MI_EINVAL, "keyfile: write: log_n > 28 or a null infinity mask");
    const struct { const void *p; uint64_t n; } arr[5] = {{d->g1_a, d->n_g1_a}, {d->g1_b, d->n_g1_b}, {d->g1_z, d->n_g1_z}, {d->g1_k, d->n_g1_k}, {d->g2_b, d->n_g2_b}};
    for (const auto &a : arr) if (!a.p && a.n) MI_FAIL(ctx, MI_EINVAL, "keyfile: write: a null point array with a count that is not 0");
    for (uint32_t k = 0; k < n_ped; k++) if ((!ped[k].basis_dev || !ped[k].basis_exp_sigma_dev) && ped[k].n) MI_FAIL(ctx, MI_EINVAL, "keyfile: write: a null Pedersen array");
    const bool compressed = encoding == MI_KEYFILE_COMPRESSED;
    const size_t g1b = MI_KEYFILE_G1_BYTES(compressed), g2b = MI_KEYFILE_G2_BYTES(compressed);
    ctx->keyfile_stats = mi_keyfile_stats{};
    const double t0 = now_ms();
    // the point sections, in stream order, back to back in one device buffer
    struct Section { const void *src; uint64_t n; bool g2; size_t at; };
    std::vector<Section> sec;
    size_t staged = 0;
    auto add = [&](const void *src, uint64_t n, bool g2) { sec.push_back({src, n, g2, staged}); staged += (size_t)n * (g2 ? g2b : g1b); };
    add(d->g1_a, d->n_g1_a, false); add(d->g1_b, d->n_g1_b, false); add(d->g1_z, d->n_g1_z, false); add(d->g1_k, d->n_g1_k, false); add(d->g2_b, d->n_g2_b, true);
    for (uint32_t k = 0; k < n_ped; k++) { add(ped[k].basis_dev, ped[k].n, false); add(ped[k].basis_exp_sigma_dev, ped[k].n, false); }
    uint8_t *stage = nullptr;
    auto body = [&]() -> int32_t {
        MI_CHECK_HIP(ctx, hipMalloc((void **)&stage, staged ? staged : 64));
        for (const Section &s : sec) MI_TRY(s.g2 ? encode_g2(ctx, stage + s.at, s.src, (size_t)s.n, compressed) : encode_g1(ctx, stage + s.at, s.src, (size_t)s.n, compressed));
        MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        const double t_enc = now_ms();
        // the host half follows oracle/pk_raw.py; the sections are copied into place as the walk reaches them
        uint8_t *p = out_host;
        size_t next = 0;
        auto section = [&]() -> int32_t {
            const Section &s = sec[next++];
            const size_t bytes = (size_t)s.n * (s.g2 ? g2b : g1b);
            put_be(p, s.n, 4);
            if (bytes) MI_CHECK_HIP(ctx, hipMemcpyAsync(p, stage + s.at, bytes, hipMemcpyDeviceToHost, ctx->stream));
            p += bytes;
            return MI_OK;
        };
        const Fr gen = fr_domain_generator(d->log_n), card = fe_to_mont(Fr{{(u32)1 << d->log_n, 0, 0, 0, 0, 0, 0, 0}}), five = fe_from_u32<FrParams>(5);
        put_be(p, (uint64_t)1 << d->log_n, 8);
        put_fr(p, fe_inv(card)); put_fr(p, gen); put_fr(p, fe_inv(gen)); put_fr(p, five); put_fr(p, fe_inv(five));
        *p++ = 1;   // withPrecompute
        G1Aff s1[3];
        G2Aff s2[2];
        std::memcpy(&s1[0], &d->alpha1, 64); std::memcpy(&s1[1], &d->beta1, 64); std::memcpy(&s1[2], &d->delta1, 64);
        std::memcpy(&s2[0], &d->beta2, 128); std::memcpy(&s2[1], &d->delta2, 128);
        for (const G1Aff &q : s1) { g1_encode_stream(p, q, compressed); p += g1b; }
        for (int k = 0; k < 4; k++) MI_TRY(section());
        for (const G2Aff &q : s2) { g2_encode_stream(p, q, compressed); p += g2b; }
        MI_TRY(section());
        uint64_t n_inf[2] = {0, 0};
        const uint8_t *mask[2] = {d->infinity_a, d->infinity_b};
        for (int m = 0; m < 2; m++) for (uint64_t j = 0; j < d->nb_wires; j++) n_inf[m] += mask[m][j] != 0;
        put_be(p, d->nb_wires, 8); put_be(p, n_inf[0], 8); put_be(p, n_inf[1], 8);
        for (int m = 0; m < 2; m++) {
            put_be(p, d->nb_wires, 4);
            const size_t bytes = (size_t)((d->nb_wires + 7) / 8);
            std::memset(p, 0, bytes);
            for (uint64_t j = 0; j < d->nb_wires; j++) if (mask[m][j]) p[j / 8] |= (uint8_t)(1u << (7 - j % 8));
            p += bytes;
        }
        put_be(p, n_ped, 4);
        for (uint32_t k = 0; k < 2 * n_ped; k++) MI_TRY(section());
        MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if ((size_t)(p - out_host) != need) MI_FAIL(ctx, MI_EHIP, "keyfile: write: the stream written does not have the size computed for it");
        const double t_end = now_ms();
        ctx->keyfile_stats = mi_keyfile_stats{(float)(t_end - t_enc), (float)(t_enc - t0), 0.f, 0.f, (float)(t_end - t0)};
        return MI_OK;
    };
    const int32_t rc = body();
    (void)hipStreamSynchronize(ctx->stream);
    if (stage) (void)hipFree(stage);
    return rc;
}

}  // extern "C"

// groth16.Verify from the bytes of a proof (include/mi355x_groth16_verify_bytes.h): decode and hash on the device, then one of the four
// bodies of the verifier (verify_internal.h) over the decoded records, and the three debug entry points over the same arithmetic.
//
// One batch, every launch on ctx->stream:
//   host      the framing (proof_len, null pointers: MI_EINVAL), the count inside each proof against the key's (-> malformed)
//   k_decode_g1    one lane per (proof, G1 point): Ar, Krs, the commitments, pok -> a G1Aff and a malformed byte   (decode_ops.cuh)
//   k_decode_g2    one lane per proof: Bs -> a G2Aff and a malformed byte (an Fp2 square root: four fixed exponentiations)
//   k_verify_hash  one lane per proof: commitment_values and fold_challenge from the decoded commitments, the public inputs and the
//                  key's committed lists (sha256_h2f.cuh); a proof that did not decode is skipped
//   host      the decoded records come back as mi_verify_input (verify_bytes_decode, the one front of the entry points below) and go
//             through the body of their entry point: mi_verify_run (verify.hip), mi_verify_run_wave (verify_wave.hip),
//             mi_verify_combined_run (verify_combined.hip) or mi_verify_locate_run (verify_locate.hip); a proof that did not decode
//             enters any of them as malformed and none of its words is read.
// Two decode kernels rather than one: a G2 lane does four times the work of a G1 lane, and in one wave the G1 lanes would wait for it.
// Everything of a batch lives in ONE grow-only workspace (WS_VERIFY_BYTES): nothing is allocated in steady state.
#include "verify_internal.h"
#include "../../include/mi355x_groth16_verify_bytes.h"
#include "../../include/mi355x_groth16_vkfile.h"
#include "sha256_h2f.cuh"
#include "witness_ops.cuh"
#include <cstring>
#include <string>
#include <vector>

namespace {

// enc: n_lanes encodings of 32 bytes.  per_proof == 0: back to back.  Otherwise lane = proof * per_proof + slot and the encoding is
// slot `slot` of that proof's bytes (proof_g1_slot_offset), proofs proof_len apart.
__global__ void __launch_bounds__(64, 1) k_decode_g1(const uint8_t *enc, size_t proof_len, u32 per_proof, G1Aff *out, uint8_t *bad, size_t n_lanes) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_lanes) return;
    const uint8_t *src = per_proof ? enc + (i / per_proof) * proof_len + proof_g1_slot_offset((u32)(i % per_proof)) : enc + 32 * i;
    uint8_t b[32];
    for (int k = 0; k < 32; k++) b[k] = src[k];
    G1Aff p;
    const bool ok = g1_decode(&p, b);
    out[i] = p;
    bad[i] = ok ? 0 : 1;
}
// enc: n encodings of 64 bytes, stride apart
__global__ void __launch_bounds__(64, 1) k_decode_g2(const uint8_t *enc, size_t stride, G2Aff *out, uint8_t *bad, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t *src = enc + i * stride;
    uint8_t b[64];
    for (int k = 0; k < 64; k++) b[k] = src[k];
    G2Aff q;
    const bool ok = g2_decode(&q, b);
    out[i] = q;
    bad[i] = ok ? 0 : 1;
}
// g1: per proof its 3 + nc decoded points in slot order (commitments from slot 2); bad1 / bad2 / bad_count -> bad[i] for the host
__global__ void __launch_bounds__(64, 1) k_verify_hash(const G1Aff *g1, const uint8_t *bad1, const uint8_t *bad2, u32 nc, const Fr *public_inputs, u32 n_pub,
                                                       const u32 *pc_off, const u32 *pc_idx, Fr *values, Fr *folds, uint8_t *bad, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32 slots = proof_g1_slots(nc);
    u32 b = bad[i] | bad2[i];   // bad[i] arrives holding the host's count check
    for (u32 s = 0; s < slots; s++) b |= bad1[i * slots + s];
    bad[i] = b ? 1 : 0;
    Fr fold = Fr::zero();
    for (u32 k = 0; k < nc; k++) values[i * nc + k] = Fr::zero();
    if (!b && nc) bsb22_hashes(g1 + i * slots + 2, nc, public_inputs + i * n_pub, n_pub, pc_off, pc_idx, values + i * nc, &fold);
    folds[i] = fold;
}
// The public inputs of a batch from their bytes (mi_groth16_verify_files*): lane i * n_pub + j reads value j of witness i -- 32 bytes at
// wit + i * stride + 32 j, any alignment -- and writes row i, column j of the n x n_pub matrix k_verify_hash and the verifier's bodies
// read.  A value that is not below r leaves zero and sets bad[i]; the kernel only ever sets a byte.
__global__ void __launch_bounds__(64) k_witness_decode(const uint8_t *wit, size_t stride, u32 n_pub, Fr *out, uint8_t *bad, size_t n_lanes) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_lanes) return;
    const size_t i = t / n_pub, j = t % n_pub;
    const uint8_t *src = wit + i * stride + 32 * j;
    // the 32 bytes into registers: two 16-byte loads where the address allows it (the staging image of a batch always does: consecutive
    // lanes then read consecutive 32-byte strings), byte loads otherwise
    union { uint4 q[2]; uint8_t b[32]; } buf;
    if (((uintptr_t)src & 15) == 0) {
        buf.q[0] = ((const uint4 *)src)[0];
        buf.q[1] = ((const uint4 *)src)[1];
    } else {
        for (int k = 0; k < 32; k++) buf.b[k] = src[k];
    }
    Fr v;
    if (!fr_from_be32(&v, buf.b)) bad[i] = 1;
    out[t] = v;
}
__global__ void __launch_bounds__(64, 1) k_hash_to_field(const uint8_t *msgs, size_t msg_len, const uint8_t *dst, u32 dst_len, Fr *out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint8_t d[255];
    for (u32 k = 0; k < dst_len; k++) d[k] = dst[k];
    out[i] = hash_to_field(d, dst_len, msgs + i * msg_len, msg_len);
}

// A batch decoded: dec, the records as mi_verify_input for any body of the verifier, over the vectors that hold their words, and
// bad[i] != 0 where proof i did not decode (the bodies' decode_malformed)
struct Decoded {
    std::vector<G1Aff> g1;
    std::vector<G2Aff> g2;
    std::vector<Fr> values, folds;
    std::vector<uint8_t> bad;
    std::vector<mi_verify_input> dec;
    const Fr *pub_dev = nullptr;   // the files front: the public inputs stay on the device (WS_VERIFY_BYTES), n x n_pub
};
// has_verdict: the caller's verdict pointer passes its own rule.  n = 0 leaves *d empty.
// Two fronts, one of `in` and `fin`: Montgomery public inputs from the caller's memory, or (mi_groth16_verify_files*) witness bytes,
// which travel in the same staging image and are decoded in front of k_verify_hash into the region the other front uploads to.
int32_t verify_bytes_decode(mi_ctx *ctx, const mi_vk *vk, const mi_verify_bytes_input *in, const mi_verify_files_input *fin, size_t n, bool has_verdict,
                            Decoded *d) {
    if (!ctx) return MI_EINVAL;
    const std::string w = fin ? "verify files: " : "verify bytes: ";
    if (!vk || (!in && !fin && n) || !has_verdict) MI_FAIL(ctx, MI_EINVAL, w + "null vk, input or verdict pointer");
    if (n > ((size_t)1 << 24)) MI_FAIL(ctx, MI_EINVAL, w + "more than 2^24 proofs in one batch");
    const u32 nc = vk->n_commitments, n_pub = vk->nb_public - 1, slots = proof_g1_slots(nc);
    const size_t plen = proof_bytes_len(nc);
    auto proof_of = [&](size_t i) { return fin ? fin[i].proof : in[i].proof; };
    for (size_t i = 0; i < n; i++) {
        const size_t len = fin ? fin[i].proof_len : in[i].proof_len;
        if (!proof_of(i)) MI_FAIL(ctx, MI_EINVAL, w + "proof is null");
        if (len != plen) MI_FAIL(ctx, MI_EINVAL, w + "proof_len is " + std::to_string(len) + ", the key's proofs have " + std::to_string(plen) + " bytes");
        if (!fin && n_pub && !in[i].public_inputs) MI_FAIL(ctx, MI_EINVAL, w + "public_inputs is null");
        if (fin) {
            if (!fin[i].witness) MI_FAIL(ctx, MI_EINVAL, w + "witness is null");
            if (fin[i].witness_len < MI_WITNESS_HEADER_BYTES || (fin[i].witness_len - MI_WITNESS_HEADER_BYTES) % 32 ||
                (fin[i].witness_len - MI_WITNESS_HEADER_BYTES) / 32 != witness_be32(fin[i].witness + 8))
                MI_FAIL(ctx, MI_EINVAL, w + "witness_len is " + std::to_string(fin[i].witness_len) + ", not 12 + 32 n of the witness's own header");
        }
    }
    if (!n) return MI_OK;
    // ---- workspace; the first four regions travel as one image (the files front: the witnesses' public bytes in it, off_pub after it)
    const size_t n_idx = vk->pc_idx.size(), wstride = (size_t)n_pub * 32;
    WsCut cut;
    const size_t off_bytes = cut.take(n * plen), off_front = cut.take(fin ? n * wstride : n * n_pub * sizeof(Fr)), off_po = cut.take((nc + 1) * sizeof(u32));
    const size_t off_pi = cut.take(n_idx * sizeof(u32)), image = cut.total;
    const size_t off_pub = fin ? cut.take(n * n_pub * sizeof(Fr)) : off_front, off_wit = off_front;
    const size_t off_g1 = cut.take(n * slots * sizeof(G1Aff)), off_g2 = cut.take(n * sizeof(G2Aff)), off_b1 = cut.take(n * slots);
    const size_t off_b2 = cut.take(n), off_bad = cut.take(n), off_val = cut.take(n * nc * sizeof(Fr)), off_fold = cut.take(n * sizeof(Fr));
    MI_TRY(mi_reserve(ctx, ctx->ws[WS_VERIFY_BYTES], cut.total));
    char *ws = (char *)ctx->ws[WS_VERIFY_BYTES].p;
    // ---- host: one staging image of the first four regions and the count check
    *d = Decoded{std::vector<G1Aff>(n * slots), std::vector<G2Aff>(n), std::vector<Fr>((size_t)n * nc), std::vector<Fr>(n),
                 std::vector<uint8_t>(n, 0), std::vector<mi_verify_input>(n)};
    std::vector<uint8_t> stage(image, 0);
    for (size_t i = 0; i < n; i++) {
        std::memcpy(&stage[off_bytes + i * plen], proof_of(i), plen);
        d->bad[i] = proof_bytes_count(proof_of(i)) != nc;
        if (!fin) {
            if (n_pub) std::memcpy(&stage[off_pub + i * n_pub * sizeof(Fr)], in[i].public_inputs, (size_t)n_pub * sizeof(Fr));
            continue;
        }
        // the header against the key and against itself; the public part is the first nbPublic values, the rest is not read
        const uint8_t *wt = fin[i].witness;
        const uint64_t w_pub = witness_be32(wt), w_sec = witness_be32(wt + 4), w_n = witness_be32(wt + 8);
        if (w_pub != n_pub || w_pub + w_sec != w_n) d->bad[i] = 1;   // its values stay zero bytes in the image
        else if (n_pub) std::memcpy(&stage[off_wit + i * wstride], wt + MI_WITNESS_HEADER_BYTES, wstride);
    }
    std::memcpy(&stage[off_po], vk->pc_off.data(), (nc + 1) * sizeof(u32));
    if (n_idx) std::memcpy(&stage[off_pi], vk->pc_idx.data(), n_idx * sizeof(u32));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(ws + off_bytes, stage.data(), image, hipMemcpyHostToDevice, ctx->stream));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(ws + off_bad, d->bad.data(), n, hipMemcpyHostToDevice, ctx->stream));
    // ---- device: decode, hash
    const uint8_t *bytes = (const uint8_t *)(ws + off_bytes);
    if (fin) {
        MI_TRY(mi_launch64(ctx, k_witness_decode, n * n_pub, (const uint8_t *)(ws + off_wit), wstride, n_pub, (Fr *)(ws + off_pub), (uint8_t *)(ws + off_bad), n * n_pub));
        d->pub_dev = (const Fr *)(ws + off_pub);
    }
    MI_TRY(mi_launch64(ctx, k_decode_g1, n * slots, bytes, plen, slots, (G1Aff *)(ws + off_g1), (uint8_t *)(ws + off_b1), n * slots));
    MI_TRY(mi_launch64(ctx, k_decode_g2, n, bytes + MI_PROOF_OFF_BS, plen, (G2Aff *)(ws + off_g2), (uint8_t *)(ws + off_b2), n));
    MI_TRY(mi_launch64(ctx, k_verify_hash, n, (const G1Aff *)(ws + off_g1), (const uint8_t *)(ws + off_b1), (const uint8_t *)(ws + off_b2), nc,
                       (const Fr *)(ws + off_pub), n_pub, (const u32 *)(ws + off_po), (const u32 *)(ws + off_pi), (Fr *)(ws + off_val),
                       (Fr *)(ws + off_fold), (uint8_t *)(ws + off_bad), n));
    // ---- host: the decoded records as mi_verify_input
    MI_CHECK_HIP(ctx, hipMemcpyAsync(d->g1.data(), ws + off_g1, d->g1.size() * sizeof(G1Aff), hipMemcpyDeviceToHost, ctx->stream));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(d->g2.data(), ws + off_g2, d->g2.size() * sizeof(G2Aff), hipMemcpyDeviceToHost, ctx->stream));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(d->bad.data(), ws + off_bad, n, hipMemcpyDeviceToHost, ctx->stream));
    if (nc) MI_CHECK_HIP(ctx, hipMemcpyAsync(d->values.data(), ws + off_val, d->values.size() * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(d->folds.data(), ws + off_fold, n * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    mi_verify_input *dec = d->dec.data();
    for (size_t i = 0; i < n; i++) {
        const G1Aff *p = &d->g1[i * slots];
        std::memcpy(&dec[i].proof.ar, &p[0], sizeof(G1Aff));
        std::memcpy(&dec[i].proof.bs, &d->g2[i], sizeof(G2Aff));
        std::memcpy(&dec[i].proof.krs, &p[1], sizeof(G1Aff));
        dec[i].commitments = (const mi_g1_affine *)(p + 2);
        dec[i].pok = (const mi_g1_affine *)(p + 2 + nc);
        dec[i].public_inputs = fin ? nullptr : in[i].public_inputs;
        dec[i].commitment_values = nc ? (const mi_fr *)&d->values[i * nc] : nullptr;
        dec[i].fold_challenge = (const mi_fr *)&d->folds[i];
    }
    return MI_OK;
}

}   // namespace

extern "C" {

int32_t mi_vk_set_public_committed(mi_ctx *ctx, mi_vk *vk, const uint32_t *offsets, const uint32_t *indices) {
    if (!ctx) return MI_EINVAL;
    if (!vk || !offsets) MI_FAIL(ctx, MI_EINVAL, "public committed: null vk or offsets");
    const u32 nc = vk->n_commitments;
    if (offsets[0] != 0) MI_FAIL(ctx, MI_EINVAL, "public committed: offsets[0] is not 0");
    for (u32 i = 0; i < nc; i++)
        if (offsets[i + 1] < offsets[i]) MI_FAIL(ctx, MI_EINVAL, "public committed: offsets[" + std::to_string(i + 1) + "] is below offsets[" + std::to_string(i) + "]");
    if (offsets[nc] && !indices) MI_FAIL(ctx, MI_EINVAL, "public committed: indices is null");
    for (u32 i = 0; i < nc; i++)
        for (u32 t = offsets[i]; t < offsets[i + 1]; t++)
            if (indices[t] < 1 || indices[t] > vk->nb_public - 1 + i)
                MI_FAIL(ctx, MI_EINVAL, "public committed: indices[" + std::to_string(t) + "] = " + std::to_string(indices[t]) + " of commitment " + std::to_string(i) +
                                            " is outside 1 .. " + std::to_string(vk->nb_public - 1 + i));
    vk->pc_off.assign(offsets, offsets + nc + 1);
    vk->pc_idx.assign(indices, indices + offsets[nc]);
    return MI_OK;
}

int32_t mi_groth16_verify_bytes(mi_ctx *ctx, const mi_vk *vk, const uint8_t *proof, size_t proof_len, const mi_fr *public_inputs, uint8_t *verdict) {
    if (ctx && !verdict) MI_FAIL(ctx, MI_EINVAL, "verify bytes: null verdict pointer");
    const mi_verify_bytes_input in{proof, proof_len, public_inputs};
    return mi_groth16_verify_bytes_batch(ctx, vk, &in, 1, verdict);
}
int32_t mi_groth16_verify_bytes_batch(mi_ctx *ctx, const mi_vk *vk, const mi_verify_bytes_input *in, size_t n, uint8_t *verdicts) {
    Decoded d;
    MI_TRY(verify_bytes_decode(ctx, vk, in, nullptr, n, verdicts || !n, &d));
    return mi_verify_run(ctx, vk, d.dec.data(), n, verdicts, d.bad.data());
}

int32_t mi_groth16_verify_bytes_wave(mi_ctx *ctx, const mi_vk *vk, const mi_verify_bytes_input *in, size_t n, uint8_t *verdicts) {
    Decoded d;
    MI_TRY(verify_bytes_decode(ctx, vk, in, nullptr, n, verdicts || !n, &d));
    return mi_verify_run_wave(ctx, vk, d.dec.data(), n, verdicts, d.bad.data());
}

int32_t mi_groth16_verify_bytes_combined(mi_ctx *ctx, const mi_vk *vk, const mi_verify_bytes_input *in, size_t n, const uint8_t *seed, uint8_t *verdict,
                                         uint64_t *first_malformed) {
    Decoded d;
    MI_TRY(verify_bytes_decode(ctx, vk, in, nullptr, n, verdict != nullptr, &d));
    return mi_verify_combined_run(ctx, vk, d.dec.data(), n, seed, verdict, first_malformed, d.bad.data());
}

int32_t mi_groth16_verify_bytes_locate(mi_ctx *ctx, const mi_vk *vk, const mi_verify_bytes_input *in, size_t n, const uint8_t *seed, uint8_t *verdicts,
                                       mi_verify_locate_stats *stats) {
    Decoded d;
    MI_TRY(verify_bytes_decode(ctx, vk, in, nullptr, n, verdicts || !n, &d));
    return mi_verify_locate_run(ctx, vk, d.dec.data(), n, seed, verdicts, stats, d.bad.data());
}

// ---------------------------------------------------------------- from files (include/mi355x_groth16_vkfile.h): the same three bodies over
// the same decoded records, the public inputs as a device-resident block
int32_t mi_groth16_verify_files(mi_ctx *ctx, const mi_vk *vk, const uint8_t *proof, size_t proof_len, const uint8_t *witness, size_t witness_len,
                                uint8_t *verdict) {
    if (ctx && !verdict) MI_FAIL(ctx, MI_EINVAL, "verify files: null verdict pointer");
    const mi_verify_files_input in{proof, proof_len, witness, witness_len};
    return mi_groth16_verify_files_batch(ctx, vk, &in, 1, verdict);
}
int32_t mi_groth16_verify_files_batch(mi_ctx *ctx, const mi_vk *vk, const mi_verify_files_input *in, size_t n, uint8_t *verdicts) {
    Decoded d;
    if (ctx && !in && n) MI_FAIL(ctx, MI_EINVAL, "verify files: null input pointer");
    MI_TRY(verify_bytes_decode(ctx, vk, nullptr, in, n, verdicts || !n, &d));
    return mi_verify_run(ctx, vk, d.dec.data(), n, verdicts, d.bad.data(), d.pub_dev);
}
int32_t mi_groth16_verify_files_combined(mi_ctx *ctx, const mi_vk *vk, const mi_verify_files_input *in, size_t n, const uint8_t *seed, uint8_t *verdict,
                                         uint64_t *first_malformed) {
    Decoded d;
    if (ctx && !in && n) MI_FAIL(ctx, MI_EINVAL, "verify files: null input pointer");
    MI_TRY(verify_bytes_decode(ctx, vk, nullptr, in, n, verdict != nullptr, &d));
    return mi_verify_combined_run(ctx, vk, d.dec.data(), n, seed, verdict, first_malformed, d.bad.data(), d.pub_dev);
}
int32_t mi_groth16_verify_files_locate(mi_ctx *ctx, const mi_vk *vk, const mi_verify_files_input *in, size_t n, const uint8_t *seed, uint8_t *verdicts,
                                       mi_verify_locate_stats *stats) {
    Decoded d;
    if (ctx && !in && n) MI_FAIL(ctx, MI_EINVAL, "verify files: null input pointer");
    MI_TRY(verify_bytes_decode(ctx, vk, nullptr, in, n, verdicts || !n, &d));
    return mi_verify_locate_run(ctx, vk, d.dec.data(), n, seed, verdicts, stats, d.bad.data(), d.pub_dev);
}

// ---------------------------------------------------------------- debug surface (include/mi355x_groth16_debug.h)
int32_t mi_debug_decode_g1_dev(mi_ctx *ctx, const uint8_t *enc_dev, size_t n, mi_g1_affine *out_dev, uint8_t *bad_dev) {
    if (!ctx || ((!enc_dev || !out_dev || !bad_dev) && n) || n > ((size_t)1 << 24)) return MI_EINVAL;
    return mi_launch64(ctx, k_decode_g1, n, enc_dev, (size_t)0, 0u, (G1Aff *)out_dev, bad_dev, n);
}
int32_t mi_debug_decode_g2_dev(mi_ctx *ctx, const uint8_t *enc_dev, size_t n, mi_g2_affine *out_dev, uint8_t *bad_dev) {
    if (!ctx || ((!enc_dev || !out_dev || !bad_dev) && n) || n > ((size_t)1 << 24)) return MI_EINVAL;
    return mi_launch64(ctx, k_decode_g2, n, enc_dev, (size_t)64, (G2Aff *)out_dev, bad_dev, n);
}
int32_t mi_debug_witness_decode_dev(mi_ctx *ctx, const uint8_t *values_dev, size_t n, uint32_t n_pub, mi_fr *out_dev, uint8_t *bad_dev) {
    if (!ctx || n > ((size_t)1 << 24) || (uint64_t)n * n_pub > ((uint64_t)1 << 32) || ((!values_dev || !out_dev) && n && n_pub) || (!bad_dev && n)) return MI_EINVAL;
    return mi_launch64(ctx, k_witness_decode, n * n_pub, values_dev, (size_t)n_pub * 32, n_pub, (Fr *)out_dev, bad_dev, n * n_pub);
}
int32_t mi_debug_hash_to_field_dev(mi_ctx *ctx, const uint8_t *dst_dev, uint32_t dst_len, const uint8_t *msgs_dev, size_t msg_len, size_t n, mi_fr *out_dev) {
    if (!ctx || !dst_dev || dst_len == 0 || dst_len > 255 || ((!out_dev || (!msgs_dev && msg_len)) && n) || n > ((size_t)1 << 24)) return MI_EINVAL;
    return mi_launch64(ctx, k_hash_to_field, n, msgs_dev, msg_len, dst_dev, dst_len, (Fr *)out_dev, n);
}
}

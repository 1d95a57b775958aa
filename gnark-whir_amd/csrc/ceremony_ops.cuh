// What the checks of a ceremony (include/mi355x_groth16_phase2_check.h) hash and judge, one record per lane / per call, MI_HD: the kernels
// of phase2_check.hip, the host code of phase2_records.hip and the host build of the tests (tests/cpp/phase2_check_host.cpp, phase2_sigma_host.cpp) run this text.
//
// Coefficients of the same-ratio tests:
//     r_k = the little-endian integer of the first 16 bytes of SHA-256("mi355x-ceremony-coeff" | seed (32 bytes) | le64(k))
// The chain of a contribution's records (THIS PROJECT'S format, not gnark's):
//     hash_i = SHA-256("mi355x-phase2-record" | hash_(i-1) | le64(i) | compress(delta1_before) | compress(delta1) | compress(T))
//     c_i    = the little-endian integer of the first 16 bytes of SHA-256("mi355x-phase2-challenge" | hash_i)
//     record i holds iff   hash = hash_i   and   [z] delta1_before = T + [c_i] delta1
// compress = mi_g1_compress (keyfile_ops.cuh's g1_encode_stream gives the same 32 bytes).
#pragma once
#include "sha256_h2f.cuh"
#include "pairing_ops.cuh"
#include "keyfile_ops.cuh"
#include "point_ntt.cuh"
#include <vector>

#define MI_CEREMONY_COEFF_TAG_LEN 21
#define MI_CEREMONY_RECORD_TAG_LEN 20
#define MI_CEREMONY_CHALLENGE_TAG_LEN 23
MI_HD uint8_t ceremony_coeff_tag(int i) { constexpr char d[MI_CEREMONY_COEFF_TAG_LEN + 1] = "mi355x-ceremony-coeff"; return (uint8_t)d[i]; }
MI_HD uint8_t ceremony_record_tag(int i) { constexpr char d[MI_CEREMONY_RECORD_TAG_LEN + 1] = "mi355x-phase2-record"; return (uint8_t)d[i]; }
MI_HD uint8_t ceremony_challenge_tag(int i) { constexpr char d[MI_CEREMONY_CHALLENGE_TAG_LEN + 1] = "mi355x-phase2-challenge"; return (uint8_t)d[i]; }

// the first 16 bytes of a digest as four little-endian words
MI_HD void ceremony_low128(const uint8_t d[32], u32 out[4]) {
    for (int w = 0; w < 4; w++) out[w] = (u32)d[4 * w] | ((u32)d[4 * w + 1] << 8) | ((u32)d[4 * w + 2] << 16) | ((u32)d[4 * w + 3] << 24);
}
// One compression of SHA-256 with the state and the message schedule in registers: once the loops are unrolled every index is a
// constant.  (sha256_block of sha256_h2f.cuh is out of line and takes its state by address, which on the device is scratch memory; the
// coefficient kernel runs up to 2^27 lanes of two compressions each and keeps everything in registers instead.)
MI_HD void ceremony_sha256_compress(u32 h[8], u32 w[16]) {
    u32 a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll
    for (int t = 0; t < 64; t++) {
        if (t >= 16) {
            const u32 w15 = w[(t + 1) & 15], w2 = w[(t + 14) & 15];
            const u32 s0 = sha256_rotr(w15, 7) ^ sha256_rotr(w15, 18) ^ (w15 >> 3), s1 = sha256_rotr(w2, 17) ^ sha256_rotr(w2, 19) ^ (w2 >> 10);
            w[t & 15] += s0 + w[(t + 9) & 15] + s1;
        }
        const u32 t1 = hh + (sha256_rotr(e, 6) ^ sha256_rotr(e, 11) ^ sha256_rotr(e, 25)) + ((e & f) ^ (~e & g)) + sha256_k(t) + w[t & 15];
        const u32 t2 = (sha256_rotr(a, 2) ^ sha256_rotr(a, 13) ^ sha256_rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}
// byte j of the padded first block of a coefficient's message: tag (21) | seed (32) | le64(k) (8) | 0x80 | 0 0
MI_HD u32 ceremony_coeff_block_byte(const uint8_t seed[32], u64 k, int j) {
    if (j < MI_CEREMONY_COEFF_TAG_LEN) return ceremony_coeff_tag(j);
    if (j < MI_CEREMONY_COEFF_TAG_LEN + 32) return seed[j - MI_CEREMONY_COEFF_TAG_LEN];
    if (j < MI_CEREMONY_COEFF_TAG_LEN + 40) return (u32)(k >> (8 * (j - MI_CEREMONY_COEFF_TAG_LEN - 32))) & 0xffu;
    return j == MI_CEREMONY_COEFF_TAG_LEN + 40 ? 0x80u : 0u;
}
// out: four little-endian words of r_k.  The message is 61 bytes: one block that ends with the padding's first byte, then a block that
// holds the length alone.
MI_HD void ceremony_coefficient(const uint8_t seed[32], u64 k, u32 out[4]) {
    u32 h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    u32 w[16];
#pragma unroll
    for (int i = 0; i < 16; i++)
        w[i] = (ceremony_coeff_block_byte(seed, k, 4 * i) << 24) | (ceremony_coeff_block_byte(seed, k, 4 * i + 1) << 16) |
               (ceremony_coeff_block_byte(seed, k, 4 * i + 2) << 8) | ceremony_coeff_block_byte(seed, k, 4 * i + 3);
    ceremony_sha256_compress(h, w);
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = 0;
    w[15] = 8 * (MI_CEREMONY_COEFF_TAG_LEN + 40);
    ceremony_sha256_compress(h, w);
    // digest byte 4 i + j is byte 3 - j of h[i]: the first 16 bytes as little-endian words are h[0 .. 3] with their bytes swapped
#pragma unroll
    for (int i = 0; i < 4; i++) out[i] = (h[i] >> 24) | ((h[i] >> 8) & 0xff00u) | ((h[i] << 8) & 0xff0000u) | (h[i] << 24);
}

// One same-ratio test e(P_a, Q_a) = e(P_b, Q_b) is judged from the product of the Miller values of (P_a, Q_a) and (-P_b, Q_b) after its
// final exponentiation
MI_HD bool ceremony_relation_holds(const Fp12 *after_final_exp) { return *after_final_exp == Fp12::one(); }

// ---------------------------------------------------------------- the records of the contributions (host callers)
// the layout of mi_phase2_record
struct CeremonyRecord {
    G1Aff delta1, commit;
    Fr response;
    uint8_t hash[32];
};
MI_HD void ceremony_record_hash(const uint8_t prev[32], u64 index, const G1Aff &before, const G1Aff &after, const G1Aff &commit, uint8_t out[32]) {
    Sha256 s;
    uint8_t b[32];
    sha256_init(&s);
    for (int i = 0; i < MI_CEREMONY_RECORD_TAG_LEN; i++) sha256_byte(&s, ceremony_record_tag(i));
    sha256_update(&s, prev, 32);
    for (int i = 0; i < 8; i++) sha256_byte(&s, (uint8_t)(index >> (8 * i)));
    g1_encode_stream(b, before, true); sha256_update(&s, b, 32);
    g1_encode_stream(b, after, true); sha256_update(&s, b, 32);
    g1_encode_stream(b, commit, true); sha256_update(&s, b, 32);
    sha256_final(&s, out);
}
MI_HD void ceremony_challenge(const uint8_t hash[32], u32 c[4]) {
    Sha256 s;
    uint8_t d[32];
    sha256_init(&s);
    for (int i = 0; i < MI_CEREMONY_CHALLENGE_TAG_LEN; i++) sha256_byte(&s, ceremony_challenge_tag(i));
    sha256_update(&s, hash, 32);
    sha256_final(&s, d);
    ceremony_low128(d, c);
}
// The record of the contribution delta1 = [d] before with the nonce k (d, k Montgomery, neither 0): T = [k] before, z = k + c d.
// delta1 is given: the caller has computed it (the state's point after mi_phase2_contribute).
inline void ceremony_record_make(const uint8_t prev[32], u64 index, const G1Aff &before, const G1Aff &delta1, const Fr &d, const Fr &k, CeremonyRecord *out) {
    out->delta1 = delta1;
    out->commit = xyzz_to_affine(xyzz_scale(G1X::from_affine(before), k));
    ceremony_record_hash(prev, index, before, delta1, out->commit, out->hash);
    u32 c[4];
    ceremony_challenge(out->hash, c);
    out->response = k + fr_from_u128(c) * d;
}
// Record `index` of a chain after `prev`, over delta1_before = before.  Words that are no point of the curve, a point at infinity or a
// response that is not below r hold nothing: decided before any arithmetic touches them.
inline bool ceremony_record_holds(const uint8_t prev[32], u64 index, const G1Aff &before, const CeremonyRecord &rec) {
    if (!g1_on_curve(rec.delta1) || !g1_on_curve(rec.commit) || rec.delta1.is_inf() || rec.commit.is_inf() || !fe_is_reduced(rec.response)) return false;
    uint8_t h[32];
    ceremony_record_hash(prev, index, before, rec.delta1, rec.commit, h);
    for (int i = 0; i < 32; i++) if (h[i] != rec.hash[i]) return false;
    u32 c[4];
    ceremony_challenge(h, c);
    const G1Aff lhs = xyzz_to_affine(xyzz_scale(G1X::from_affine(before), rec.response));
    G1X rhs = G1X::from_affine(g1_scale128(rec.delta1, c));
    xyzz_madd(rhs, rec.commit, false);
    const G1Aff r = xyzz_to_affine(rhs);
    return lhs.x == r.x && lhs.y == r.y;
}
// The chain of m records that continues (start, start_hash, first_index): the index of the first record that does not hold, m when all do
inline u64 ceremony_records_first_bad(const G1Aff &start, const uint8_t start_hash[32], u64 first_index, const CeremonyRecord *rec, size_t m) {
    G1Aff before = start;
    const uint8_t *prev = start_hash;
    for (size_t i = 0; i < m; i++) {
        if (!ceremony_record_holds(prev, first_index + i, before, rec[i])) return i;
        before = rec[i].delta1;
        prev = rec[i].hash;
    }
    return m;
}

// ---------------------------------------------------------------- the steps of the sigma chain (host callers)
// One step re-randomises the nc points [-sigma_k]2 of a state under ONE challenge, over the twist:
//     hash_i = SHA-256("mi355x-phase2-sigma-record" | hash_(i-1) | le64(i) | le32(nc) | for k: compress2(before_k) | compress2(after_k) | compress2(T_k))
//     c_i    = the little-endian integer of the first 16 bytes of SHA-256("mi355x-phase2-sigma-challenge" | hash_i)
//     step i holds iff   hash = hash_i   and for every k   [z_k] before_k = T_k + [c_i] after_k
// compress2 = mi_g2_compress (keyfile_ops.cuh's g2_encode_stream gives the same 64 bytes).
#define MI_CEREMONY_SIGMA_RECORD_TAG_LEN 26
#define MI_CEREMONY_SIGMA_CHALLENGE_TAG_LEN 29
MI_HD uint8_t ceremony_sigma_record_tag(int i) { constexpr char d[MI_CEREMONY_SIGMA_RECORD_TAG_LEN + 1] = "mi355x-phase2-sigma-record"; return (uint8_t)d[i]; }
MI_HD uint8_t ceremony_sigma_challenge_tag(int i) { constexpr char d[MI_CEREMONY_SIGMA_CHALLENGE_TAG_LEN + 1] = "mi355x-phase2-sigma-challenge"; return (uint8_t)d[i]; }
// the layout of mi_phase2_sigma_proof: one commitment's part of a step
struct CeremonySigmaProof {
    G2Aff g_sigma_neg, commit;
    Fr response;
};
// before: the nc points the step starts from; step: its nc parts
inline void ceremony_sigma_hash(const uint8_t prev[32], u64 index, u32 nc, const G2Aff *before, const CeremonySigmaProof *step, uint8_t out[32]) {
    Sha256 s;
    uint8_t b[64];
    sha256_init(&s);
    for (int i = 0; i < MI_CEREMONY_SIGMA_RECORD_TAG_LEN; i++) sha256_byte(&s, ceremony_sigma_record_tag(i));
    sha256_update(&s, prev, 32);
    for (int i = 0; i < 8; i++) sha256_byte(&s, (uint8_t)(index >> (8 * i)));
    for (int i = 0; i < 4; i++) sha256_byte(&s, (uint8_t)(nc >> (8 * i)));
    for (u32 k = 0; k < nc; k++) {
        g2_encode_stream(b, before[k], true); sha256_update(&s, b, 64);
        g2_encode_stream(b, step[k].g_sigma_neg, true); sha256_update(&s, b, 64);
        g2_encode_stream(b, step[k].commit, true); sha256_update(&s, b, 64);
    }
    sha256_final(&s, out);
}
inline void ceremony_sigma_challenge(const uint8_t hash[32], u32 c[4]) {
    Sha256 s;
    uint8_t d[32];
    sha256_init(&s);
    for (int i = 0; i < MI_CEREMONY_SIGMA_CHALLENGE_TAG_LEN; i++) sha256_byte(&s, ceremony_sigma_challenge_tag(i));
    sha256_update(&s, hash, 32);
    sha256_final(&s, d);
    ceremony_low128(d, c);
}
// The step after_k = [s_k] before_k with the nonces n_k (Montgomery, none 0): T_k = [n_k] before_k, z_k = n_k + c s_k.  after is given: the
// caller has computed it (the state's points after the contribution).
inline void ceremony_sigma_step_make(const uint8_t prev[32], u64 index, u32 nc, const G2Aff *before, const G2Aff *after, const Fr *s, const Fr *n,
                                     CeremonySigmaProof *out, uint8_t hash_out[32]) {
    for (u32 k = 0; k < nc; k++) {
        out[k].g_sigma_neg = after[k];
        out[k].commit = xyzz_to_affine(xyzz_scale(G2X::from_affine(before[k]), n[k]));
    }
    ceremony_sigma_hash(prev, index, nc, before, out, hash_out);
    u32 c[4];
    ceremony_sigma_challenge(hash_out, c);
    const Fr cc = fr_from_u128(c);
    for (u32 k = 0; k < nc; k++) out[k].response = n[k] + cc * s[k];
}
// words that are a point of the twist other than infinity: decided before any arithmetic touches them
inline bool ceremony_sigma_point_ok(const G2Aff &q) { return g2_reduced(q) && !q.is_inf() && g2_on_twist(q); }
// Step `index` of a chain after `prev`, over the nc points before
inline bool ceremony_sigma_step_holds(const uint8_t prev[32], u64 index, u32 nc, const G2Aff *before, const CeremonySigmaProof *step, const uint8_t hash[32]) {
    for (u32 k = 0; k < nc; k++)
        if (!ceremony_sigma_point_ok(step[k].g_sigma_neg) || !ceremony_sigma_point_ok(step[k].commit) || !fe_is_reduced(step[k].response)) return false;
    uint8_t h[32];
    ceremony_sigma_hash(prev, index, nc, before, step, h);
    for (int i = 0; i < 32; i++) if (h[i] != hash[i]) return false;
    u32 c[4];
    ceremony_sigma_challenge(h, c);
    const Fr cc = fr_from_u128(c);
    for (u32 k = 0; k < nc; k++) {
        const G2Aff lhs = xyzz_to_affine(xyzz_scale(G2X::from_affine(before[k]), step[k].response));
        G2X rhs = xyzz_scale(G2X::from_affine(step[k].g_sigma_neg), cc);
        xyzz_madd(rhs, step[k].commit, false);
        const G2Aff r = xyzz_to_affine(rhs);
        if (!(lhs.x == r.x && lhs.y == r.y)) return false;
    }
    return true;
}
// The chain of m steps (proofs: m * nc parts, hashes: m) that continues (start, start_hash, first_index): the index of the first step that
// does not hold, m when all do
inline u64 ceremony_sigma_first_bad(const G2Aff *start, u32 nc, const uint8_t start_hash[32], u64 first_index, const CeremonySigmaProof *proofs,
                                    const uint8_t (*hashes)[32], size_t m) {
    std::vector<G2Aff> before(start, start + nc);
    const uint8_t *prev = start_hash;
    for (size_t i = 0; i < m; i++) {
        const CeremonySigmaProof *step = proofs + i * nc;
        if (!ceremony_sigma_step_holds(prev, first_index + i, nc, before.data(), step, hashes[i])) return i;
        for (u32 k = 0; k < nc; k++) before[k] = step[k].g_sigma_neg;
        prev = hashes[i];
    }
    return m;
}

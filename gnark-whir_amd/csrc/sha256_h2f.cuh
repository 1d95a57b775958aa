// SHA-256 (FIPS 180-4), expand_message_xmd with it (RFC 9380 5.3.1) for len_in_bytes = 48, and the hash-to-field of ONE element of Fr:
// the 48 bytes read big-endian, reduced mod r, in Montgomery form -- what gnark-crypto's fr.Hash(msg, dst, 1) and hash_to_field.New(dst)
// give (go/mi355x/verify.go).  On top of it the two hashes of a BSB22 proof, exactly as that file states them:
//     value_i        = H_"bsb22-commitment"(uncompressed C_i | full[j - 1] as 32 bytes big-endian canonical, for j in committed_i)
//     full           = public_inputs | value_0 | ... | value_(i-1)
//     fold_challenge = H_"G16-BSB22"(value_0 | ... | value_(nc-1), 32 bytes big-endian canonical each)
// An uncompressed C_i is 64 bytes, X | Y big-endian canonical; INFINITY IS 64 ZERO BYTES (oracle/pyref.py g1_uncompressed's rule).
// MI_HD: the hash kernel (verify_bytes.hip, one lane per proof), mi_hash_to_field (proof_read.hip) and the host build of the tests
// (tests/emu/emu_decode.cpp) run this text.  SHA-256 and expand_message_xmd are pinned by their standards; the two DST strings and the
// infinity bytes are NOT pinned to gnark's source (include/mi355x_groth16_verify_bytes.h).
#pragma once
#include "decode_ops.cuh"

struct Sha256 {
    u32 h[8];
    u32 w[16];     // the open block, big-endian words
    u64 len;       // bytes absorbed
};
MI_HD u32 sha256_k(int i) {
    constexpr u32 k[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu,
        0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau,
        0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u,
        0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u,
        0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu,
        0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
    return k[i];
}
MI_HD u32 sha256_rotr(u32 x, int n) { return (x >> n) | (x << (32 - n)); }
MI_HD void sha256_init(Sha256 *s) {
    constexpr u32 iv[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    for (int i = 0; i < 8; i++) s->h[i] = iv[i];
    for (int i = 0; i < 16; i++) s->w[i] = 0;
    s->len = 0;
}
// one compression of s->w (which it uses up as the rolling message schedule)
MI_OOL void sha256_block(Sha256 *s) {
    u32 a = s->h[0], b = s->h[1], c = s->h[2], d = s->h[3], e = s->h[4], f = s->h[5], g = s->h[6], h = s->h[7];
    for (int t = 0; t < 64; t++) {
        if (t >= 16) {
            const u32 w15 = s->w[(t + 1) & 15], w2 = s->w[(t + 14) & 15];
            const u32 s0 = sha256_rotr(w15, 7) ^ sha256_rotr(w15, 18) ^ (w15 >> 3), s1 = sha256_rotr(w2, 17) ^ sha256_rotr(w2, 19) ^ (w2 >> 10);
            s->w[t & 15] += s0 + s->w[(t + 9) & 15] + s1;
        }
        const u32 t1 = h + (sha256_rotr(e, 6) ^ sha256_rotr(e, 11) ^ sha256_rotr(e, 25)) + ((e & f) ^ (~e & g)) + sha256_k(t) + s->w[t & 15];
        const u32 t2 = (sha256_rotr(a, 2) ^ sha256_rotr(a, 13) ^ sha256_rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    s->h[0] += a; s->h[1] += b; s->h[2] += c; s->h[3] += d; s->h[4] += e; s->h[5] += f; s->h[6] += g; s->h[7] += h;
    for (int i = 0; i < 16; i++) s->w[i] = 0;
}
MI_HD void sha256_byte(Sha256 *s, uint8_t v) {
    const u32 at = (u32)(s->len & 63);
    s->w[at >> 2] |= (u32)v << (24 - 8 * (at & 3));
    s->len++;
    if (at == 63) sha256_block(s);
}
MI_HD void sha256_update(Sha256 *s, const uint8_t *msg, size_t n) {
    for (size_t i = 0; i < n; i++) sha256_byte(s, msg[i]);
}
// pads, closes and writes the 32 digest bytes; s is spent afterwards
MI_HD void sha256_final(Sha256 *s, uint8_t out[32]) {
    const u64 bits = s->len * 8;
    sha256_byte(s, 0x80);
    while ((s->len & 63) != 56) sha256_byte(s, 0);
    for (int i = 7; i >= 0; i--) sha256_byte(s, (uint8_t)(bits >> (8 * i)));
    for (int i = 0; i < 8; i++) {
        out[4 * i] = (uint8_t)(s->h[i] >> 24); out[4 * i + 1] = (uint8_t)(s->h[i] >> 16); out[4 * i + 2] = (uint8_t)(s->h[i] >> 8); out[4 * i + 3] = (uint8_t)s->h[i];
    }
}

// ---------------------------------------------------------------- expand_message_xmd, len_in_bytes = 48 (ell = 2), dst_len <= 255
//     b_0 = H(Z_pad | msg | 0x00 0x30 | 0x00 | DST'),  b_1 = H(b_0 | 0x01 | DST'),  b_2 = H((b_0 ^ b_1) | 0x02 | DST'),  DST' = DST | len(DST)
// The message is absorbed in pieces: h2f_begin, any number of sha256_update, h2f_finish.
#define MI_H2F_BYTES 48
MI_HD void h2f_begin(Sha256 *s) {
    sha256_init(s);
    for (int i = 0; i < 64; i++) sha256_byte(s, 0);   // Z_pad: one block of zeros
}
MI_HD void h2f_dst_prime(Sha256 *s, const uint8_t *dst, u32 dst_len) {
    sha256_update(s, dst, dst_len);
    sha256_byte(s, (uint8_t)dst_len);
}
MI_HD void h2f_expand_finish(Sha256 *s, const uint8_t *dst, u32 dst_len, uint8_t out[MI_H2F_BYTES]) {
    uint8_t b0[32], b1[32], b2[32];
    sha256_byte(s, 0); sha256_byte(s, MI_H2F_BYTES); sha256_byte(s, 0);
    h2f_dst_prime(s, dst, dst_len);
    sha256_final(s, b0);
    sha256_init(s);
    sha256_update(s, b0, 32); sha256_byte(s, 1);
    h2f_dst_prime(s, dst, dst_len);
    sha256_final(s, b1);
    sha256_init(s);
    for (int i = 0; i < 32; i++) sha256_byte(s, (uint8_t)(b0[i] ^ b1[i]));
    sha256_byte(s, 2);
    h2f_dst_prime(s, dst, dst_len);
    sha256_final(s, b2);
    for (int i = 0; i < 32; i++) out[i] = b1[i];
    for (int i = 0; i < 16; i++) out[32 + i] = b2[i];
}
// 48 bytes big-endian = hi 2^256 + lo (hi < 2^128) -> its residue mod r, Montgomery form.  lo is brought below r by at most five
// conditional subtractions (2^256 < 6 r) before the multiplier sees it; hi is below r as it stands.
MI_HD Fr fr_from_be48(const uint8_t in[MI_H2F_BYTES]) {
    Fr hi = Fr::zero(), lo;
    for (int i = 0; i < 4; i++) {
        const uint8_t *w = in + 12 - 4 * i;
        hi.l[i] = ((u32)w[0] << 24) | ((u32)w[1] << 16) | ((u32)w[2] << 8) | (u32)w[3];
    }
    for (int i = 0; i < 8; i++) {
        const uint8_t *w = in + 16 + 28 - 4 * i;
        lo.l[i] = ((u32)w[0] << 24) | ((u32)w[1] << 16) | ((u32)w[2] << 8) | (u32)w[3];
    }
    for (int k = 0; k < 5; k++) {
        Fr d;
        const u32 borrow = fe_sub_raw(d, lo, Fr::modulus());
        for (int i = 0; i < 8; i++) lo.l[i] = borrow ? lo.l[i] : d.l[i];
    }
    const Fr r2 = Fr::r2();
    return (hi * r2) * r2 + lo * r2;   // hi R, then hi R^2 = (hi 2^256) R; lo R
}
MI_HD Fr h2f_finish(Sha256 *s, const uint8_t *dst, u32 dst_len) {
    uint8_t x[MI_H2F_BYTES];
    h2f_expand_finish(s, dst, dst_len, x);
    return fr_from_be48(x);
}
MI_HD Fr hash_to_field(const uint8_t *dst, u32 dst_len, const uint8_t *msg, size_t msg_len) {
    Sha256 s;
    h2f_begin(&s);
    sha256_update(&s, msg, msg_len);
    return h2f_finish(&s, dst, dst_len);
}

// ---------------------------------------------------------------- the hashes of one BSB22 proof
#define MI_DST_COMMITMENT_LEN 16
#define MI_DST_FOLD_LEN 9
MI_HD uint8_t dst_commitment(int i) { constexpr char d[MI_DST_COMMITMENT_LEN + 1] = "bsb22-commitment"; return (uint8_t)d[i]; }
MI_HD uint8_t dst_fold(int i) { constexpr char d[MI_DST_FOLD_LEN + 1] = "G16-BSB22"; return (uint8_t)d[i]; }
MI_HD void g1_absorb_uncompressed(Sha256 *s, const G1Aff &p) {
    uint8_t b[32];
    fe_to_be32(b, p.x); sha256_update(s, b, 32);   // infinity is (0, 0): 64 zero bytes come out by themselves
    fe_to_be32(b, p.y); sha256_update(s, b, 32);
}
// values[nc] and *fold from the decoded commitments, the public inputs (n_pub of them, without the ONE wire) and the key's
// PublicAndCommitmentCommitted lists in CSR form (pc_off[nc + 1], pc_idx; an index j names full[j - 1] and was range-checked when the
// lists were set: 1 <= j <= n_pub + i for commitment i).  fold is written with any commitment, as gnark computes it; the verifier
// reads it with more than one.
MI_HD void bsb22_hashes(const G1Aff *commitments, u32 nc, const Fr *public_inputs, u32 n_pub, const u32 *pc_off, const u32 *pc_idx, Fr *values, Fr *fold) {
    uint8_t dst[MI_DST_COMMITMENT_LEN], b[32];
    for (int i = 0; i < MI_DST_COMMITMENT_LEN; i++) dst[i] = dst_commitment(i);
    Sha256 s;
    for (u32 i = 0; i < nc; i++) {
        h2f_begin(&s);
        g1_absorb_uncompressed(&s, commitments[i]);
        for (u32 t = pc_off[i]; t < pc_off[i + 1]; t++) {
            const u32 j = pc_idx[t] - 1;
            fe_to_be32(b, j < n_pub ? public_inputs[j] : values[j - n_pub]);
            sha256_update(&s, b, 32);
        }
        values[i] = h2f_finish(&s, dst, MI_DST_COMMITMENT_LEN);
    }
    if (!nc) return;
    for (int i = 0; i < MI_DST_FOLD_LEN; i++) dst[i] = dst_fold(i);
    h2f_begin(&s);
    for (u32 i = 0; i < nc; i++) { fe_to_be32(b, values[i]); sha256_update(&s, b, 32); }
    *fold = h2f_finish(&s, dst, MI_DST_FOLD_LEN);
}

// The records of a phase-1 ceremony's contributions (include/mi355x_groth16_phase1.h), beside ceremony_ops.cuh and on its helpers: host
// callers (phase1.hip, phase1_records.hip, tests/cpp/phase1_host.cpp).  THIS PROJECT'S format, not gnark's.
//
// A contribution multiplies tau, alpha, beta by t, a, b.  Three points are watched: x = 0: tau_g1[1], 1: alpha_tau_g1[0], 2: beta_tau_g1[0],
// which the step multiplies by d_0 = t, d_1 = a, d_2 = b.  Three Schnorr proofs under ONE challenge:
//     T_x    = [k_x] before_x
//     hash_i = SHA-256("mi355x-phase1-record" | hash_(i-1) | le64(i) | compress(before_x) x3 | compress(after_x) x3 | compress(T_x) x3)
//     c_i    = the little-endian integer of the first 16 bytes of SHA-256("mi355x-phase1-challenge" | hash_i)     (ceremony_low128)
//     z_x    = k_x + c_i d_x
//     record i holds iff   hash = hash_i   and   [z_x] before_x = T_x + [c_i] after_x   for x = 0, 1, 2
#pragma once
#include "ceremony_ops.cuh"

#define MI_PHASE1_RECORD_TAG_LEN 20
#define MI_PHASE1_CHALLENGE_TAG_LEN 23
MI_HD uint8_t phase1_record_tag(int i) { constexpr char d[MI_PHASE1_RECORD_TAG_LEN + 1] = "mi355x-phase1-record"; return (uint8_t)d[i]; }
MI_HD uint8_t phase1_challenge_tag(int i) { constexpr char d[MI_PHASE1_CHALLENGE_TAG_LEN + 1] = "mi355x-phase1-challenge"; return (uint8_t)d[i]; }

// the layout of mi_phase1_record
struct Phase1Record {
    G1Aff after[3], commit[3];
    Fr response[3];
    uint8_t hash[32];
};
inline void phase1_record_hash(const uint8_t prev[32], u64 index, const G1Aff before[3], const G1Aff after[3], const G1Aff commit[3], uint8_t out[32]) {
    Sha256 s;
    uint8_t b[32];
    sha256_init(&s);
    for (int i = 0; i < MI_PHASE1_RECORD_TAG_LEN; i++) sha256_byte(&s, phase1_record_tag(i));
    sha256_update(&s, prev, 32);
    for (int i = 0; i < 8; i++) sha256_byte(&s, (uint8_t)(index >> (8 * i)));
    for (const G1Aff *row : {before, after, commit})
        for (int x = 0; x < 3; x++) { g1_encode_stream(b, row[x], true); sha256_update(&s, b, 32); }
    sha256_final(&s, out);
}
inline void phase1_challenge(const uint8_t hash[32], u32 c[4]) {
    Sha256 s;
    uint8_t d[32];
    sha256_init(&s);
    for (int i = 0; i < MI_PHASE1_CHALLENGE_TAG_LEN; i++) sha256_byte(&s, phase1_challenge_tag(i));
    sha256_update(&s, hash, 32);
    sha256_final(&s, d);
    ceremony_low128(d, c);
}
// The record of the step after[x] = [d[x]] before[x] with the nonces k[x] (Montgomery, none 0).  after is given: the state's points
// after the contribution.
inline void phase1_record_make(const uint8_t prev[32], u64 index, const G1Aff before[3], const G1Aff after[3], const Fr d[3], const Fr k[3], Phase1Record *out) {
    for (int x = 0; x < 3; x++) {
        out->after[x] = after[x];
        out->commit[x] = xyzz_to_affine(xyzz_scale(G1X::from_affine(before[x]), k[x]));
    }
    phase1_record_hash(prev, index, before, out->after, out->commit, out->hash);
    u32 c[4];
    phase1_challenge(out->hash, c);
    for (int x = 0; x < 3; x++) out->response[x] = k[x] + fr_from_u128(c) * d[x];
}
// Words that are no point of the curve, a point at infinity or a response that is not below r hold nothing: decided before any
// arithmetic touches them (as ceremony_record_holds).
inline bool phase1_record_holds(const uint8_t prev[32], u64 index, const G1Aff before[3], const Phase1Record &rec) {
    for (int x = 0; x < 3; x++)
        if (!g1_on_curve(rec.after[x]) || !g1_on_curve(rec.commit[x]) || rec.after[x].is_inf() || rec.commit[x].is_inf() || !fe_is_reduced(rec.response[x])) return false;
    uint8_t h[32];
    phase1_record_hash(prev, index, before, rec.after, rec.commit, h);
    for (int i = 0; i < 32; i++) if (h[i] != rec.hash[i]) return false;
    u32 c[4];
    phase1_challenge(h, c);
    for (int x = 0; x < 3; x++) {
        const G1Aff lhs = xyzz_to_affine(xyzz_scale(G1X::from_affine(before[x]), rec.response[x]));
        G1X rhs = G1X::from_affine(g1_scale128(rec.after[x], c));
        xyzz_madd(rhs, rec.commit[x], false);
        const G1Aff r = xyzz_to_affine(rhs);
        if (!(lhs.x == r.x && lhs.y == r.y)) return false;
    }
    return true;
}
// The chain of m records that continues (start[3], start_hash, first_index): the index of the first record that does not hold, m when all do
inline u64 phase1_records_first_bad(const G1Aff start[3], const uint8_t start_hash[32], u64 first_index, const Phase1Record *rec, size_t m) {
    G1Aff before[3] = {start[0], start[1], start[2]};
    const uint8_t *prev = start_hash;
    for (size_t i = 0; i < m; i++) {
        if (!phase1_record_holds(prev, first_index + i, before, rec[i])) return i;
        for (int x = 0; x < 3; x++) before[x] = rec[i].after[x];
        prev = rec[i].hash;
    }
    return m;
}

// The coefficients of the combined batch verifier (include/mi355x_groth16_verify_combined.h):
//     r_i = the little-endian integer of the first 16 bytes of SHA-256("mi355x-g16-combine" | seed | le64(n) | le64(i))
// Host work (one hash per proof); verify_combined.hip and the host build of the tests (tests/emu/emu_verify_combined.cpp) run this text.
#pragma once
#include "sha256_h2f.cuh"

#define MI_COMBINE_TAG_LEN 18
MI_HD uint8_t combine_tag(int i) { constexpr char d[MI_COMBINE_TAG_LEN + 1] = "mi355x-g16-combine"; return (uint8_t)d[i]; }
// out: four little-endian words of r_i
MI_HD void combine_coefficient(const uint8_t seed[32], u64 n, u64 i, u32 out[4]) {
    Sha256 s;
    uint8_t d[32];
    sha256_init(&s);
    for (int k = 0; k < MI_COMBINE_TAG_LEN; k++) sha256_byte(&s, combine_tag(k));
    sha256_update(&s, seed, 32);
    for (int k = 0; k < 8; k++) sha256_byte(&s, (uint8_t)(n >> (8 * k)));
    for (int k = 0; k < 8; k++) sha256_byte(&s, (uint8_t)(i >> (8 * k)));
    sha256_final(&s, d);
    for (int w = 0; w < 4; w++) out[w] = (u32)d[4 * w] | ((u32)d[4 * w + 1] << 8) | ((u32)d[4 * w + 2] << 16) | ((u32)d[4 * w + 3] << 24);
}

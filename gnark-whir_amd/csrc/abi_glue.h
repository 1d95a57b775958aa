// Small host helpers the entry-point files share (not part of the C-ABI): a value of the C-ABI as the library's own type, and the
// operating system's randomness (api.hip holds the library's one getrandom call).
#pragma once
#include "ctx.h"
#include "curve.cuh"
#include <cstring>
#include <string>

inline Fr fr_of(const mi_fr &x) { Fr r; std::memcpy(&r, &x, 32); return r; }   // Montgomery words, as they are
inline G1Aff g1_of(const mi_g1_affine &p) { G1Aff a; std::memcpy(&a, &p, sizeof(a)); return a; }
inline G2Aff g2_of(const mi_g2_affine &p) { G2Aff a; std::memcpy(&a, &p, sizeof(a)); return a; }

// n bytes of the operating system's into buf, or MI_ENODEV with msg, the caller's own text
int32_t mi_os_random(mi_ctx *ctx, const std::string &msg, uint8_t *buf, size_t n);
// a drawn Schnorr nonce (phase2_check.hip): 48 bytes of the operating system's reduced mod r (uniform to within 2^-128); a draw of 0 is
// refused.  MI_ENODEV with msg_no_random or msg_zero
int32_t mi_draw_nonce(mi_ctx *ctx, const char *msg_no_random, const char *msg_zero, Fr &k);

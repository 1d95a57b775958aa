// The per-value text of the witness codec (include/mi355x_groth16_vkfile.h): what one lane of k_witness_decode (verify_bytes.hip) does
// with one value of witness.WriteTo's bytes, MI_HD so that mi_public_witness_read (vkfile_inspect.hip) and the host build of the tests
// (tests/emu/emu_witness.cpp, overflow traps on) run the same body.
#pragma once
#include "decode_ops.cuh"

#define MI_WITNESS_HEADER_BYTES 12
// 32 bytes at any alignment, big-endian -> the Montgomery scalar; false when the integer is not below r, and *out = 0: nothing that is
// not reduced reaches the arithmetic (ONE ENCODING, include/mi355x_groth16_verify.h)
MI_HD bool fr_from_be32(Fr *out, const uint8_t *in) {
    Fr c;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint8_t *w = in + 28 - 4 * i;
        c.l[i] = ((u32)w[0] << 24) | ((u32)w[1] << 16) | ((u32)w[2] << 8) | (u32)w[3];
    }
    const bool below = fe_is_reduced(c);
    if (!below) c = Fr::zero();
    *out = fe_to_mont(c);
    return below;
}
MI_HD u32 witness_be32(const uint8_t *b) { return ((u32)b[0] << 24) | ((u32)b[1] << 16) | ((u32)b[2] << 8) | (u32)b[3]; }

// Host build of the per-point text of the key-file codecs (gnark-whir_amd/csrc/keyfile_ops.cuh): the same bodies the bulk kernels of
// keyfile.hip run one lane each, compiled with -DMI_CHECK_NOWRAP so that every bound of the arithmetic underneath traps.
#include <cstddef>
#include "../../gnark-whir_amd/csrc/keyfile_ops.cuh"

extern "C" {
// y[i] = a[i]^((p + 1) / 4) by the fixed window, and by the bit-by-bit chain of the proof decoders
int emu_kf_fp_root(void *y_win, void *y_bits, const void *a, size_t n) {
    for (size_t i = 0; i < n; i++) {
        fp_sqrt_candidate_win4((Fp *)y_win + i, (const Fp *)a + i);
        fp_sqrt_candidate((Fp *)y_bits + i, (const Fp *)a + i);
    }
    return 0;
}
int emu_kf_fp2_sqrt(void *y, const void *a, size_t n, unsigned char *ok) {
    for (size_t i = 0; i < n; i++) ok[i] = fp2_sqrt_win4((Fp2 *)y + i, (const Fp2 *)a + i) ? 1 : 0;
    return 0;
}
int emu_kf_decode_g1(const unsigned char *enc, size_t n, int compressed, void *out, unsigned char *bad) {
    for (size_t i = 0; i < n; i++) bad[i] = g1_decode_stream((G1Aff *)out + i, enc + MI_KEYFILE_G1_BYTES(compressed) * i, compressed != 0) ? 0 : 1;
    return 0;
}
int emu_kf_decode_g2(const unsigned char *enc, size_t n, int compressed, void *out, unsigned char *bad) {
    for (size_t i = 0; i < n; i++) bad[i] = g2_decode_stream((G2Aff *)out + i, enc + MI_KEYFILE_G2_BYTES(compressed) * i, compressed != 0) ? 0 : 1;
    return 0;
}
int emu_kf_encode_g1(const void *pts, size_t n, int compressed, unsigned char *out) {
    for (size_t i = 0; i < n; i++) g1_encode_stream(out + MI_KEYFILE_G1_BYTES(compressed) * i, ((const G1Aff *)pts)[i], compressed != 0);
    return 0;
}
int emu_kf_encode_g2(const void *pts, size_t n, int compressed, unsigned char *out) {
    for (size_t i = 0; i < n; i++) g2_encode_stream(out + MI_KEYFILE_G2_BYTES(compressed) * i, ((const G2Aff *)pts)[i], compressed != 0);
    return 0;
}
// both membership tests on points of the twist: by_psi[i] the endomorphism test, by_r[i] g2_in_subgroup's [r] Q
int emu_kf_subgroup(const void *pts, size_t n, unsigned char *by_psi, unsigned char *by_r) {
    for (size_t i = 0; i < n; i++) {
        by_psi[i] = g2_in_subgroup_psi((const G2Aff *)pts + i) ? 1 : 0;
        by_r[i] = g2_in_subgroup((const G2Aff *)pts + i) ? 1 : 0;
    }
    return 0;
}
}

// Host build of what reads a proof's bytes (gnark-whir_amd/csrc/decode_ops.cuh, sha256_h2f.cuh): the same bodies the kernels of
// verify_bytes.hip and the host entry points of proof_read.hip run, compiled with -DMI_CHECK_NOWRAP so that every bound of the arithmetic
// underneath traps.  The host twins of mi_debug_decode_g1_dev / _g2_dev / mi_debug_hash_to_field_dev (same layouts), and one whole proof
// from its bytes the way mi_groth16_verify_bytes judges it.
#include <cstddef>
#include <cstring>
#include "../../gnark-whir_amd/csrc/pairing_ops.cuh"
#include "../../gnark-whir_amd/csrc/sha256_h2f.cuh"

extern "C" {
// ok[i] = 1 when y[i]^2 == a[i]; y[i] is written either way
int emu_fp_sqrt(void *y, const void *a, size_t n, unsigned char *ok) {
    for (size_t i = 0; i < n; i++) ok[i] = fp_sqrt((Fp *)y + i, ((const Fp *)a)[i]) ? 1 : 0;
    return 0;
}
int emu_fp2_sqrt(void *y, const void *a, size_t n, unsigned char *ok) {
    for (size_t i = 0; i < n; i++) ok[i] = fp2_sqrt((Fp2 *)y + i, (const Fp2 *)a + i) ? 1 : 0;
    return 0;
}
int emu_decode_g1(const unsigned char *enc, size_t n, void *out, unsigned char *bad) {
    for (size_t i = 0; i < n; i++) bad[i] = g1_decode((G1Aff *)out + i, enc + 32 * i) ? 0 : 1;
    return 0;
}
int emu_decode_g2(const unsigned char *enc, size_t n, void *out, unsigned char *bad) {
    for (size_t i = 0; i < n; i++) bad[i] = g2_decode((G2Aff *)out + i, enc + 64 * i) ? 0 : 1;
    return 0;
}
int emu_sha256(const unsigned char *msg, size_t len, unsigned char *out) {
    Sha256 s;
    sha256_init(&s);
    sha256_update(&s, msg, len);
    sha256_final(&s, out);
    return 0;
}
int emu_expand_xmd48(const unsigned char *dst, unsigned dst_len, const unsigned char *msg, size_t len, unsigned char *out) {
    Sha256 s;
    h2f_begin(&s);
    sha256_update(&s, msg, len);
    h2f_expand_finish(&s, dst, dst_len, out);
    return 0;
}
int emu_fr_from_be48(const unsigned char *in, void *out) {
    *(Fr *)out = fr_from_be48(in);
    return 0;
}
int emu_hash_to_field(const unsigned char *dst, unsigned dst_len, const unsigned char *msgs, size_t msg_len, size_t n, void *out) {
    for (size_t i = 0; i < n; i++) ((Fr *)out)[i] = hash_to_field(dst, dst_len, msgs + i * msg_len, msg_len);
    return 0;
}
int emu_bsb22_hashes(const void *commitments, unsigned nc, const void *public_inputs, unsigned n_pub, const unsigned *pc_off, const unsigned *pc_idx,
                     void *values, void *fold) {
    bsb22_hashes((const G1Aff *)commitments, nc, (const Fr *)public_inputs, n_pub, pc_off, pc_idx, (Fr *)values, (Fr *)fold);
    return 0;
}
// One whole proof from its bytes the way mi_groth16_verify_bytes judges it, host half included: the framing (-1), the count, the
// decoders, the hashes, then emu_pairing.cpp's emu_verify_assemble line by line (verify_well_formed, a naive MSM, verify_assemble, the
// Bs check, the Miller loops, verify_judge).  k: nb_public + nc points; ped: 2 nc twist points; pc_off / pc_idx: the committed lists.
// decoded (may be null): (4 + nc) * 8 + 8 words -- Ar | Bs | Krs | commitments | pok as the decoders wrote them.
int emu_verify_bytes(const void *k, const void *gamma2, const void *delta2, const void *ped, unsigned nb_public, unsigned nc, const void *e_alpha_beta,
                     const unsigned char *proof, size_t proof_len, const void *public_inputs, const unsigned *pc_off, const unsigned *pc_idx, void *decoded) {
    if (nb_public == 0 || nc > 16 || proof_len != proof_bytes_len(nc)) return -1;
    const G1Aff *kk = (const G1Aff *)k;
    const unsigned n_pub = nb_public - 1, np = verify_pairs_per_proof(nc);
    bool malformed = proof_bytes_count(proof) != nc;
    G1Aff g[3 + 16];
    G2Aff bs;
    for (unsigned s = 0; s < proof_g1_slots(nc); s++) malformed = !g1_decode(&g[s], proof + proof_g1_slot_offset(s)) || malformed;
    malformed = !g2_decode(&bs, proof + MI_PROOF_OFF_BS) || malformed;
    if (decoded) {
        char *d = (char *)decoded;
        std::memcpy(d, &g[0], sizeof(G1Aff)); std::memcpy(d + sizeof(G1Aff), &bs, sizeof(G2Aff)); std::memcpy(d + sizeof(G1Aff) + sizeof(G2Aff), &g[1], sizeof(G1Aff));
        std::memcpy(d + 2 * sizeof(G1Aff) + sizeof(G2Aff), &g[2], (nc + 1) * sizeof(G1Aff));
    }
    Fr values[16] = {}, fold = Fr::zero();
    if (!malformed && nc) bsb22_hashes(g + 2, nc, (const Fr *)public_inputs, n_pub, pc_off, pc_idx, values, &fold);
    const VerifyKeyRef vk{kk, (const G2Aff *)gamma2, (const G2Aff *)delta2, (const G2Aff *)ped, n_pub, nc};
    const VerifyProofRef in{&g[0], &bs, &g[1], g + 2, g + 2 + nc, (const Fr *)public_inputs, values, &fold};
    malformed = malformed || !verify_well_formed(vk, in);
    G1X msm = G1X::inf();
    if (!malformed)
        for (unsigned i = 0; i < n_pub + nc; i++) {
            const Fr s = i < n_pub ? in.public_inputs[i] : in.commitment_values[i - n_pub];
            xyzz_add(msm, xyzz_mul_256(G1X::from_affine(kk[1 + i]), fe_from_mont(s).l));
        }
    G1Aff p[MI_VERIFY_GROTH_PAIRS + 17];
    G2Aff q[MI_VERIFY_GROTH_PAIRS + 17];
    verify_assemble(vk, in, !malformed, xyzz_to_affine(msm), p, q);
    if (!g2_in_subgroup(&q[0])) malformed = true;
    Fp12 ml[MI_VERIFY_GROTH_PAIRS + 17];
    for (unsigned i = 0; i < np; i++) pairing_miller_loop(&ml[i], &p[i], &q[i]);
    return verify_judge(ml, np - MI_VERIFY_GROTH_PAIRS, (const Fp12 *)e_alpha_beta, malformed);
}
// e(alpha, beta)^d', what mi_vk_load computes once
int emu_pairing_one(const void *p, const void *q, void *gt) {
    Fp12 f;
    pairing_miller_loop(&f, (const G1Aff *)p, (const G2Aff *)q);
    pairing_final_exp(&f, &f);
    *(Fp12 *)gt = f;
    return 0;
}
}

// Mutation driver for the reader of a proof's bytes: mi_proof_read, mi_hash_to_field and the decoders under them (gnark-whir_amd/csrc/
// proof_read.hip, decode_ops.cuh, sha256_h2f.cuh), built as plain C++ with -fsanitize=address,undefined (gnark-whir_amd/Makefile
// `sanitize-decode`) and run by tests/test_decode_cpu.py.  Seeds are valid proofs written by the same encoders' rules (the generator and
// infinity, so no point arithmetic is needed here); the mutants are bit flips, byte splices, wrong counts and every truncation, with every
// length from 0 to 164 + 32 * 17.  Each input lives in a heap block of exactly its length, so a read past the end is a report.
//     decode_fuzz <seed>      prints "<accepted> <refused>", exits 0 when every contract held
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/mi355x_groth16_verify_bytes.h"

static uint64_t state;
static uint64_t rnd() {   // splitmix64
    uint64_t z = (state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static long accepted, refused;

static bool all_zero(const void *p, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (((const unsigned char *)p)[i]) return false;
    return true;
}
static int run(const std::vector<uint8_t> &v, uint32_t nc) {
    uint8_t *blk = (uint8_t *)std::malloc(v.size() ? v.size() : 1);   // exactly as long as the input
    if (!blk) return 1;
    if (!v.empty()) std::memcpy(blk, v.data(), v.size());
    mi_proof_out proof;
    mi_g1_affine pok;
    std::vector<mi_g1_affine> cm(nc ? nc : 1);
    std::memset(&proof, 0xAA, sizeof(proof)); std::memset(&pok, 0xAA, sizeof(pok)); std::memset(cm.data(), 0xAA, cm.size() * sizeof(mi_g1_affine));
    const int32_t rc = mi_proof_read(blk, v.size(), nc, &proof, nc ? cm.data() : nullptr, &pok);
    int bad = 0;
    if (rc == MI_OK) {
        accepted++;
        if (v.size() != 164 + 32 * (size_t)nc) bad = 1;   // accepted with another length
    } else {
        refused++;
        if (rc != MI_EINVAL) bad = 3;
        if (!all_zero(&proof, sizeof(proof)) || !all_zero(&pok, sizeof(pok))) bad = 4;   // a refusal leaves infinities, not half a proof
    }
    mi_fr h;
    if (mi_hash_to_field((const uint8_t *)"fuzz", 4, blk, v.size(), &h) != MI_OK) bad = 5;
    std::free(blk);
    if (bad) std::fprintf(stderr, "contract %d broken at length %zu, nc %u\n", bad, v.size(), nc);
    return bad;
}

int main(int argc, char **argv) {
    state = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
    int bad = 0;
    for (uint32_t nc = 0; nc <= 17 && !bad; nc++) {
        // a valid seed: Ar = the generator (80 00 .. 01), Bs and Krs infinity, commitments alternate, pok the generator
        std::vector<uint8_t> seed(164 + 32 * (size_t)nc, 0);
        seed[0] = 0x80; seed[31] = 1; seed[32] = 0x40; seed[96] = 0x40;
        seed[131] = (uint8_t)nc;
        for (uint32_t k = 0; k <= nc; k++) {
            uint8_t *q = &seed[132 + 32 * (size_t)k];
            if (k & 1) q[0] = 0x40; else { q[0] = 0x80; q[31] = 1; }
        }
        if (nc <= 16) { bad |= run(seed, nc); if (accepted == 0) { std::fprintf(stderr, "the seed of nc %u was refused\n", nc); bad = 6; } }
        for (size_t len = 0; len <= seed.size() && !bad; len++) {   // every truncation, against the right and a wrong count
            std::vector<uint8_t> t(seed.begin(), seed.begin() + len);
            bad |= run(t, nc);
            if (len + 1 == seed.size() || len % 37 == 0) bad |= run(t, (uint32_t)(rnd() % 19));
        }
        for (int m = 0; m < 600 && !bad; m++) {
            std::vector<uint8_t> t = seed;
            const int kind = (int)(rnd() % 5);
            if (kind == 0) t[rnd() % t.size()] ^= (uint8_t)(1u << (rnd() % 8));
            else if (kind == 1) for (int k = 0; k < 8; k++) t[rnd() % t.size()] = (uint8_t)rnd();
            else if (kind == 2) { const size_t at = 32 * (rnd() % (t.size() / 32)); for (int k = 0; k < 32 && at + k < t.size(); k++) t[at + k] = (uint8_t)rnd(); t[at] |= 0x80; t[at] &= 0xEF; }
            else if (kind == 3) t[128 + rnd() % 4] = (uint8_t)rnd();
            else t.resize(rnd() % (164 + 32 * 17 + 1), (uint8_t)rnd());
            bad |= run(t, nc);
        }
    }
    std::printf("%ld %ld\n", accepted, refused);
    return bad ? 1 : 0;
}

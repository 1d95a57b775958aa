// Stand-alone host run of the sigma chain of a phase-2 ceremony (gnark-whir_amd/csrc/ceremony_ops.cuh: the hash, the challenge and the
// making of a step over the twist) and of mi_phase2_sigma_records_verify (csrc/phase2_records.hip, which holds no HIP call): built with
// -fsanitize=address,undefined by `make sanitize-phase2-sigma`, run by tests/test_phase2_sigma_cpu.py, which holds the cases and
// compares what this prints with hashlib and oracle/pyref.py.  It stands beside tests/cpp/phase2_check_host.cpp, which does the same
// for the delta chain over G1.  The proofs and the hashes of a chain are heap blocks of exactly m * nc proofs and m hashes.
//
// Commands on stdin, one per line; every number is a plain integer in hex (scalars below r), <id>: 64 hex digits = 32 bytes:
//     sigma <id> <first_index> <nc> <e_start> x nc <m> ((<s> <nonce>) x nc) x m <tamper> <i> <k>
//                                                        m steps of nc commitments from g_sigma_neg_k = e_start_k g2 with the chain
//                                                        value <id>; prints each step (per commitment g_sigma_neg, commit, response:
//                                                        one line each, then the step's hash), then tampers and prints
//                                                        "rc <rc> first_bad <n>" of mi_phase2_sigma_records_verify.  tamper: none |
//                                                        response (commitment k of step i: + 1) | responser (its words + r) | commit |
//                                                        after (replaced by 5 g2) | offtwist (one bit of after's x) | infinity (commit
//                                                        zeroed) | hashbyte (one bit of step i's hash) | swap (steps i, i + 1) | index
//                                                        (first_index + 1) | starthash (one bit of <id>) | null (a null argument) |
//                                                        nczero | startinf | startoff (start point k)
// A point of the twist prints as x.a0 x.a1 y.a0 y.a1 in hex, or "inf".
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <cstring>
#include "../../include/mi355x_groth16_phase2_check.h"
#include "../../gnark-whir_amd/csrc/ceremony_ops.cuh"

namespace {

template <class P>
Fe<P> fe_from_hex(const std::string &h) {
    Fe<P> t = Fe<P>::zero();
    int bit = 0;
    for (size_t i = h.size(); i-- > 0 && bit < 256; bit += 4) {
        const char c = h[i];
        const u32 v = c >= '0' && c <= '9' ? (u32)(c - '0') : c >= 'a' && c <= 'f' ? (u32)(c - 'a' + 10) : (u32)(c - 'A' + 10);
        t.l[bit >> 5] |= v << (bit & 31);
    }
    return fe_to_mont(t);
}
bool bytes_from_hex(const std::string &h, uint8_t out[32]) {
    if (h.size() != 64) return false;
    for (int i = 0; i < 32; i++) out[i] = (uint8_t)std::strtoul(h.substr(2 * (size_t)i, 2).c_str(), nullptr, 16);
    return true;
}
void print_bytes(const uint8_t *b, int n) {
    for (int i = 0; i < n; i++) std::printf("%02x", b[i]);
    std::printf("\n");
}
template <class P>
void print_fe(const Fe<P> &x) {
    const Fe<P> c = fe_from_mont(x);
    for (int i = 7; i >= 0; i--) std::printf("%08x", c.l[i]);
}
void print_point2(const G2Aff &p) {
    if (p.is_inf()) { std::printf("inf\n"); return; }
    print_fe(p.x.a0); std::printf(" "); print_fe(p.x.a1); std::printf(" "); print_fe(p.y.a0); std::printf(" "); print_fe(p.y.a1); std::printf("\n");
}
G2Aff g2_times(const Fr &e) { return xyzz_to_affine(xyzz_scale(G2X::from_affine(g2_generator()), e)); }

bool run(const std::string &cmd, std::istringstream &in) {
    if (cmd == "sigma") {
        std::string id, first;
        uint32_t nc = 0;
        size_t m = 0;
        in >> id >> first >> std::dec >> nc;
        uint8_t start_hash[32];
        if (!in || !bytes_from_hex(id, start_hash) || !nc || nc > 8) return false;
        uint64_t first_index = std::strtoull(first.c_str(), nullptr, 16);
        std::unique_ptr<mi_g2_affine[]> start(new mi_g2_affine[nc]);
        std::unique_ptr<G2Aff[]> before(new G2Aff[nc]), after(new G2Aff[nc]);
        std::unique_ptr<Fr[]> ss(new Fr[nc]), nn(new Fr[nc]);
        for (uint32_t k = 0; k < nc; k++) {
            std::string e;
            in >> e;
            before[k] = g2_times(fe_from_hex<FrParams>(e));
            std::memcpy(&start[k], &before[k], sizeof(G2Aff));
        }
        in >> std::dec >> m;
        if (!in || m > 16) return false;
        std::unique_ptr<mi_phase2_sigma_proof[]> proofs(new mi_phase2_sigma_proof[m ? m * nc : 1]);
        std::unique_ptr<uint8_t[][32]> hashes(new uint8_t[m ? m : 1][32]);
        uint8_t prev[32];
        std::memcpy(prev, start_hash, 32);
        for (size_t i = 0; i < m; i++) {
            for (uint32_t k = 0; k < nc; k++) {
                std::string sv, nv;
                in >> sv >> nv;
                ss[k] = fe_from_hex<FrParams>(sv); nn[k] = fe_from_hex<FrParams>(nv);
                after[k] = xyzz_to_affine(xyzz_scale(G2X::from_affine(before[k]), ss[k]));
            }
            std::unique_ptr<CeremonySigmaProof[]> step(new CeremonySigmaProof[nc]);
            ceremony_sigma_step_make(prev, first_index + i, nc, before.get(), after.get(), ss.get(), nn.get(), step.get(), hashes[i]);
            std::memcpy(&proofs[i * nc], step.get(), nc * sizeof(CeremonySigmaProof));
            for (uint32_t k = 0; k < nc; k++) {
                print_point2(step[k].g_sigma_neg); print_point2(step[k].commit); print_fe(step[k].response); std::printf("\n");
                before[k] = after[k];
            }
            print_bytes(hashes[i], 32);
            std::memcpy(prev, hashes[i], 32);
        }
        std::string tamper;
        size_t at = 0;
        uint32_t k = 0;
        in >> tamper >> at >> k;
        if (!in || k >= nc || (m && at >= m && tamper != "none") || (!m && tamper != "none") || (tamper == "swap" && at + 1 >= m)) return false;
        const mi_g2_affine *start_arg = start.get();
        mi_phase2_sigma_proof *hit = m ? &proofs[at * nc + k] : nullptr;
        if (tamper == "response") {
            Fr z;
            std::memcpy(&z, &hit->response, 32);
            z = z + Fr::one();
            std::memcpy(&hit->response, &z, 32);
        } else if (tamper == "responser") {   // the same element of the field in words that are not below r
            Fr z;
            std::memcpy(&z, &hit->response, 32);
            fe_add_raw(z, z, Fr::modulus());   // 2 r < 2^256: no carry out
            std::memcpy(&hit->response, &z, 32);
        } else if (tamper == "commit" || tamper == "after") {
            const G2Aff other = g2_times(fe_from_u32<FrParams>(5));
            std::memcpy(tamper == "commit" ? &hit->commit : &hit->g_sigma_neg, &other, sizeof(other));
        } else if (tamper == "offtwist") {
            reinterpret_cast<uint8_t *>(&hit->g_sigma_neg)[0] ^= 1;
        } else if (tamper == "infinity") {
            std::memset(&hit->commit, 0, sizeof(hit->commit));
        } else if (tamper == "hashbyte") {
            hashes[at][17] ^= 0x10;
        } else if (tamper == "swap") {
            for (uint32_t j = 0; j < nc; j++) std::swap(proofs[at * nc + j], proofs[(at + 1) * nc + j]);
            uint8_t t[32];
            std::memcpy(t, hashes[at], 32); std::memcpy(hashes[at], hashes[at + 1], 32); std::memcpy(hashes[at + 1], t, 32);
        } else if (tamper == "index") {
            first_index++;
        } else if (tamper == "starthash") {
            start_hash[31] ^= 1;
        } else if (tamper == "null") {
            start_arg = nullptr;
        } else if (tamper == "nczero") {
            nc = 0;
        } else if (tamper == "startinf") {
            std::memset(&start[k], 0, sizeof(mi_g2_affine));
        } else if (tamper == "startoff") {
            reinterpret_cast<uint8_t *>(&start[k])[0] ^= 1;
        } else if (tamper != "none") {
            return false;
        }
        uint64_t first_bad = ~(uint64_t)0;
        const int32_t rc = mi_phase2_sigma_records_verify(start_arg, nc, start_hash, first_index, proofs.get(), hashes.get(), m, &first_bad);
        std::printf("rc %d first_bad %llu\n", rc, (unsigned long long)first_bad);
    } else {
        return false;
    }
    return (bool)in;
}

}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        std::printf("%s\n", line.c_str());
        if (!run(cmd, in)) { std::printf("malformed command\n"); return 2; }
    }
    return 0;
}

// Stand-alone host run of what the ceremony checks hash and judge on the host (gnark-whir_amd/csrc/ceremony_ops.cuh: the coefficient of
// a same-ratio test, the hash and the challenge of a contribution's record, the making of a record) and of mi_phase2_records_verify
// (csrc/phase2_records.hip, which holds no HIP call): built with -fsanitize=address,undefined by `make sanitize-phase2-check`, run by
// tests/test_phase2_check_cpu.py, which holds the cases and compares what this prints with hashlib and oracle/pyref.py.  The records
// of a chain are a heap block of exactly m records.
//
// Commands on stdin, one per line; every number is a plain integer in hex (scalars below r), <seed>, <id>: 64 hex digits = 32 bytes:
//     coeff <seed> <k>                                   prints r_k
//     hash  <id> <index> <e_before> <e_after> <e_commit> the points are e g1; prints the record hash, then its challenge
//     chain <id> <first_index> <e_start> <m> (<d> <nonce>) x m <tamper> <i>
//                                                        m records from delta1 = e_start g1 with the chain hash <id>; prints each record
//                                                        (delta1, commit, response, hash: one line each), then tampers and prints
//                                                        "rc <rc> first_bad <n>" of mi_phase2_records_verify.  tamper: none | response
//                                                        (record i's + 1) | commit | delta1 (record i's replaced by 5 g1) | hashbyte
//                                                        (one bit of record i's hash) | swap (records i, i + 1) | index (first_index + 1)
//                                                        | starthash (one bit of <id>) | null (a null argument)
// A point prints as its affine coordinates in hex, or "inf".
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
void print_point(const G1Aff &p) {
    if (p.is_inf()) { std::printf("inf\n"); return; }
    print_fe(p.x); std::printf(" "); print_fe(p.y); std::printf("\n");
}
G1Aff g1_times(const Fr &e) { return xyzz_to_affine(xyzz_scale(G1X::from_affine(G1Aff{Fp::one(), fe_from_u32<FpParams>(2)}), e)); }

bool run(const std::string &cmd, std::istringstream &in) {
    if (cmd == "coeff") {
        std::string seed, k;
        in >> seed >> k;
        uint8_t s[32];
        if (!bytes_from_hex(seed, s)) return false;
        u32 w[4];
        ceremony_coefficient(s, std::strtoull(k.c_str(), nullptr, 16), w);
        std::printf("%08x%08x%08x%08x\n", w[3], w[2], w[1], w[0]);
    } else if (cmd == "hash") {
        std::string id, index, eb, ea, ec;
        in >> id >> index >> eb >> ea >> ec;
        uint8_t prev[32], h[32];
        if (!bytes_from_hex(id, prev)) return false;
        ceremony_record_hash(prev, std::strtoull(index.c_str(), nullptr, 16), g1_times(fe_from_hex<FrParams>(eb)), g1_times(fe_from_hex<FrParams>(ea)),
                             g1_times(fe_from_hex<FrParams>(ec)), h);
        print_bytes(h, 32);
        u32 c[4];
        ceremony_challenge(h, c);
        std::printf("%08x%08x%08x%08x\n", c[3], c[2], c[1], c[0]);
    } else if (cmd == "chain") {
        std::string id, first, es;
        size_t m = 0;
        in >> id >> first >> es >> std::dec >> m;
        uint8_t start_hash[32];
        if (!bytes_from_hex(id, start_hash) || m > 64) return false;
        uint64_t first_index = std::strtoull(first.c_str(), nullptr, 16);
        const G1Aff start = g1_times(fe_from_hex<FrParams>(es));
        std::unique_ptr<mi_phase2_record[]> rec(new mi_phase2_record[m ? m : 1]);
        G1Aff before = start;
        uint8_t prev[32];
        std::memcpy(prev, start_hash, 32);
        for (size_t i = 0; i < m; i++) {
            std::string d, k;
            in >> d >> k;
            const Fr dd = fe_from_hex<FrParams>(d), kk = fe_from_hex<FrParams>(k);
            CeremonyRecord r;
            ceremony_record_make(prev, first_index + i, before, xyzz_to_affine(xyzz_scale(G1X::from_affine(before), dd)), dd, kk, &r);
            std::memcpy(&rec[i], &r, sizeof(r));
            print_point(r.delta1); print_point(r.commit); print_fe(r.response); std::printf("\n"); print_bytes(r.hash, 32);
            before = r.delta1;
            std::memcpy(prev, r.hash, 32);
        }
        std::string tamper;
        size_t at = 0;
        in >> tamper >> at;
        if (!in || (m && at >= m && tamper != "none") || (tamper == "swap" && at + 1 >= m)) return false;
        mi_g1_affine start_words;
        std::memcpy(&start_words, &start, sizeof(start));
        const mi_g1_affine *start_arg = &start_words;
        if (tamper == "response") {
            Fr z;
            std::memcpy(&z, &rec[at].response, 32);
            z = z + Fr::one();
            std::memcpy(&rec[at].response, &z, 32);
        } else if (tamper == "commit" || tamper == "delta1") {
            const G1Aff other = g1_times(fe_from_u32<FrParams>(5));
            std::memcpy(tamper == "commit" ? &rec[at].commit : &rec[at].delta1, &other, sizeof(other));
        } else if (tamper == "hashbyte") {
            rec[at].hash[17] ^= 0x10;
        } else if (tamper == "swap") {
            std::swap(rec[at], rec[at + 1]);
        } else if (tamper == "index") {
            first_index++;
        } else if (tamper == "starthash") {
            start_hash[31] ^= 1;
        } else if (tamper == "null") {
            start_arg = nullptr;
        } else if (tamper != "none") {
            return false;
        }
        uint64_t first_bad = ~(uint64_t)0;
        const int32_t rc = mi_phase2_records_verify(start_arg, start_hash, first_index, rec.get(), m, &first_bad);
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

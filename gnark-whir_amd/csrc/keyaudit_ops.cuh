// What the audit of a key (include/mi355x_groth16_keyaudit.h) runs per lane, MI_HD, and its host-only bookkeeping: the kernels of
// keyaudit.hip and the host build of the tests (tests/cpp/keyaudit_host.cpp) run this text.
//
// Per lane:
//   keyaudit_masked        r^X[j]: the coefficient of a wire of class X, 0 for the others
//   keyaudit_bitrev        the index permutation of pk.G1.Z and of a DIF transform's output
//   keyaudit_g1_ok / _g2_ok   a claimed point: reduced words, on its curve; (0, 0) passes where the array may hold it -- the audit's
//                          name for point_check.cuh's point_ok under POINT_RULE_AUDIT, which is what the kernels run
// Host only:
//   keyaudit_wire_lists    the wire classes and, per compacted array of the key, the wires of its slots in order
//   keyaudit_shape_refusal a claim whose counts are not the circuit's: the text that names the count
#pragma once
#include "pairing_ops.cuh"
#include "point_check.cuh"
#include <string>
#include <vector>

enum { KEYAUDIT_P = 0, KEYAUDIT_V = 1, KEYAUDIT_C = 2, KEYAUDIT_CLASSES = 3 };   // private / public + commitment wires / committed

MI_HD Fr keyaudit_masked(const Fr &r, uint8_t cls, uint8_t want) { return cls == want ? r : Fr::zero(); }
MI_HD bool keyaudit_g1_ok(const G1Aff &p, bool allow_inf) { return point_ok(p, point_rule_audit(allow_inf)); }
MI_HD bool keyaudit_g2_ok(const G2Aff &q, bool allow_inf) { return point_ok(q, point_rule_audit(allow_inf)); }
MI_HD u64 keyaudit_bitrev(u64 i, u32 log_n) {
    u64 r = 0;
    for (u32 b = 0; b < log_n; b++) { r = (r << 1) | (i & 1); i >>= 1; }
    return r;
}

// ---------------------------------------------------------------------------------------------------- host only
// what the audit reads of a circuit once mi_r1cs_validate has passed it: every list holds private wires, no wire twice
struct KeyAuditCircuit {
    u64 N = 0, nb_wires = 0;
    u32 nb_public = 0, n_commitments = 0;
    const uint32_t *const *committed = nullptr;
    const uint64_t *n_committed = nullptr;
    const uint32_t *commitment_wire = nullptr;
};
// the counts of a claim
struct KeyAuditCounts {
    u64 nb_wires = 0, n_a = 0, n_b = 0, n_g2_b = 0, n_k = 0, n_z = 0, n_vk = 0;
    std::vector<u64> n_basis;   // one per Pedersen key of the proving key
    u64 n_vk_ped = 0;           // Pedersen pairs of the verifying key
};
struct KeyAuditWires {
    std::vector<uint8_t> cls;                  // nb_wires: KEYAUDIT_P / _V / _C
    std::vector<u32> a, b, k, v;               // the wires of pk.G1.A / pk.G1.B (+ G2.B) / pk.G1.K / vk.G1.K, slot by slot
    std::vector<std::vector<u32>> c;           // the wires of Basis[k], slot by slot
};
// inf_a, inf_b: a byte per wire, non-zero = the wire owns no point of A / B
inline void keyaudit_wire_lists(const KeyAuditCircuit &cs, const uint8_t *inf_a, const uint8_t *inf_b, KeyAuditWires &w) {
    w.cls.assign((size_t)cs.nb_wires, (uint8_t)KEYAUDIT_P);
    for (u64 j = 0; j < cs.nb_public && j < cs.nb_wires; j++) w.cls[(size_t)j] = KEYAUDIT_V;
    w.c.assign(cs.n_commitments, std::vector<u32>());
    std::vector<u32> cw;
    for (u32 k = 0; k < cs.n_commitments; k++) {
        for (u64 i = 0; i < cs.n_committed[k]; i++) {
            const u32 j = cs.committed[k][i];
            w.cls[j] = KEYAUDIT_C;
            w.c[k].push_back(j);
        }
        w.cls[cs.commitment_wire[k]] = KEYAUDIT_V;
    }
    w.a.clear(); w.b.clear(); w.k.clear(); w.v.clear();
    for (u64 j = 0; j < cs.nb_wires; j++) {
        if (!inf_a[j]) w.a.push_back((u32)j);
        if (!inf_b[j]) w.b.push_back((u32)j);
        if (w.cls[(size_t)j] == KEYAUDIT_P) w.k.push_back((u32)j);
        if (w.cls[(size_t)j] == KEYAUDIT_V) w.v.push_back((u32)j);   // public wires, then the commitment wires ascending
    }
}
// "" when the claim has the circuit's shape, else what mi_last_error says (w: keyaudit_wire_lists over the CLAIM's masks)
inline std::string keyaudit_shape_refusal(const KeyAuditCircuit &cs, const KeyAuditCounts &c, const KeyAuditWires &w) {
    auto differs = [](const char *what, u64 have, const char *why, u64 want) {
        return std::string("key audit: claim.") + what + " is " + std::to_string(have) + ", " + why + " " + std::to_string(want);
    };
    if (c.nb_wires != cs.nb_wires) return differs("nb_wires", c.nb_wires, "the circuit has", cs.nb_wires);
    if (c.n_z != cs.N) return differs("n_z", c.n_z, "the circuit's domain N is", cs.N);
    if (c.n_a != w.a.size()) return differs("n_a", c.n_a, "the clear bytes of infinity_a number", w.a.size());
    if (c.n_b != w.b.size()) return differs("n_b", c.n_b, "the clear bytes of infinity_b number", w.b.size());
    if (c.n_g2_b != w.b.size()) return differs("n_g2_b", c.n_g2_b, "the clear bytes of infinity_b number", w.b.size());
    if (c.n_k != w.k.size()) return differs("n_k", c.n_k, "the private wires that are neither committed nor a commitment wire number", w.k.size());
    if (c.n_vk != (u64)cs.nb_public + cs.n_commitments) return differs("vk.n_k", c.n_vk, "nb_public + n_commitments is", (u64)cs.nb_public + cs.n_commitments);
    if (c.n_basis.size() != cs.n_commitments) return differs("n_ped", c.n_basis.size(), "the circuit's n_commitments is", cs.n_commitments);
    if (c.n_vk_ped != cs.n_commitments) return differs("vk.n_commitments", c.n_vk_ped, "the circuit's n_commitments is", cs.n_commitments);
    for (u32 k = 0; k < cs.n_commitments; k++)
        if (c.n_basis[k] != cs.n_committed[k])
            return differs(("n_basis[" + std::to_string(k) + "]").c_str(), c.n_basis[k], ("n_committed[" + std::to_string(k) + "] is").c_str(), cs.n_committed[k]);
    return std::string();
}

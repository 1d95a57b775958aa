// Stand-alone host run of the key audit's host-only bookkeeping and of its per-lane text (gnark-whir_amd/csrc/keyaudit_ops.cuh: the wire
// classes, the wires of every compacted array slot by slot, the shape refusals, the index permutation and the class mask) and of the one
// point predicate (gnark-whir_amd/csrc/point_check.cuh) over every rule and input, against the three predicates it replaced: built with -fsanitize=address,undefined by `make sanitize-keyaudit`, run by tests/test_keyaudit_cpu.py.  Every list lives in a
// heap block of exactly its length, so a slot past an end is an error the sanitizer reports.  Prints "keyaudit host: ok".
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>
#include "../../gnark-whir_amd/csrc/keyaudit_ops.cuh"
#include "../../gnark-whir_amd/csrc/point_check.cuh"

namespace {

int fails = 0;
void expect(bool ok, const char *what) {
    if (!ok) { std::printf("FAIL: %s\n", what); fails++; }
}
bool names(const std::string &msg, const char *count) { return msg.find(count) != std::string::npos; }

// ---- the three predicates the kernels ran before point_check.cuh, copied as they stood: the expected table of the matrix below
// phase2.hip, k_phase2_check_g1 / _g2 (an SRS row): on the curve and not at infinity; the words are not asked to be reduced
bool old_on_curve(const G1Aff &p) { return fe_sqr(p.y) == fe_sqr(p.x) * p.x + curve_b((const Fp *)0); }
bool old_on_curve(const G2Aff &p) { return fe_sqr(p.y) == fe_sqr(p.x) * p.x + fp12c_twist_b(); }
template <class A> bool old_srs_row(const A &p) { return !(p.is_inf() || !old_on_curve(p)); }
// phase2_check.hip, k_ceremony_claim_check (a claimed array): pairing.cuh's g1_on_curve -- reduced words, on the curve, infinity passes
bool old_claim(const G1Aff &p) {
    if (!g1_reduced(p)) return false;
    if (p.is_inf()) return true;
    return fe_sqr(p.y) == fe_sqr(p.x) * p.x + curve_b((const Fp *)0);
}
// keyaudit_ops.cuh, keyaudit_g1_ok / _g2_ok as they stood (an array of a key claim)
bool old_audit(const G1Aff &p, bool allow_inf) { return old_claim(p) && (allow_inf || !p.is_inf()); }
bool old_audit(const G2Aff &q, bool allow_inf) { return g2_reduced(q) && g2_on_twist(q) && (allow_inf || !q.is_inf()); }

// x + q, word by word: still below 2^256
Fp plus_modulus(const Fp &x) {
    const Fp q = Fp::modulus();
    Fp out;
    uint64_t carry = 0;
    for (int i = 0; i < 8; i++) { const uint64_t t = (uint64_t)x.l[i] + q.l[i] + carry; out.l[i] = (u32)t; carry = t >> 32; }
    if (carry) { std::printf("FAIL: x + q does not fit 256 bits\n"); fails++; }
    return out;
}
// the five inputs of one curve: a good point, infinity, a point off the curve, the good point with x + q, and (q, q)
template <class A>
void point_matrix(const char *curve, const A (&in)[5]) {
    const char *const input[5] = {"good", "infinity", "off curve", "x + q", "(q, q)"};
    // want[rule][input], stated: what every rule bit is for
    const bool want[4][5] = {/* POINT_RULE_SRS_ROW            */ {true, false, false, true, false},
                             /* POINT_ALLOW_INF alone         */ {true, true, false, true, false},
                             /* POINT_NEED_REDUCED (audit)    */ {true, false, false, false, false},
                             /* both (a claim; audit + inf)   */ {true, true, false, false, false}};
    for (u32 rule = 0; rule < 4; rule++)
        for (int k = 0; k < 5; k++) {
            const std::string what = std::string(curve) + ", rule " + std::to_string(rule) + ", " + input[k];
            expect(point_ok(in[k], rule) == want[rule][k], what.c_str());
        }
    for (int k = 0; k < 5; k++) {
        const std::string what = std::string(curve) + ", " + input[k] + ": against the predicate it replaced";
        expect(point_ok(in[k], POINT_RULE_SRS_ROW) == old_srs_row(in[k]), what.c_str());
        expect(point_ok(in[k], point_rule_audit(false)) == old_audit(in[k], false), what.c_str());
        expect(point_ok(in[k], point_rule_audit(true)) == old_audit(in[k], true), what.c_str());
        expect(point_ok(in[k], POINT_ALLOW_INF) == (in[k].is_inf() || old_srs_row(in[k])), what.c_str());
    }
}

}  // namespace

int main() {
    // 12 wires, 3 public; commitment 0 commits to wires 4, 6 and owns wire 8; commitment 1 commits to wire 5 and owns wire 9
    const u64 nw = 12;
    std::unique_ptr<uint32_t[]> c0(new uint32_t[2]{4, 6}), c1(new uint32_t[1]{5}), cw(new uint32_t[2]{8, 9});
    std::unique_ptr<uint64_t[]> nco(new uint64_t[2]{2, 1});
    const uint32_t *lists[2] = {c0.get(), c1.get()};
    KeyAuditCircuit cs;
    cs.N = 8; cs.nb_wires = nw; cs.nb_public = 3; cs.n_commitments = 2;
    cs.committed = lists; cs.n_committed = nco.get(); cs.commitment_wire = cw.get();
    std::unique_ptr<uint8_t[]> ia(new uint8_t[nw]()), ib(new uint8_t[nw]());
    ia[2] = ia[7] = 1;              // wires 2 and 7 own no point of A
    ib[0] = ib[7] = ib[11] = 1;
    KeyAuditWires w;
    keyaudit_wire_lists(cs, ia.get(), ib.get(), w);
    expect(w.cls == std::vector<uint8_t>({1, 1, 1, 0, 2, 2, 2, 0, 1, 1, 0, 0}), "wire classes");
    expect(w.a == std::vector<u32>({0, 1, 3, 4, 5, 6, 8, 9, 10, 11}), "slots of A");
    expect(w.b == std::vector<u32>({1, 2, 3, 4, 5, 6, 8, 9, 10}), "slots of B");
    expect(w.k == std::vector<u32>({3, 7, 10, 11}), "slots of K: a private wire in no constraint keeps its slot");
    expect(w.v == std::vector<u32>({0, 1, 2, 8, 9}), "slots of vk.K: public wires, then the commitment wires");
    expect(w.c.size() == 2 && w.c[0] == std::vector<u32>({4, 6}) && w.c[1] == std::vector<u32>({5}), "slots of the bases");
    KeyAuditCounts ok;
    ok.nb_wires = nw; ok.n_a = 10; ok.n_b = ok.n_g2_b = 9; ok.n_k = 4; ok.n_z = 8; ok.n_vk = 5; ok.n_basis = {2, 1}; ok.n_vk_ped = 2;
    expect(keyaudit_shape_refusal(cs, ok, w).empty(), "the circuit's own shape passes");
    struct { const char *count; void (*change)(KeyAuditCounts &); } bad[] = {
        {"claim.nb_wires", [](KeyAuditCounts &c) { c.nb_wires++; }}, {"claim.n_z", [](KeyAuditCounts &c) { c.n_z = 16; }},
        {"claim.n_a", [](KeyAuditCounts &c) { c.n_a--; }}, {"claim.n_b", [](KeyAuditCounts &c) { c.n_b++; }},
        {"claim.n_g2_b", [](KeyAuditCounts &c) { c.n_g2_b--; }}, {"claim.n_k", [](KeyAuditCounts &c) { c.n_k++; }},
        {"claim.vk.n_k", [](KeyAuditCounts &c) { c.n_vk--; }}, {"claim.n_ped", [](KeyAuditCounts &c) { c.n_basis.pop_back(); }},
        {"claim.vk.n_commitments", [](KeyAuditCounts &c) { c.n_vk_ped = 1; }}, {"claim.n_basis[1]", [](KeyAuditCounts &c) { c.n_basis[1] = 2; }}};
    for (const auto &b : bad) {
        KeyAuditCounts c = ok;
        b.change(c);
        expect(names(keyaudit_shape_refusal(cs, c, w), b.count), b.count);
    }
    // no commitments, one wire, N = 1
    KeyAuditCircuit one;
    one.N = 1; one.nb_wires = 1; one.nb_public = 1;
    std::unique_ptr<uint8_t[]> m(new uint8_t[1]());
    keyaudit_wire_lists(one, m.get(), m.get(), w);
    expect(w.cls.size() == 1 && w.k.empty() && w.v.size() == 1 && w.c.empty(), "one wire");
    // the permutation is an involution on every size, and the identity at log_n = 0
    expect(keyaudit_bitrev(0, 0) == 0, "bitrev at log_n 0");
    for (u32 log_n = 1; log_n <= 12; log_n++) {
        std::unique_ptr<uint8_t[]> seen(new uint8_t[(size_t)1 << log_n]());
        for (u64 i = 0; i < ((u64)1 << log_n); i++) {
            const u64 j = keyaudit_bitrev(i, log_n);
            expect(j < ((u64)1 << log_n) && keyaudit_bitrev(j, log_n) == i, "bitrev is an involution inside the domain");
            seen[j] = 1;
        }
        for (u64 i = 0; i < ((u64)1 << log_n); i++) expect(seen[i] == 1, "bitrev is onto");
    }
    expect(keyaudit_bitrev(1, 27) == (u64)1 << 26 && keyaudit_bitrev(6, 3) == 3, "bitrev values");
    // the class mask
    const Fr five = fe_from_u32<FrParams>(5);
    expect(keyaudit_masked(five, 2, 2) == five && keyaudit_masked(five, 1, 2).is_zero(), "class mask");
    // the point predicate: every rule over every input, both curves
    const Fp q = Fp::modulus();
    const G1Aff g1 = g1_generator(), inf1{Fp::zero(), Fp::zero()}, off1{Fp::one(), Fp::one()};
    const G1Aff in1[5] = {g1, inf1, off1, G1Aff{plus_modulus(g1.x), g1.y}, G1Aff{q, q}};
    point_matrix("G1", in1);
    expect(old_claim(g1) && old_claim(inf1) && !old_claim(off1) && !old_claim(in1[3]) && !old_claim(in1[4]), "G1: the claim rule is the audit's with infinity allowed");
    for (int k = 0; k < 5; k++) expect(point_ok(in1[k], POINT_RULE_CLAIM) == old_claim(in1[k]), "G1: a claimed point against the predicate it replaced");
    const G2Aff g2 = g2_generator(), inf2{Fp2::zero(), Fp2::zero()}, off2{g2.x, g2.x};
    const G2Aff in2[5] = {g2, inf2, off2, G2Aff{Fp2{plus_modulus(g2.x.a0), g2.x.a1}, g2.y}, G2Aff{Fp2{q, q}, Fp2{q, q}}};
    point_matrix("G2", in2);
    // the audit's own names for its rule
    expect(keyaudit_g1_ok(g1, false) && keyaudit_g1_ok(inf1, true) && !keyaudit_g1_ok(inf1, false) && !keyaudit_g1_ok(off1, true), "G1 point check");
    expect(keyaudit_g2_ok(g2, false) && keyaudit_g2_ok(inf2, true) && !keyaudit_g2_ok(inf2, false) && !keyaudit_g2_ok(off2, true), "G2 point check");
    if (fails) return 1;
    std::printf("keyaudit host: ok\n");
    return 0;
}

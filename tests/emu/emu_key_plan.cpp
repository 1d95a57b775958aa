// Host build of gnark-whir_amd/csrc/key_plan.h (the arithmetic of loading a proving key: window counts, the fixed-base table plan, the
// walk over the wire masks) behind a C interface for tests/test_key_plan_cpu.py.  g++ alone: the header has no HIP include.
#include <cstring>
#include "../../gnark-whir_amd/csrc/key_plan.h"

extern "C" {
uint32_t emu_msm_nwin(uint32_t c) { return msm_nwin(c); }
void emu_fixed_base_plan(const uint32_t knob[3], uint64_t budget_bytes, uint64_t n_ak, uint64_t n_b, uint64_t n_z, uint32_t c_out[3]) {
    const FixedBasePlan p = fixed_base_plan(knob, budget_bytes, n_ak, n_b, n_z);
    std::memcpy(c_out, p.c, sizeof(p.c));
}
// idx_a / idx_b / idx_k: room for w_hi - w_lo entries each; counts[9] = entries written to each, then n_a, n_b, n_k, a0, b0, k0
void emu_wire_indices(const uint8_t *infinity_a, const uint8_t *infinity_b, uint64_t nb_wires, uint64_t nb_public, const uint32_t *committed,
                      uint64_t n_committed, uint64_t w_lo, uint64_t w_hi, uint32_t *idx_a, uint32_t *idx_b, uint32_t *idx_k, uint64_t counts[9]) {
    const WireIndices x = wire_indices(infinity_a, infinity_b, nb_wires, nb_public, committed, n_committed, w_lo, w_hi);
    auto copy = [](uint32_t *dst, const std::vector<uint32_t> &v) { if (!v.empty()) std::memcpy(dst, v.data(), v.size() * 4); };
    copy(idx_a, x.a); copy(idx_b, x.b); copy(idx_k, x.k);
    const uint64_t c[9] = {x.a.size(), x.b.size(), x.k.size(), x.n_a, x.n_b, x.n_k, x.a0, x.b0, x.k0};
    std::memcpy(counts, c, sizeof(c));
}
}

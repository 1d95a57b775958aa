// The host arithmetic of loading a proving key (prove.hip, group.hip): window counts, the fixed-base table plan, the walk over the static
// wire masks.  Plain C++17 without a HIP include: tests/emu/emu_key_plan.cpp compiles it with g++.
#pragma once
#include <cstdint>
#include <vector>

constexpr uint32_t msm_nwin(uint32_t c) { return (256 + c - 1) / c; }   // windows of c bits that cover a 256-bit scalar

// Fixed-base window tables per group of MSMs that share a sort, in the order A+K, B1+B2, Z; 0 = none (the generic path).  Automatic
// widths 19 / 17 / 20, measured at N = 2^23 with proofs overlapping: +7 % proofs/s over the generic c = 16 path (13..15
// windows instead of 16); B went from 18 to 17 when the G2 additions got 18 % cheaper and the 2^17-bucket G2 reduce weighed more (30.2 vs
// 29.9 proofs/s); wider windows lose it again to the bucket reduce (2^(c-1) buckets, G2 first).
// knob (mi_debug_set_prove_fixed_base): 1 = never, 17..22 = that width whatever it costs, else automatic: a group gets tables when its
// MSM has >= 2^20 points and they fit what the groups chosen before it left of budget_bytes (smallest first: Z, B, A+K).  n_*: points
// of the group's MSMs; a point of A+K is two G1 points, one of B a G1 and a G2 point.
struct FixedBasePlan { uint32_t c[3]; };
inline FixedBasePlan fixed_base_plan(const uint32_t knob[3], uint64_t budget_bytes, uint64_t n_ak, uint64_t n_b, uint64_t n_z) {
    const struct { int group; uint32_t c_auto; uint64_t n, bytes_per_point; } order[3] = {{2, 20, n_z, 64}, {1, 17, n_b, 64 + 128}, {0, 19, n_ak, 2 * 64}};
    FixedBasePlan plan{};
    for (const auto &g : order) {
        const uint32_t k = knob[g.group];
        const uint64_t need = msm_nwin(g.c_auto) * g.n * g.bytes_per_point;
        if (k >= 17 && k <= 22) plan.c[g.group] = k;
        else if (k != 1 && g.n >= ((uint64_t)1 << 20) && need <= budget_bytes) { plan.c[g.group] = g.c_auto; budget_bytes -= need; }
    }
    return plan;
}

// Gather indices from the static masks (prove.go: the wireValuesA / B filters; K drops the public and the committed wires) for the
// wires [w_lo, w_hi) of a key, relative to w_lo.  n_*: points of the WHOLE key; a0 / b0 / k0: points of the wires before w_lo = where
// the range's points start in the whole key's arrays.  committed must be sorted.
struct WireIndices { std::vector<uint32_t> a, b, k; uint64_t n_a = 0, n_b = 0, n_k = 0, a0 = 0, b0 = 0, k0 = 0; };
inline WireIndices wire_indices(const uint8_t *infinity_a, const uint8_t *infinity_b, uint64_t nb_wires, uint64_t nb_public,
                                const uint32_t *committed, uint64_t n_committed, uint64_t w_lo, uint64_t w_hi) {
    WireIndices x;
    uint64_t ci = 0;
    for (uint64_t j = 0; j < nb_wires; j++) {
        const bool in = j >= w_lo && j < w_hi;
        if (j == w_lo) { x.a0 = x.n_a; x.b0 = x.n_b; x.k0 = x.n_k; }
        if (!infinity_a[j]) { x.n_a++; if (in) x.a.push_back((uint32_t)(j - w_lo)); }
        if (!infinity_b[j]) { x.n_b++; if (in) x.b.push_back((uint32_t)(j - w_lo)); }
        if (j < nb_public) continue;
        while (ci < n_committed && committed[ci] < j) ci++;
        if (ci < n_committed && committed[ci] == j) continue;
        x.n_k++;
        if (in) x.k.push_back((uint32_t)(j - w_lo));
    }
    if (w_lo >= nb_wires) { x.a0 = x.n_a; x.b0 = x.n_b; x.k0 = x.n_k; }
    return x;
}

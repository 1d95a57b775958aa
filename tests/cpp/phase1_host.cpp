// Stand-alone host run of the per-lane text of the phase-1 kernels (gnark-whir_amd/csrc/scale_powers.cuh: the scalar's recoding into
// signed fixed-window digits, the per-lane table and the ladder -- MI_HD, the text phase1.hip's kernels run) and of the contribution
// records (csrc/phase1_ops.cuh, csrc/phase1_records.hip: mi_phase1_records_verify, no HIP call): built with -fsanitize=address,undefined
// by `make sanitize-phase1`, run by tests/test_phase1_host.py.  The program judges for itself: it prints one line per group of checks,
// "FAIL ..." for the first failure of a group, and exits 1 if anything failed.
//
//   recode   for W = 2..5 and every scalar of the set: the digits popped from the top are in [-2^(W-1), 2^(W-1)] and
//            sum_j d_j 2^(W j) is the scalar as a big integer
//   ladder   for W = 2..5, G1 and G2: the lane's table and ladder against xyzz_mul_256 after xyzz_to_affine, over the same scalars, the
//            points taken in turn from a handful (infinity included); the table is lane-interleaved with a stride above 1
//   chain    three honest records verify; every single tamper is rejected at the record it touches
// The scalars: 0, 1, 2, r - 1, r - 2, 2^j and 2^j - 1 for j <= 253, 2^254 - 1 (every window all ones: a carry through every digit, and
// the last carry lands in the digit above the scalar's own bits), 200 random scalars below r.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include "../../include/mi355x_groth16_phase1.h"
#include "../../gnark-whir_amd/csrc/fp12.cuh"
#include "../../gnark-whir_amd/csrc/scale_powers.cuh"
#include "../../gnark-whir_amd/csrc/phase1_ops.cuh"

namespace {

struct U256 { u32 l[8]; };
int failures = 0;
void fail(const char *what, int w, size_t i) { std::printf("FAIL %s W=%d scalar #%zu\n", what, w, i); failures++; }

U256 u256_pow2(int j, bool minus_one) {
    U256 x{};
    x.l[j >> 5] = 1u << (j & 31);
    if (minus_one) {   // 2^j - 1: every bit below j
        x = U256{};
        for (int b = 0; b < j; b++) x.l[b >> 5] |= 1u << (b & 31);
    }
    return x;
}
u64 rng_state = 0x9e3779b97f4a7c15ull;
u32 rng32() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (u32)(rng_state >> 16);
}
std::vector<U256> scalar_set() {
    std::vector<U256> s;
    U256 z{}, one{}, two{}, rm1{}, rm2{};
    one.l[0] = 1; two.l[0] = 2;
    for (int i = 0; i < 8; i++) rm1.l[i] = rm2.l[i] = FrParams::p[i];
    rm1.l[0] -= 1; rm2.l[0] -= 2;
    s.insert(s.end(), {z, one, two, rm1, rm2});
    for (int j = 0; j <= 253; j++) { s.push_back(u256_pow2(j, false)); s.push_back(u256_pow2(j, true)); }
    s.push_back(u256_pow2(254, true));
    for (int n = 0; n < 200; n++) {
        Fr x;
        for (int i = 0; i < 8; i++) x.l[i] = rng32();
        x.l[7] &= 0x1fffffffu;   // below 2^253 < r
        U256 u;
        std::memcpy(u.l, x.l, 32);
        s.push_back(u);
    }
    return s;
}

// acc <- acc 2^W + d over 9 words; the running value of digits taken from the top is never negative
bool push_digit(u32 acc[9], int W, int d) {
    for (int i = 8; i > 0; i--) acc[i] = (acc[i] << W) | (acc[i - 1] >> (32 - W));
    acc[0] <<= W;
    long long carry = d;
    for (int i = 0; i < 9; i++) {
        carry += acc[i];
        acc[i] = (u32)carry;
        carry >>= 32;   // arithmetic: a borrow goes on as -1
    }
    return carry == 0;
}
template <int W>
void check_recode(const std::vector<U256> &set) {
    size_t bad = 0;
    for (size_t n = 0; n < set.size(); n++) {
        u32 e[8], acc[9] = {0};
        scale_powers_recode<W>(set[n].l, e);
        bool ok = true;
        for (int j = 0; j < ScalePowers<W>::digits; j++) {
            const int d = scale_powers_next_digit<W>(e);
            ok = ok && d >= -(1 << (W - 1)) && d <= (1 << (W - 1)) && push_digit(acc, W, d);
        }
        ok = ok && acc[8] == 0 && std::memcmp(acc, set[n].l, 32) == 0;
        if (!ok && !bad++) fail("recode", W, n);
    }
    std::printf("recode W=%d digits=%d scalars=%zu bad=%zu\n", W, ScalePowers<W>::digits, set.size(), bad);
}

template <class F> struct Gen;
template <> struct Gen<Fp> { static Affine<Fp> g() { return g1_generator(); } static const char *name() { return "G1"; } };
template <> struct Gen<Fp2> { static Affine<Fp2> g() { return g2_generator(); } static const char *name() { return "G2"; } };

template <class F>
std::vector<Affine<F>> point_set() {
    const XYZZ<F> g = XYZZ<F>::from_affine(Gen<F>::g());
    std::vector<Affine<F>> p;
    p.push_back(Gen<F>::g());
    p.push_back(xyzz_to_affine(xyzz_mul_u32(g, 5)));
    p.push_back(Affine<F>{F::zero(), F::zero()});
    p.push_back(xyzz_to_affine(xyzz_neg(xyzz_mul_u32(g, 0x7fffffffu))));
    p.push_back(xyzz_to_affine(xyzz_mul_u32(g, 2)));
    return p;
}
template <class F>
bool same(const Affine<F> &a, const Affine<F> &b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

template <class F, int W>
void check_ladder(const std::vector<U256> &set, const std::vector<Affine<F>> &pts, const std::vector<Affine<F>> &want) {
    constexpr u64 STRIDE = 3;   // the lane's entries lie STRIDE points apart, as in a chunk of three lanes; this lane is the middle one
    std::vector<std::unique_ptr<XYZZ<F>[]>> tabs;
    for (const auto &p : pts) {
        tabs.emplace_back(new XYZZ<F>[STRIDE * ScalePowers<W>::entries]);   // exactly the table's size: a step past it is a heap overflow
        scale_powers_table_lane<F, W>(tabs.back().get() + 1, STRIDE, p);
    }
    size_t bad = 0;
    for (size_t n = 0; n < set.size(); n++) {
        const size_t which = n % pts.size();
        const Affine<F> got = xyzz_to_affine(scale_powers_ladder_lane<F, W>(tabs[which].get() + 1, STRIDE, set[n].l));
        if (!same(got, want[n]) && !bad++) fail(Gen<F>::name(), W, n);
    }
    std::printf("ladder %s W=%d scalars=%zu bad=%zu\n", Gen<F>::name(), W, set.size(), bad);
}
template <class F>
void check_ladders(const std::vector<U256> &set) {
    const std::vector<Affine<F>> pts = point_set<F>();
    std::vector<Affine<F>> want;
    for (size_t n = 0; n < set.size(); n++) want.push_back(xyzz_to_affine(xyzz_mul_256(XYZZ<F>::from_affine(pts[n % pts.size()]), set[n].l)));
    size_t inf = 0;
    for (const auto &w : want) inf += w.is_inf();
    std::printf("reference %s points=%zu at_infinity=%zu\n", Gen<F>::name(), want.size(), inf);
    check_ladder<F, 2>(set, pts, want);
    check_ladder<F, 3>(set, pts, want);
    check_ladder<F, 4>(set, pts, want);
    check_ladder<F, 5>(set, pts, want);
}

// ---------------------------------------------------------------------------------------------------- the records
G1Aff g1_times(const Fr &e) { return xyzz_to_affine(xyzz_scale(G1X::from_affine(g1_generator()), e)); }
Fr fr_small(u32 v) { return fe_from_u32<FrParams>(v); }

struct Chain {
    static constexpr size_t M = 3;
    mi_g1_affine start[3];
    uint8_t start_hash[32];
    uint64_t first_index = 5;
    std::unique_ptr<mi_phase1_record[]> rec{new mi_phase1_record[M]};   // a heap block of exactly M records
};
void make_chain(Chain &c) {
    for (int i = 0; i < 32; i++) c.start_hash[i] = (uint8_t)(7 * i + 1);
    Fr e[3] = {fr_small(11), fr_small(13), fr_small(17)};
    G1Aff before[3];
    for (int x = 0; x < 3; x++) before[x] = g1_times(e[x]);
    std::memcpy(c.start, before, sizeof(before));
    uint8_t prev[32];
    std::memcpy(prev, c.start_hash, 32);
    Fr full;   // a full-width value
    for (int i = 0; i < 8; i++) full.l[i] = FrParams::r2[i];
    for (size_t i = 0; i < Chain::M; i++) {
        Fr d[3] = {full * fr_small(3 + (u32)i), fr_small(3 + (u32)i), fe_neg(fr_small(2 + (u32)i))};
        Fr k[3] = {fe_neg(Fr::one()), full * fr_small(101 + (u32)i), fr_small(9 + (u32)i)};
        G1Aff after[3];
        for (int x = 0; x < 3; x++) { e[x] = e[x] * d[x]; after[x] = g1_times(e[x]); }
        Phase1Record r;
        phase1_record_make(prev, c.first_index + i, before, after, d, k, &r);
        std::memcpy(&c.rec[i], &r, sizeof(r));
        std::memcpy(before, after, sizeof(after));
        std::memcpy(prev, r.hash, 32);
    }
}
void expect(const char *what, size_t at, const Chain &c, uint64_t want_bad, int32_t want_rc = MI_OK) {
    uint64_t fb = ~(uint64_t)0;
    const int32_t rc = mi_phase1_records_verify(c.start, c.start_hash, c.first_index, c.rec.get(), Chain::M, &fb);
    if (rc != want_rc || (rc == MI_OK && fb != want_bad)) {
        std::printf("FAIL chain %s at %zu: rc %d first_bad %llu, expected rc %d first_bad %llu\n", what, at, rc, (unsigned long long)fb, want_rc, (unsigned long long)want_bad);
        failures++;
    }
}
void check_chain() {
    Chain good;
    make_chain(good);
    expect("honest", 0, good, Chain::M);
    auto copy = [&](Chain &c) {
        std::memcpy(c.start, good.start, sizeof(c.start));
        std::memcpy(c.start_hash, good.start_hash, 32);
        c.first_index = good.first_index;
        std::memcpy(c.rec.get(), good.rec.get(), Chain::M * sizeof(mi_phase1_record));
    };
    size_t cases = 1;
    // one flipped bit in each field of each record: three points after, three commitments, three responses, the hash
    const size_t field_at[10] = {0, 64, 128, 192, 256, 320, 384, 416, 448, 480};
    for (size_t i = 0; i < Chain::M; i++)
        for (size_t f = 0; f < 10; f++) {
            Chain c; copy(c);
            ((uint8_t *)&c.rec[i])[field_at[f] + 5] ^= 0x04;
            expect("bit flip in field", 10 * i + f, c, i); cases++;
        }
    { Chain c; copy(c); c.first_index++; expect("first_index", 0, c, 0); cases++; }
    { Chain c; copy(c); c.start_hash[31] ^= 1; expect("start_hash", 0, c, 0); cases++; }
    { Chain c; copy(c); std::swap(c.rec[0], c.rec[1]); expect("swap", 0, c, 0); cases++; }
    { Chain c; copy(c); std::swap(c.rec[1], c.rec[2]); expect("swap", 1, c, 1); cases++; }
    for (size_t i = 0; i < Chain::M; i++) {
        { Chain c; copy(c); Fp y; std::memcpy(&y, &c.rec[i].alpha1.y, 32); y = y + Fp::one(); std::memcpy(&c.rec[i].alpha1.y, &y, 32); expect("off the curve", i, c, i); cases++; }
        { Chain c; copy(c); std::memset(&c.rec[i].commit[2], 0, 64); expect("commitment at infinity", i, c, i); cases++; }
        { Chain c; copy(c); std::memset(&c.rec[i].tau1, 0, 64); expect("point at infinity", i, c, i); cases++; }
        {   // the response's words plus r: the same residue, not below r
            Chain c; copy(c);
            Fr z, sum;
            std::memcpy(&z, &c.rec[i].response[1], 32);
            fe_add_raw(sum, z, Fr::modulus());
            std::memcpy(&c.rec[i].response[1], &sum, 32);
            expect("response + r", i, c, i); cases++;
        }
    }
    {   // a chain in two pieces: the second continues where the first ended
        uint64_t fb = 0;
        const int32_t rc = mi_phase1_records_verify(&good.rec[0].tau1, good.rec[0].hash, good.first_index + 1, good.rec.get() + 1, Chain::M - 1, &fb);
        if (rc != MI_OK || fb != Chain::M - 1) { std::printf("FAIL chain continued: rc %d first_bad %llu\n", rc, (unsigned long long)fb); failures++; }
        cases++;
    }
    {   // null arguments and a start that is no point: MI_EINVAL, nothing written
        uint64_t fb = 77;
        int bad = 0;
        bad += mi_phase1_records_verify(nullptr, good.start_hash, 0, good.rec.get(), Chain::M, &fb) != MI_EINVAL;
        bad += mi_phase1_records_verify(good.start, nullptr, 0, good.rec.get(), Chain::M, &fb) != MI_EINVAL;
        bad += mi_phase1_records_verify(good.start, good.start_hash, 0, nullptr, Chain::M, &fb) != MI_EINVAL;
        bad += mi_phase1_records_verify(good.start, good.start_hash, 0, good.rec.get(), Chain::M, nullptr) != MI_EINVAL;
        mi_g1_affine s[3];
        std::memcpy(s, good.start, sizeof(s));
        std::memset(&s[1], 0, 64);
        bad += mi_phase1_records_verify(s, good.start_hash, 0, good.rec.get(), Chain::M, &fb) != MI_EINVAL;
        bad += mi_phase1_records_verify(good.start, good.start_hash, 0, nullptr, 0, &fb) != MI_OK || fb != 0;   // no record: all of none hold
        if (bad) { std::printf("FAIL chain null arguments: %d\n", bad); failures++; }
        cases++;
    }
    std::printf("chain cases=%zu\n", cases);
}

}  // namespace

int main() {
    const std::vector<U256> set = scalar_set();
    check_recode<2>(set);
    check_recode<3>(set);
    check_recode<4>(set);
    check_recode<5>(set);
    check_ladders<Fp>(set);
    check_ladders<Fp2>(set);
    check_chain();
    std::printf("failures=%d\n", failures);
    return failures ? 1 : 0;
}

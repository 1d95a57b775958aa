// Stand-alone sanitizer run of kSum over a window table (gnark-whir_amd/csrc/ksum_ops.cuh): built with -fsanitize=address,undefined
// -DMI_CHECK_NOWRAP by `make sanitize-ksum`, run by tests/test_ksum_cpu.py.  The table is a heap block of exactly ksum_table_bytes, the
// rows and multiples of the build, the scalars, the partial sums and the sums are heap blocks of exactly the sizes csrc/ksum.hip
// computes for them, so one record read or written too far is a report.  For every width c in {8, 4, 2}, keys of 1, 2 and 3 bases (one
// of them at infinity, two of them equal) and batches of 1, 3 and 34 rows under the slices ksum_slices chooses and under 1, 7 and 48
// forced ones, every sum is compared with double-and-add over the bases themselves.  Prints the number of batches checked.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <utility>
#include "../../gnark-whir_amd/csrc/ksum_ops.cuh"

namespace {
unsigned checked = 0;
void require(bool ok, const char *what, unsigned ns, unsigned c, size_t n, unsigned slices) {
    if (ok) return;
    std::printf("FAILED: %s (ns %u, c %u, n %zu, slices %u)\n", what, ns, c, n, slices);
    std::exit(1);
}
uint64_t state = 0x9E3779B97F4A7C15ull;
u32 next32() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (u32)(state >> 32); }
// a Montgomery scalar: of four kinds by turn -- zero, a byte, full width (top word below r's), only the top window of c = 8
Fr scalar(unsigned kind) {
    Fr x = Fr::zero();
    if (kind % 4 == 1) x.l[0] = next32() & 255;
    if (kind % 4 == 2) { for (auto &w : x.l) w = next32(); x.l[7] &= 0x0fffffffu; }
    if (kind % 4 == 3) x.l[7] = 0x2f000000u;
    return fe_to_mont(x);
}
G1Aff multiple_of_generator(u32 k) {
    u32 kk[8] = {k, 0, 0, 0, 0, 0, 0, 0};
    return xyzz_to_affine(xyzz_mul_256(G1X::from_affine(G1Aff{Fp::one(), Fp::one() + Fp::one()}), kk));
}

struct Key { std::unique_ptr<G1Aff[]> k, table; };
// the bases and their table, built once per (ns, c) by the build's own lanes
Key build(unsigned ns, unsigned c) {
    const u32 windows = ksum_windows(c), entries = (u32)ksum_row_entries(c);
    const size_t n = 0;
    const unsigned forced = 0;
    std::unique_ptr<G1Aff[]> k(new G1Aff[ns]);
    for (unsigned j = 0; j < ns; j++) k[j] = multiple_of_generator(5 + 3 * j);
    if (ns > 1) k[1] = k[0];                                   // equal bases: the doubling branch of the row's sum
    if (ns > 2) k[2] = G1Aff{Fp::zero(), Fp::zero()};          // a base at infinity: a row of infinities
    // ---- the build
    require(ksum_table_bytes(ns, c) == (uint64_t)ns * windows * entries * sizeof(G1Aff), "table bytes", ns, c, n, forced);
    std::unique_ptr<G1Aff[]> table(new G1Aff[(size_t)ns * windows * entries]);
    std::unique_ptr<G1X[]> rows(new G1X[(size_t)ns * windows]), mult(new G1X[entries]);
    for (unsigned j = 0; j < ns; j++) ksum_rows_lane(k[j], c, windows, rows.get() + (size_t)j * windows);
    for (size_t rw = 0; rw < (size_t)ns * windows; rw++) {
        ksum_multiples_lane(rows[rw], entries, mult.get());
        for (u32 d = 0; d < entries; d++) table[rw * entries + d] = xyzz_to_affine(mult[d]);
    }
    return Key{std::move(k), std::move(table)};
}

// ---- the sums of a batch
void run(const Key &key, unsigned ns, unsigned c, size_t n, unsigned forced) {
    const u32 windows = ksum_windows(c);
    const G1Aff *k = key.k.get(), *table = key.table.get();
    const u32 S = forced ? forced : ksum_slices(ns, c, n), R = ksum_reduce_lanes(S);
    const uint64_t terms = (uint64_t)ns * windows, L = ksum_slice_terms(ns, c, S);
    require(S >= 1 && R >= 1 && R <= 64 && (R & (R - 1)) == 0 && (uint64_t)S * L >= terms, "the cut of a row", ns, c, n, forced);
    std::unique_ptr<Fr[]> scal(new Fr[n * ns]);
    std::unique_ptr<uint8_t[]> skip(new uint8_t[n]);
    for (size_t t = 0; t < n * ns; t++) scal[t] = scalar((unsigned)(t + t / ns));
    for (size_t i = 0; i < n; i++) skip[i] = i % 5 == 4;
    std::unique_ptr<G1X[]> part(new G1X[n * S]), sums(new G1X[n]), lanes(new G1X[R]);
    for (size_t t = 0; t < n * S; t++) {
        const size_t i = t / S, s = t - i * S;
        if (skip[i]) continue;                                 // neither read nor written: the block stays uninitialised
        const uint64_t t0 = s * L, t1 = t0 + L < terms ? t0 + L : terms;
        part[t] = t0 < terms ? ksum_lane(table, scal.get() + i * ns, c, t0, t1) : G1X::inf();
    }
    for (size_t i = 0; i < n; i++) {
        for (u32 sub = 0; sub < R; sub++) lanes[sub] = skip[i] ? G1X::inf() : ksum_strided_sum(part.get() + i * S, S, sub, R);
        for (u32 h = R >> 1; h; h >>= 1)
            for (u32 sub = 0; sub < h; sub++) xyzz_add(lanes[sub], lanes[sub + h]);
        sums[i] = lanes[0];
    }
    // ---- against double-and-add over the bases
    for (size_t i = 0; i < n; i++) {
        G1X want = G1X::inf();
        for (unsigned j = 0; j < ns && !skip[i]; j++) xyzz_add(want, xyzz_mul_256(G1X::from_affine(k[j]), fe_from_mont(scal[i * ns + j]).l));
        const G1Aff a = xyzz_to_affine(sums[i]), b = xyzz_to_affine(want);
        require(a.x == b.x && a.y == b.y, "a row's sum", ns, c, n, forced);
    }
    checked++;
}
}   // namespace

int main() {
    for (unsigned c : {8u, 4u, 2u})
        for (unsigned ns : {1u, 2u, 3u}) {
            const Key key = build(ns, c);
            for (size_t n : {(size_t)1, (size_t)3, (size_t)34})
                for (unsigned forced : {0u, 1u, 7u, 48u}) {
                    if (n == 34 && forced == 0 && c != 8) continue;   // 34 rows of 1024 slices in this build take long: once is enough
                    run(key, ns, c, n, forced);
                }
        }
    std::printf("%u\n", checked);
    return 0;
}

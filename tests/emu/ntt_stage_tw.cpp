// Stand-alone host driver for NttPass::tw_stage (stage twiddles by global index, gnark-whir_amd/csrc/ntt_tile.cuh): the records of
// ntt_build_transform run through ntt_tile_load / ntt_tile_stage / ntt_tile_store with the stage-twiddle tables bound, against the
// same records with the null pointer (tile-local twiddles + the product at the pass's edge) and, at the smallest size, against a
// direct O(N^2) evaluation.  Built with -DMI_CHECK_NOWRAP: every bound of the lazy arithmetic traps.  tests/test_ntt_stage_twiddles_cpu.py
// builds and runs it; exit status 0 and a last line "ok" mean every case held.
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <vector>
#include "../../gnark-whir_amd/csrc/ntt_tile.cuh"

static Fr fr_pow_u64(Fr b, u64 e) { Fr acc = Fr::one(); while (e) { if (e & 1) acc = acc * b; b = fe_sqr(b); e >>= 1; } return acc; }
static Fr fr_from_u64x4(u64 a, u64 b, u64 c, u64 d) {
    Fr t; t.l[0] = (u32)a; t.l[1] = (u32)(a >> 32); t.l[2] = (u32)b; t.l[3] = (u32)(b >> 32);
    t.l[4] = (u32)c; t.l[5] = (u32)(c >> 32); t.l[6] = (u32)d; t.l[7] = (u32)(d >> 32);
    return fe_to_mont(t);
}
static bool fr_same(const Fr &x, const Fr &y) { for (int i = 0; i < 8; i++) if (x.l[i] != y.l[i]) return false; return true; }
static bool fr_below(const Fr &x, const Fr &bound) { Fr d; return fe_sub_raw(d, x, bound) != 0; }   // as 256-bit integers
static Fr fr_root_2p28() { return fr_from_u64x4(0x9bd61b6e725b19f0ull, 0x402d111e41112ed4ull, 0x00e0a7eb8ef62abcull, 0x2a3c09f0a58a7e85ull); }
static u64 rng_state = 0x243f6a8885a308d3ull;
static u64 rng() { u64 z = (rng_state += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
static Fr fr_random() { return fr_from_u64x4(rng(), rng(), rng(), rng() >> 3); }   // below 2^253 < p, to Montgomery form

// the tables of one transform as ntt.hip binds them (emu.cpp builds the same seven), plus the stage twiddles of every strided pass
struct Bound {
    std::vector<Fr> small, twlo, twhi, sclo, schi, nv;
    std::vector<std::vector<Fr>> stage;
    NttTables t;
    Fr w, g, ninv;
};
static void build_tables(Bound &b, u32 log_n, u32 flags) {
    const bool inverse = flags & NTT_INVERSE, coset = flags & NTT_COSET;
    const Fr root = fr_root_2p28();
    Fr w4096 = root; for (int k = 12; k < 28; k++) w4096 = fe_sqr(w4096);
    Fr w = root; for (u32 k = log_n; k < 28; k++) w = fe_sqr(w);
    if (inverse) { w = fe_inv(w); w4096 = fe_inv(w4096); }
    Fr g = fe_from_u32<FrParams>(5); if (inverse) g = fe_inv(g);
    Fr nn = Fr::zero(); nn.l[0] = 1u << log_n; const Fr ninv = fe_inv(fe_to_mont(nn));
    const u32 h = (log_n + 1) / 2, nlo = 1u << h, nhi = 1u << (log_n - h);
    b.small.resize(2048); b.twlo.resize(nlo); b.twhi.resize(nhi); b.sclo.resize(nlo); b.schi.resize(nhi);
    for (u32 j = 0; j < 2048; j++) b.small[j] = j ? b.small[j - 1] * w4096 : Fr::one();
    for (u32 j = 0; j < nlo; j++) { b.twlo[j] = fr_pow_u64(w, j); b.sclo[j] = fr_pow_u64(g, j); }
    for (u32 j = 0; j < nhi; j++) { b.twhi[j] = fr_pow_u64(w, (u64)j << h); b.schi[j] = fr_pow_u64(g, (u64)j << h); if (inverse) b.schi[j] = b.schi[j] * ninv; }
    b.t = NttTables{b.small.data(), b.twlo.data(), b.twhi.data(), b.sclo.data(), b.schi.data(), nullptr, h};
    b.nv.assign(1, ninv);
    if (inverse && !coset) { b.t.sc_lo = b.nv.data(); b.t.sc_hi = b.nv.data(); }
    b.w = w; b.g = g; b.ninv = ninv;
}
// bind == true: every strided pass gets its stage-twiddle table (powers of w_N taken one by one: no shared code with the stages)
static void bind_stage_tables(Bound &b, NttTransform &tr, bool bind) {
    b.stage.clear();
    b.stage.resize(tr.n_pass);
    for (u32 i = 0; i < tr.n_pass; i++) {
        NttPass &p = tr.pass[i];
        p.tw_stage = nullptr;
        if (!bind || !p.twiddle) continue;
        const u32 R = 1u << p.log_r, S = 1u << p.log_s;
        b.stage[i].assign((size_t)R * S, Fr::zero());
        for (u32 lo = 0; lo < S; lo++)
            for (u32 d = 1; d < R; d <<= 1)
                for (u32 j = 0; j < d; j++) {
                    const u64 e = ((u64)j * S + lo) * ((u64)1 << tr.log_n) / (2ull * d * S);   // w_(2dS)^(j S + lo) as a power of w_N
                    const u32 idx = lo * R + d + j;
                    if (ntt_stage_tw_exponent(tr.log_n, p.log_r, p.log_s, idx) != e) { std::printf("FAIL exponent of entry %u\n", idx); std::exit(1); }
                    b.stage[i][idx] = fr_pow_u64(b.w, e);
                }
        p.tw_stage = b.stage[i].data();
    }
}
// what the kernels do, one thread after the other; after_pass(step) sees the array as the pass stored it
template <class F>
static void run_passes(const NttTransform &tr, const NttTables &t, Fr *data, u32 nthr, F after_pass) {
    for (u32 step = 0; step < tr.n_pass; step++) {
        const NttPass &p = tr.pass[step];
        const u32 tiles = 1u << (tr.log_n - p.log_r - p.log_c);
        std::vector<U4> lds((size_t)2 * ntt_plane_slots(p));
        for (u32 tile = 0; tile < tiles; tile++) {
            for (u32 tid = 0; tid < nthr; tid++) ntt_tile_load(p, t, data, tile, tid, nthr, lds.data());
            for (u32 s = 0; s < p.log_r; s++)
                for (u32 tid = 0; tid < nthr; tid++) ntt_tile_stage(p, t, s, tid, nthr, lds.data(), tile);
            for (u32 tid = 0; tid < nthr; tid++) ntt_tile_store(p, t, data, tile, tid, nthr, lds.data());
        }
        after_pass(step);
    }
}
static u32 bitrev(u32 x, u32 bits) { u32 r = 0; for (u32 k = 0; k < bits; k++) { r = (r << 1) | (x & 1); x >>= 1; } return r; }
// fft.Domain's transform by its definition: N^2 products
static std::vector<Fr> direct(const std::vector<Fr> &in, u32 log_n, u32 flags, u32 n_valid, const Bound &b) {
    const bool inverse = flags & NTT_INVERSE, coset = flags & NTT_COSET, dit = flags & NTT_DIT;
    const u32 n = 1u << log_n;
    std::vector<Fr> x(n), out(n), wp(n);
    for (u32 i = 0; i < n; i++) { const Fr v = i < n_valid ? in[i] : Fr::zero(); x[dit ? bitrev(i, log_n) : i] = v; }
    wp[0] = Fr::one();
    for (u32 i = 1; i < n; i++) wp[i] = wp[i - 1] * b.w;
    if (coset && !inverse) { Fr gp = Fr::one(); for (u32 i = 0; i < n; i++) { x[i] = x[i] * gp; gp = gp * b.g; } }
    Fr gk = Fr::one();
    for (u32 k = 0; k < n; k++) {
        Fr acc = Fr::zero();
        for (u32 i = 0; i < n; i++) acc = acc + x[i] * wp[(u32)(((u64)i * k) & (n - 1))];
        if (inverse) acc = acc * b.ninv;
        if (inverse && coset) { acc = acc * gk; gk = gk * b.g; }
        out[dit ? k : bitrev(k, log_n)] = acc;
    }
    return out;
}

int main() {
    int failures = 0;
    u32 cases = 0;
    const NttKnobs plans[2] = {NttKnobs{5, 4, 3}, NttKnobs{6, 5, 4}};
    // every size, plan and mode: bound against null, element by element; at 2^8 both against the definition
    for (u32 log_n = 8; log_n <= 13; log_n++)
        for (const NttKnobs &kn : plans)
            for (u32 flags = 0; flags < 8; flags++) {
                const u32 n = 1u << log_n, n_valid = n - 37, nthr = 64;
                Bound b;
                build_tables(b, log_n, flags);
                std::vector<Fr> in(n);
                for (Fr &v : in) v = fr_random();
                NttTransform tr = ntt_build_transform(log_n, flags, NTT_PLAIN, kn, false, n_valid);
                u32 strided = 0;
                for (u32 i = 0; i < tr.n_pass; i++) strided += tr.pass[i].twiddle;
                std::vector<Fr> plain = in, staged = in;
                bind_stage_tables(b, tr, false);
                run_passes(tr, b.t, plain.data(), nthr, [](u32) {});
                bind_stage_tables(b, tr, true);
                run_passes(tr, b.t, staged.data(), nthr, [](u32) {});
                u32 bad = 0;
                for (u32 i = 0; i < n; i++) bad += !fr_same(plain[i], staged[i]);
                if (log_n == 8) {
                    const std::vector<Fr> want = direct(in, log_n, flags, n_valid, b);
                    for (u32 i = 0; i < n; i++) bad += !fr_same(want[i], staged[i]) + !fr_same(want[i], plain[i]);
                }
                if (bad || !strided) { std::printf("FAIL log_n=%u plan=(%u,%u,%u) flags=%u strided=%u mismatches=%u\n", log_n, kn.log_e, kn.max_contig, kn.max_strided, flags, strided, bad); failures++; }
                std::printf("case log_n=%u plan=(%u,%u,%u) flags=%u passes=%u strided=%u\n", log_n, kn.log_e, kn.max_contig, kn.max_strided, flags, tr.n_pass, strided);
                cases++;
            }
    // the lazy contract without the edge product: a DIF pass fed 2p - 1 everywhere stores below 2p, a DIT pass fed 4p - 1 everywhere
    // stores below 4p (transforms that neither scale nor canonicalise, as computeH's inner ones), and the residues are the null path's
    const Fr two_p = fe_twice_modulus<FrParams>();
    Fr four_p; fe_add_raw(four_p, two_p, two_p);
    for (u32 dit = 0; dit < 2; dit++)
        for (u32 log_n : {10u, 13u})
            for (const NttKnobs &kn : plans) {
                const u32 n = 1u << log_n, flags = dit ? (u32)NTT_DIT : (u32)NTT_INVERSE;
                const Fr bound = dit ? four_p : two_p;
                Fr top = bound; top.l[0] -= 1;   // (2p and 4p are even and their low limb is not zero)
                Bound b;
                build_tables(b, log_n, flags);
                NttTransform tr = ntt_build_transform(log_n, flags, NTT_INV_UNSCALED, kn, false, n);
                std::vector<Fr> plain(n, top), staged(n, top);
                bind_stage_tables(b, tr, false);
                run_passes(tr, b.t, plain.data(), 64, [](u32) {});
                bind_stage_tables(b, tr, true);
                u32 outside = 0, bad = 0;
                run_passes(tr, b.t, staged.data(), 64, [&](u32) { for (const Fr &v : staged) outside += !fr_below(v, bound); });
                for (u32 i = 0; i < n; i++) bad += !fr_same(fe_canon(plain[i]), fe_canon(staged[i]));
                if (outside || bad) { std::printf("FAIL lazy dit=%u log_n=%u plan=(%u,%u,%u) outside=%u mismatches=%u\n", dit, log_n, kn.log_e, kn.max_contig, kn.max_strided, outside, bad); failures++; }
                std::printf("case lazy dit=%u log_n=%u plan=(%u,%u,%u) passes=%u\n", dit, log_n, kn.log_e, kn.max_contig, kn.max_strided, tr.n_pass);
                cases++;
            }
    std::printf("cases=%u failures=%d\n", cases, failures);
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}

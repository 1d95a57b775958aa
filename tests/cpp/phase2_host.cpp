// Stand-alone host run of the per-lane text of the phase-2 kernels (gnark-whir_amd/csrc/point_ntt.cuh: the butterfly and the stage of
// the inverse NTT over points; csrc/sparse_points.cuh: the term of a sparse sum of points and the run over a column), G1 and G2: built
// with -fsanitize=address,undefined by `make sanitize-phase2`, run by tests/test_phase2_host.py, which holds the cases and compares what
// this prints with oracle/pyref.py.  Every array is a heap block of exactly the size the text may touch.
//
// Commands on stdin, one per line; every number is a plain integer in hex (scalars below r):
//     ntt  <1|2> <log_n> <tau>                          P_k = tau^k g, k < N; the transform; prints [L_i], i = 0 .. N - 1 (natural order)
//     bfly <1|2> <ea> <eb> <k_top> <k_bot>              a = ea g, b = eb g (0 = infinity); one butterfly; prints the two results
//     col  <1|2> <log_n> <tau> <n> (<row> <coeff>) x n  the basis as ntt leaves it (bit-reversed, affine); the run over the n entries of
//                                                       one column; prints the sum
// A point prints as its affine coordinates in hex (G2: x.a0 x.a1 y.a0 y.a1), or "inf".
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>
#include "../../gnark-whir_amd/csrc/fp12.cuh"
#include "../../gnark-whir_amd/csrc/sparse_points.cuh"

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
void print_fp(const Fp &x) {
    const Fp c = fe_from_mont(x);
    for (int i = 7; i >= 0; i--) std::printf("%08x", c.l[i]);
}
void print_point(const G1Aff &p) {
    if (p.is_inf()) { std::printf("inf\n"); return; }
    print_fp(p.x); std::printf(" "); print_fp(p.y); std::printf("\n");
}
void print_point(const G2Aff &p) {
    if (p.is_inf()) { std::printf("inf\n"); return; }
    print_fp(p.x.a0); std::printf(" "); print_fp(p.x.a1); std::printf(" "); print_fp(p.y.a0); std::printf(" "); print_fp(p.y.a1); std::printf("\n");
}
template <class F> Affine<F> generator();
template <> G1Aff generator<Fp>() { return G1Aff{Fp::one(), fe_from_u32<FpParams>(2)}; }
template <> G2Aff generator<Fp2>() { return G2Aff{fp12c_g2gen_x(), fp12c_g2gen_y()}; }

// the SRS row tau^k g, k < N, then the transform as phase2.hip runs it: stage by stage, lane by lane, the 1 / N in stage 0
template <class F>
std::unique_ptr<Affine<F>[]> lagrange_basis(u32 log_n, const Fr &tau) {
    const u64 N = (u64)1 << log_n;
    std::unique_ptr<XYZZ<F>[]> x(new XYZZ<F>[N]);
    Fr pw = Fr::one();
    for (u64 k = 0; k < N; k++) {
        // through affine, as the SRS arrives
        x[k] = XYZZ<F>::from_affine(xyzz_to_affine(xyzz_scale(XYZZ<F>::from_affine(generator<F>()), pw)));
        pw = pw * tau;
    }
    const u64 half = N / 2;
    std::unique_ptr<Fr[]> tw(new Fr[half ? half : 1]);
    const Fr w_inv = fe_inv(fr_domain_generator(log_n));
    Fr t = Fr::one();
    for (u64 m = 0; m < half; m++) { tw[m] = t; t = t * w_inv; }
    const Fr n_inv = fe_inv(fe_from_u32<FrParams>((u32)N));
    for (u32 s = 0; s < log_n; s++)
        for (u64 lane = 0; lane < half; lane++) point_ntt_stage_lane(x.get(), log_n, s, lane, tw.get(), s == 0 ? n_inv : Fr::one());
    std::unique_ptr<Affine<F>[]> out(new Affine<F>[N]);
    for (u64 i = 0; i < N; i++) out[i] = xyzz_to_affine(x[i]);
    return out;
}

struct HostEntries {
    std::vector<u32> rows, coeffs;
    u32 row(u32 e) const { return rows.at(e); }
    u32 coeff(u32 e) const { return coeffs.at(e); }
};

template <class F>
void run(const std::string &cmd, std::istringstream &in) {
    if (cmd == "ntt") {
        u32 log_n; std::string tau;
        in >> log_n >> tau;
        const auto basis = lagrange_basis<F>(log_n, fe_from_hex<FrParams>(tau));
        for (u32 i = 0; i < (1u << log_n); i++) print_point(basis[bitrev_u32(i, log_n)]);
    } else if (cmd == "bfly") {
        std::string ea, eb, kt, kb;
        in >> ea >> eb >> kt >> kb;
        std::unique_ptr<XYZZ<F>[]> ab(new XYZZ<F>[2]);
        const XYZZ<F> g = XYZZ<F>::from_affine(generator<F>());
        ab[0] = xyzz_scale(g, fe_from_hex<FrParams>(ea));
        ab[1] = xyzz_scale(g, fe_from_hex<FrParams>(eb));
        point_butterfly(&ab[0], &ab[1], fe_from_hex<FrParams>(kt), fe_from_hex<FrParams>(kb));
        print_point(xyzz_to_affine(ab[0]));
        print_point(xyzz_to_affine(ab[1]));
    } else if (cmd == "col") {
        u32 log_n, n; std::string tau;
        in >> log_n >> tau >> n;
        const auto basis = lagrange_basis<F>(log_n, fe_from_hex<FrParams>(tau));
        HostEntries en;
        std::unique_ptr<Fr[]> coeffs(new Fr[n ? n : 1]);
        for (u32 e = 0; e < n; e++) {
            u32 row; std::string c;
            in >> std::hex >> row >> c;
            en.rows.push_back(row); en.coeffs.push_back(e);
            coeffs[e] = fe_from_hex<FrParams>(c);
        }
        XYZZ<F> acc = XYZZ<F>::inf();
        sparse_points_run(acc, en, 0, n, PointTerm<F>{basis.get(), coeffs.get(), log_n});
        print_point(xyzz_to_affine(acc));
    } else {
        std::printf("unknown command %s\n", cmd.c_str());
        std::exit(2);
    }
}

}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        int group = 0;
        if (!(in >> cmd >> group)) continue;
        std::printf("%s\n", line.c_str());
        if (group == 1) run<Fp>(cmd, in); else run<Fp2>(cmd, in);
        if (!in) { std::printf("malformed command\n"); return 2; }
    }
    return 0;
}

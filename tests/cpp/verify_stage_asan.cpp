// Stand-alone sanitizer run of the verifier's staged batch (gnark-whir_amd/csrc/pairing_ops.cuh, VerifyStage): built with
// -fsanitize=address,undefined -DMI_CHECK_NOWRAP by `make sanitize-stage`, run by tests/test_decode_cpu.py.  Every array a proof points
// to is a heap block of exactly the size the stage may read, so one word read too far is a report.  Keys (n_pub, nc) = (0, 0), (1, 0),
// (0, 1), (3, 3), batches of 0, 1 and 3 proofs; optional pointers are null exactly where mi_verify_input allows it (fold_challenge with
// nc = 1 too), and a proof flagged by decode_malformed has EVERY pointer null.  The flags, the first flagged index and every scalar row
// are compared with what this program wrote into the arrays itself.  Prints the number of stages checked; any mismatch exits with 1.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>
#include "../../gnark-whir_amd/csrc/pairing_ops.cuh"

namespace {
unsigned checked = 0;
void require(bool ok, const char *what, unsigned n_pub, unsigned nc, size_t n, int variant) {
    if (ok) return;
    std::printf("FAILED: %s (n_pub %u, nc %u, n %zu, variant %d)\n", what, n_pub, nc, n, variant);
    std::exit(1);
}
Fr scalar(u32 v) { Fr x = Fr::zero(); x.l[0] = v; x.l[3] = v ^ 0x5a5a5a5au; return x; }   // far below r: the top words are zero
template <class F> F not_reduced() { F x = F::zero(); for (auto &w : x.l) w = 0xffffffffu; return x; }
G1Aff generator() { return G1Aff{Fp::one(), Fp::one() + Fp::one()}; }                      // (1, 2)
template <class T> T *block(std::vector<std::unique_ptr<T[]>> &keep, size_t count, const T &fill) {
    keep.emplace_back(new T[count]);
    for (size_t i = 0; i < count; i++) keep.back()[i] = fill;
    return keep.back().get();
}

// variant 0: every proof well formed.  1: proof n / 2 flagged by decode_malformed, all of its pointers null.  2: proof n / 2 has one word
// that is not reduced (its last scalar, or with no scalar a coordinate of Krs), found by the host's checks.  3: both, at 0 and n - 1.
void run(unsigned n_pub, unsigned nc, size_t n, int variant) {
    const unsigned ns = n_pub + nc;
    std::vector<std::unique_ptr<G1Aff[]>> g1s;
    std::vector<std::unique_ptr<G2Aff[]>> g2s;
    std::vector<std::unique_ptr<Fr[]>> frs;
    std::vector<std::unique_ptr<uint8_t[]>> bytes;
    const G1Aff k0 = generator();
    const G2Aff g2{fp12c_g2gen_x(), fp12c_g2gen_y()};
    const VerifyKeyRef key{&k0, &g2, &g2, nc ? block(g2s, 2 * nc, g2) : nullptr, n_pub, nc};
    std::vector<VerifyProofRef> refs(n);
    std::vector<uint8_t> want_flags(n, 0);
    std::vector<Fr> want_scal(n * ns, Fr::zero());
    uint8_t *decode_malformed = variant & 1 ? block(bytes, n, (uint8_t)0) : nullptr;
    for (size_t i = 0; i < n; i++) {
        const bool undecoded = (variant == 1 && i == n / 2) || (variant == 3 && i == 0);
        const bool broken = (variant == 2 && i == n / 2) || (variant == 3 && i == n - 1 && n > 1);
        want_flags[i] = undecoded || broken;
        if (undecoded) {
            decode_malformed[i] = 1;
            refs[i] = VerifyProofRef{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
            continue;
        }
        Fr *pub = n_pub ? block(frs, n_pub, Fr::zero()) : nullptr, *cv = nc ? block(frs, nc, Fr::zero()) : nullptr;
        for (unsigned j = 0; j < ns; j++) (j < n_pub ? pub[j] : cv[j - n_pub]) = scalar((u32)(1000 * i + j + 1));
        G1Aff *krs = block(g1s, 1, generator());
        if (broken && ns) (nc ? cv[nc - 1] : pub[n_pub - 1]) = not_reduced<Fr>();
        if (broken && !ns) krs->y = not_reduced<Fp>();
        if (!broken)
            for (unsigned j = 0; j < ns; j++) want_scal[i * ns + j] = j < n_pub ? pub[j] : cv[j - n_pub];
        refs[i] = VerifyProofRef{block(g1s, 1, generator()), block(g2s, 1, g2), krs, nc ? block(g1s, nc, generator()) : nullptr,
                                 nc ? block(g1s, 1, generator()) : nullptr, pub, cv, nc > 1 ? block(frs, 1, scalar(7)) : nullptr};
    }
    size_t want_first = n;
    for (size_t i = n; i-- > 0;)
        if (want_flags[i]) want_first = i;
    VerifyStage st(key, refs, decode_malformed);
    require(st.n() == n && st.n_pub == n_pub && st.nc == nc && st.ns == ns, "counts", n_pub, nc, n, variant);
    require(st.flags == want_flags, "flags", n_pub, nc, n, variant);
    require(st.first_flagged == want_first, "first flagged index", n_pub, nc, n, variant);
    require(st.scal.size() == want_scal.size(), "size of the scalar matrix", n_pub, nc, n, variant);
    for (size_t t = 0; t < want_scal.size(); t++) require(st.scal[t] == want_scal[t], "scalar row", n_pub, nc, n, variant);
    // the device's answer: the last proof outside the r-torsion
    if (n) {
        uint8_t *dev = block(bytes, n, (uint8_t)0);
        dev[n - 1] = 1;
        st.merge(dev);
        want_flags[n - 1] = 1;
        require(st.flags == want_flags && st.first_flagged == (want_first < n ? want_first : n - 1), "merged flags", n_pub, nc, n, variant);
    }
    checked++;
}
}   // namespace

int main() {
    const unsigned keys[4][2] = {{0, 0}, {1, 0}, {0, 1}, {3, 3}};
    for (const auto &k : keys)
        for (size_t n : {0, 1, 3})
            for (int variant = 0; variant < 4; variant++) run(k[0], k[1], n, variant);
    std::printf("%u\n", checked);
    return 0;
}

// Stand-alone sanitizer run of the wave-per-pairing phases (gnark-whir_amd/csrc/fp12_wave.cuh, pairing_wave.cuh): built with
// -fsanitize=address,undefined -DMI_CHECK_NOWRAP by `make sanitize-pairing-wave`, run by tests/test_pairing_wave_cpu.py.  The image is a
// heap block of exactly MI_WAVE_IMAGE_RECORDS records, the size the phases declare, so one record read or written past it is a report.
// One product, one line product, one Miller loop and one final exponentiation, each compared with the one-lane body of fp12.cuh /
// pairing.cuh.  Prints the number of comparisons and "checked"; any mismatch exits with 1.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include "../../gnark-whir_amd/csrc/pairing_wave.cuh"

namespace {
unsigned checked = 0;
void require(bool ok, const char *what) {
    if (!ok) { std::printf("FAILED: %s\n", what); std::exit(1); }
    checked++;
}
Fp2 small(u32 v) { return Fp2{fe_from_u32<FpParams>(v), fe_from_u32<FpParams>(v ^ 0x9e3779b9u)}; }
Fp12 value(u32 seed) {
    return Fp12{Fp6{small(seed), small(seed + 1), small(seed + 2)}, Fp6{small(seed + 3), small(seed + 4), small(seed + 5)}};
}
}   // namespace

int main() {
    std::unique_ptr<Fp2[]> image(new Fp2[MI_WAVE_IMAGE_RECORDS]);
    Fp2 *im = image.get();
    for (u32 i = 0; i < MI_WAVE_IMAGE_RECORDS; i++) im[i] = Fp2::zero();
    const Fp12 x = value(3), y = value(1000);
    Fp12 want, got;

    w12_put(im, MI_WAVE_S(1), x);
    w12_put(im, MI_WAVE_S(6), y);                 // the last slot in front of the products
    w12_mul(im, MI_WAVE_S(0), MI_WAVE_S(1), MI_WAVE_S(6));
    fp12_mul(&want, &x, &y);
    require(w12_get(im, MI_WAVE_S(0)) == want, "product");

    im[WM_L0] = y.c0.b0; im[WM_L3] = y.c1.b0; im[WM_L4] = y.c1.b1;
    w12_mul_line(im, MI_WAVE_S(6), MI_WAVE_S(1), WM_L0, WM_L3, WM_L4);
    fp12_mul_by_line(&want, &x, &y.c0.b0, &y.c1.b0, &y.c1.b1);
    require(w12_get(im, MI_WAVE_S(6)) == want, "line product");

    const G1Aff p = g1_generator();
    const G2Aff q = g2_generator();
    wave_miller_loop(im, &p, &q);
    pairing_miller_loop(&want, &p, &q);
    MI_WAVE_PHASE(w12_ph_store(lane, im, &got, MI_WAVE_S(0)));
    require(got == want, "Miller loop");

    wave_final_exp(im);
    pairing_final_exp(&want, &want);
    require(w12_get(im, MI_WAVE_S(0)) == want && !(want == Fp12::one()), "final exponentiation");
    std::printf("%u checked\n", checked);
    return 0;
}

"""Generates tests/golden/pairing.json from the definitional reference tests/pairing_ref.py: a handful of (P, Q, e(P, Q)^s) triples
(canonical hex; GT as the 12 tower coefficients) and one accepted toy proof with its verifying key.  A guard against drift of the
reference, the tower order or the exponent.  Run: python tools/gen_pairing_golden.py"""
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import pyref as P            # noqa: E402
import pairing_ref as R      # noqa: E402
import verify_cases as V     # noqa: E402

h = lambda v: hex(v)
h1 = lambda pt: None if pt is None else [h(pt[0]), h(pt[1])]
h2 = lambda pt: None if pt is None else [h(pt[0][0]), h(pt[0][1]), h(pt[1][0]), h(pt[1][1])]


def main():
    pairs = [(P.G1_GEN, P.G2_GEN), (P.g1_mul(P.G1_GEN, 2), P.g2_mul(P.G2_GEN, 3)), (P.g1_mul(P.G1_GEN, R.r - 1), P.G2_GEN),
             (P.g1_mul(P.G1_GEN, 0xDEADBEEF), P.g2_mul(P.G2_GEN, 0xC0FFEE)), (None, P.G2_GEN)]
    triples = [{"p": h1(a), "q": h2(b), "gt": [h(c) for c in R.pairing_tower(a, b)]} for a, b in pairs]
    case = V.toy_case(0)
    assert V.ref_verdict(case) == R.OK
    vk = case["vk"]
    proof = {"alpha1": h1(vk["alpha1"]), "beta2": h2(vk["beta2"]), "gamma2": h2(vk["gamma2"]), "delta2": h2(vk["delta2"]),
             "k": [h1(k) for k in vk["k"]], "nb_public": vk["nb_public"], "ar": h1(case["proof"][0]), "bs": h2(case["proof"][1]),
             "krs": h1(case["proof"][2]), "public_inputs": [h(v) for v in case["public_inputs"]]}
    out = os.path.join(ROOT, "tests", "golden", "pairing.json")
    with open(out, "w") as f:
        json.dump({"d_prime_bits": R.D_PRIME.bit_length(), "triples": triples, "proof": proof}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

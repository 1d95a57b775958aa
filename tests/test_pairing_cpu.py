"""CPU suite: the tower, the pairing and the verifier's judgement of gnark-whir_amd/csrc/fp12.cuh / pairing.cuh / pairing_ops.cuh in
their host build (tests/emu/emu_pairing.cpp, -DMI_CHECK_NOWRAP: every bound of the arithmetic underneath traps) against the definitional
reference tests/pairing_ref.py, which shares no formula with them, and whole toy proofs against pyref.trapdoor_check."""
import ctypes as C
import json
import os
import random
import numpy as np
import pytest
import pyref as P
import pairing_ref as R
import verify_cases as V
from helpers import g1_arr, g2_arr

p, r = R.p, R.r
ft, tt = R.from_tower, R.to_tower


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return C.CDLL(V.build_emu(str(tmp_path_factory.mktemp("emu") / "libemu_pairing.so")))


def _op(emu, op, xs, ys=None):
    X = V.gt_arr(xs); Y = None if ys is None else V.gt_arr(ys); Z = np.zeros_like(X)
    assert emu.emu_fp12_op(C.c_int(op), V.p_(Z), V.p_(X), V.p_(Y), C.c_size_t(len(X))) == 0
    return V.gt_vals(Z)


def _pair(emu, ps, qs, final=True):
    pa, qa = g1_arr(ps), g2_arr(qs); out = np.zeros((len(ps), 48), np.uint64)
    assert emu.emu_pairing(V.p_(pa), V.p_(qa), C.c_size_t(len(ps)), V.p_(out), C.c_uint(1 if final else 0)) == 0
    return V.gt_vals(out)


def _operands():
    rnd = random.Random(2024)
    edge = [[0] * 12, [1] + [0] * 11, [p - 1] * 12, [0] * 11 + [1], [p - 1] + [0] * 11, [1] * 12]
    return edge + [[rnd.randrange(p) for _ in range(12)] for _ in range(6)]


def test_reference_checks_itself():
    g = R.pairing(P.G1_GEN, P.G2_GEN)
    assert g != R.ONE and R.f_pow(g, r) == R.ONE
    assert R.f_mul(g, R.f_inv(g)) == R.ONE and ft(tt(g)) == g
    assert R.pairing(P.g1_mul(P.G1_GEN, 3), P.g2_mul(P.G2_GEN, 5)) == R.f_pow(g, 15)
    assert ft([0, 1] + [0] * 10) == R.f_sub(tuple(1 if k == 6 else 0 for k in range(12)), R.f_scalar(9))   # u = w^6 - 9
    assert R.D_PRIME % r != 0 and R.S_COFACTOR * ((p ** 4 - p ** 2 + 1) // r) * (p ** 6 - 1) * (p ** 2 + 1) == R.D_PRIME


def test_fp12_ops_equal_the_reference(emu):
    xs = _operands(); ys = xs[3:] + xs[:3]
    fx, fy = [ft(x) for x in xs], [ft(y) for y in ys]
    assert _op(emu, V.F12_MUL, xs, ys) == [tt(R.f_mul(a, b)) for a, b in zip(fx, fy)]
    assert _op(emu, V.F12_ADD, xs, ys) == [tt(R.f_add(a, b)) for a, b in zip(fx, fy)]
    assert _op(emu, V.F12_SUB, xs, ys) == [tt(R.f_sub(a, b)) for a, b in zip(fx, fy)]
    assert _op(emu, V.F12_SQR, xs) == [tt(R.f_mul(a, a)) for a in fx]
    assert _op(emu, V.F12_CONJ, xs) == [tt(R.f_pow(a, p ** 6)) for a in fx]
    for k, op in ((1, V.F12_FROB1), (2, V.F12_FROB2), (3, V.F12_FROB3)):
        assert _op(emu, op, xs) == [tt(R.f_pow(a, p ** k)) for a in fx], k
    inv = _op(emu, V.F12_INV, xs)
    assert inv[0] == [0] * 12                                                      # 0 -> 0
    assert inv[1:] == [tt(R.f_inv(a)) for a in fx[1:]]
    assert _op(emu, V.F12_MUL, xs[1:], inv[1:]) == [tt(R.ONE)] * (len(xs) - 1)     # x x^-1 = 1
    sparse = [[y[i] if i in (0, 1, 6, 7, 8, 9) else 0 for i in range(12)] for y in ys]
    assert _op(emu, V.F12_MUL_LINE, xs, ys) == [tt(R.f_mul(a, ft(sp))) for a, sp in zip(fx, sparse)]
    # Frobenius identities: p then p^2 is p^3; p^2 three times is p^6 = conj; p six times... on the device code alone
    assert _op(emu, V.F12_FROB2, _op(emu, V.F12_FROB1, xs)) == _op(emu, V.F12_FROB3, xs)
    assert _op(emu, V.F12_FROB3, _op(emu, V.F12_FROB3, xs)) == _op(emu, V.F12_CONJ, xs)


def test_fp6_layer_equals_the_reference(emu):
    xs = _operands(); ys = xs[2:] + xs[:2]
    half = lambda t, i: ft([t[k] if k // 6 == i else 0 for k in range(12)])
    got = _op(emu, V.F12_FP6_MUL, xs, ys)
    W1_inv = R.f_inv(tuple(1 if k == 1 else 0 for k in range(12)))
    for x, y, g in zip(xs, ys, got):
        want0 = tt(R.f_mul(half(x, 0), half(y, 0)))
        want1 = tt(R.f_mul(R.f_mul(half(x, 1), half(y, 1)), W1_inv))     # (a w)(b w) / w = a b w
        assert g[:6] == want0[:6] and g[6:] == want1[6:] and not any(want0[6:]) and not any(want1[:6])
    sq = _op(emu, V.F12_FP6_SQR, xs)
    assert sq == _op(emu, V.F12_FP6_MUL, xs, xs)
    nz = [xs[2], xs[5]] + xs[6:]                                     # operands whose two halves are both non-zero
    inv = _op(emu, V.F12_FP6_INV, nz)
    one6 = [1] + [0] * 5
    assert _op(emu, V.F12_FP6_MUL, nz, inv) == [one6 + one6] * len(inv)
    assert _op(emu, V.F12_FP6_INV, [xs[0]]) == [[0] * 12]             # 0 -> 0


def test_final_exponentiation_is_one_pow_by_d_prime(emu):
    xs = _operands()[6:10]
    assert _op(emu, V.F12_EASY, xs) == [tt(R.f_pow(ft(x), (p ** 6 - 1) * (p ** 2 + 1))) for x in xs]
    assert _op(emu, V.F12_FINAL_EXP, xs) == [tt(R.f_pow(ft(x), R.D_PRIME)) for x in xs]
    easy = _op(emu, V.F12_EASY, xs)
    assert _op(emu, V.F12_CYCLO_SQR, easy) == _op(emu, V.F12_SQR, easy)            # in the cyclotomic subgroup only
    assert _op(emu, V.F12_CYCLO_SQR, xs) != _op(emu, V.F12_SQR, xs)


def test_pairing_bit_equal_for_seeded_pairs(emu):
    rnd = random.Random(99)
    ps = [P.g1_mul(P.G1_GEN, rnd.randrange(1, r)) for _ in range(8)]
    qs = [P.g2_mul(P.G2_GEN, rnd.randrange(1, r)) for _ in range(8)]
    got = _pair(emu, ps, qs)
    assert got == [R.pairing_tower(a, b) for a, b in zip(ps, qs)]
    # the Miller values differ from the reference's by subfield factors only: equal after the final exponentiation
    ml = _pair(emu, ps[:2], qs[:2], final=False)
    assert _op(emu, V.F12_FINAL_EXP, ml) == got[:2]


def test_bilinearity_order_and_infinity(emu):
    g = R.pairing(P.G1_GEN, P.G2_GEN)
    for a, b in ((0, 1), (1, 0), (1, 1), (r - 1, 1), (1, r - 1), (r - 1, r - 1), (2, 3)):
        got = _pair(emu, [P.g1_mul(P.G1_GEN, a)], [P.g2_mul(P.G2_GEN, b)])[0]
        assert got == tt(R.f_pow(g, a * b % r)), (a, b)
    e = _pair(emu, [P.G1_GEN, P.g1_neg(P.G1_GEN), None, P.G1_GEN, None], [P.G2_GEN, P.G2_GEN, P.G2_GEN, None, None])
    one = tt(R.ONE)
    assert e[0] != one and tt(R.f_pow(ft(e[0]), r)) == one
    assert _op(emu, V.F12_MUL, [e[0]], [e[1]]) == [one]
    assert e[2] == one and e[3] == one and e[4] == one
    assert _pair(emu, [None, P.G1_GEN], [P.G2_GEN, None], final=False) == [one, one]


def test_point_checks(emu):
    q_bad = V.twist_point_outside_subgroup()
    for Q, on, sub in ((P.G2_GEN, 1, 1), (None, 1, 1), (q_bad, 1, 0), (((1, 2), (3, 4)), 0, 0)):
        a = g2_arr([Q])
        assert (emu.emu_g2_on_twist(V.p_(a)), emu.emu_g2_in_subgroup(V.p_(a))) == (on, sub)
        assert R.g2_in_subgroup(Q) == bool(sub)
    for Pt, on in ((P.G1_GEN, 1), (None, 1), ((1, 3), 0)):
        assert emu.emu_g1_on_curve(V.p_(g1_arr([Pt]))) == on


@pytest.mark.parametrize("n_commitments", [0, 1])
def test_whole_verification_of_a_toy_proof(emu, n_commitments):
    """the host bodies of what the device runs per proof (Miller loops of its pairs, verify_judge) against groth16_verify of the reference
    and against pyref.trapdoor_check on the same proof; then one tamper per verdict code"""
    case = V.toy_case(n_commitments)
    assert P.trapdoor_check(case["cs"], case["td"], case["exps"], case["toy_proof"], case["r"], case["s"])
    eab = V.gt_arr([R.pairing_tower(case["vk"]["alpha1"], case["vk"]["beta2"])])

    def judge(**over):
        pa, qa, n_ped = V.emu_pairs(case, **over)
        return emu.emu_verify_pairs(V.p_(pa), V.p_(qa), C.c_uint(n_ped), V.p_(eab), 0)

    assert V.ref_verdict(case) == R.OK and judge() == R.OK
    ar, bs, krs = case["proof"]
    other = P.g1_mul(P.G1_GEN, 12345)
    for over in (dict(proof=(other, bs, krs)), dict(proof=(ar, bs, other)), dict(public_inputs=[case["public_inputs"][0] + 1] + case["public_inputs"][1:])):
        assert V.ref_verdict(case, **over) == R.PAIRING and judge(**over) == R.PAIRING
    bad = dict(case["toy_proof"], krs=other)
    assert not P.trapdoor_check(case["cs"], case["td"], case["exps"], bad, case["r"], case["s"])
    if n_commitments:
        over = dict(pok=other)
        assert V.ref_verdict(case, **over) == R.PEDERSEN and judge(**over) == R.PEDERSEN
        over = dict(commitment_values=[case["commitment_values"][0] + 1])
        assert V.ref_verdict(case, **over) == R.PAIRING and judge(**over) == R.PAIRING
    pa, qa, n_ped = V.emu_pairs(case)
    assert emu.emu_verify_pairs(V.p_(pa), V.p_(qa), C.c_uint(n_ped), V.p_(eab), 1) == R.MALFORMED


def test_golden_fixture_has_not_drifted(emu):
    """tests/golden/pairing.json (tools/gen_pairing_golden.py, from the reference): the triples through the host bodies, the proof
    through the reference"""
    path = os.path.join(V.HERE, "golden", "pairing.json")
    g = json.load(open(path))
    assert g["d_prime_bits"] == R.D_PRIME.bit_length() and len(g["triples"]) >= 4
    pt1 = lambda v: None if v is None else (int(v[0], 16), int(v[1], 16))
    pt2 = lambda v: None if v is None else ((int(v[0], 16), int(v[1], 16)), (int(v[2], 16), int(v[3], 16)))
    ps = [pt1(t["p"]) for t in g["triples"]]; qs = [pt2(t["q"]) for t in g["triples"]]
    assert _pair(emu, ps, qs) == [[int(c, 16) for c in t["gt"]] for t in g["triples"]]
    pr = g["proof"]
    vk = {"alpha1": pt1(pr["alpha1"]), "beta2": pt2(pr["beta2"]), "gamma2": pt2(pr["gamma2"]), "delta2": pt2(pr["delta2"]),
          "k": [pt1(k) for k in pr["k"]], "nb_public": pr["nb_public"], "ped": []}
    proof = (pt1(pr["ar"]), pt2(pr["bs"]), pt1(pr["krs"]))
    assert R.groth16_verify(vk, proof, [int(v, 16) for v in pr["public_inputs"]]) == R.OK

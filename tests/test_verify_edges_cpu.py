"""CPU suite: the HOST half of groth16.Verify -- the range and curve checks, kSum, the folded commitments, the layout of the pairs
(verify_well_formed / verify_assemble of gnark-whir_amd/csrc/pairing_ops.cuh, which csrc/verify.hip calls) -- in the host build
(tests/emu/emu_pairing.cpp: emu_verify_assemble, -DMI_CHECK_NOWRAP, so a word that is not reduced and reaches the arithmetic traps)
on forged, edge and non-reduced inputs.  The expected verdict of every case is computed in the exponent (tests/verify_forge.py); one
case of each kind also goes through the definitional pairing (tests/pairing_ref.py), which ties the exponent rule to the equations."""
import ctypes as C
import time
import numpy as np
import pytest
import cref
import pyref as P
import pairing_ref as R
import verify_cases as V
import verify_forge as F
from helpers import g1_arr, g2_arr

p, r = R.p, R.r


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return C.CDLL(V.build_emu(str(tmp_path_factory.mktemp("emu") / "libemu_pairing.so")))


@pytest.fixture(scope="module")
def judge(emu):
    """(vk, verify_input dict) -> the verdict of emu_verify_assemble; e(alpha, beta) once per key, by the host build's own pairing
    (bit-equal to the reference: tests/test_pairing_cpu.py)"""
    keys = {}

    def run(vk, inp):
        if id(vk) not in keys:
            d, nbp, ped = V.vk_arrays(vk)
            eab = np.zeros((1, 48), np.uint64)
            assert emu.emu_pairing(V.p_(d["alpha1"]), V.p_(d["beta2"]), C.c_size_t(1), V.p_(eab), C.c_uint(1)) == 0
            keys[id(vk)] = (vk, d, nbp, ped, eab)
        _, d, nbp, ped, eab = keys[id(vk)]
        a = {n: (None if inp.get(n) is None else np.ascontiguousarray(inp[n], np.uint64)) for n in
             ("raw", "commitments", "pok", "public_inputs", "commitment_values", "fold_challenge")}
        return emu.emu_verify_assemble(V.p_(d["k"]), V.p_(d["gamma2"]), V.p_(d["delta2"]), V.p_(ped), C.c_uint(nbp),
                                       C.c_uint(0 if ped is None else len(ped)), V.p_(eab), V.p_(a["raw"]), V.p_(a["commitments"]), V.p_(a["pok"]),
                                       V.p_(a["public_inputs"]), V.p_(a["commitment_values"]), V.p_(a["fold_challenge"]))
    return run


def test_the_case_list_states_what_the_exponent_rule_computes():
    """the list is written down by hand, verdict_in_exponent computes: they agree, every verdict and every key shape occurs, and every
    word of a non-reduced case lies in [its modulus, 2^256) (verify_input asserts that while it builds the arrays)"""
    t = time.perf_counter()
    cases = F.cases()
    for c in cases:
        assert F.verdict_in_exponent(c["key"], c) == c["want"], c["name"]
        inp = F.verify_input(c)
        for field, i, _ in c["words"]:
            v = cref.limbs_to_int(inp[field].reshape(-1, 4)[~i if i < 0 else i])
            assert F.WORD_FIELDS[field] <= v < 1 << 256, c["name"]
    print(f"\n{len(cases)} cases and their arrays built in {time.perf_counter() - t:.2f} s")
    assert {c["want"] for c in cases} == {R.OK, R.PAIRING, R.PEDERSEN, R.MALFORMED}
    shapes = {(c["key"]["nb_public"], c["key"]["n_commitments"]) for c in cases}
    assert shapes == set(F.KEY_SHAPES)
    assert len({c["name"] for c in cases}) == len(cases)
    assert sum(c["want"] == R.OK for c in cases) >= 30 and sum(bool(c["words"]) for c in cases) >= 15


def test_every_case_through_the_host_half(judge):
    bad = []
    for c in F.cases():
        got = judge(c["key"]["vk"], F.verify_input(c))
        if got != c["want"]:
            bad.append((c["name"], got, c["want"]))
    assert not bad, bad


def test_one_case_of_each_kind_through_the_definitional_pairing(judge):
    """the first case of each kind on the key with the fewest pairs; the non-reduced ones are left out: the reference works on
    integers and has no second encoding of anything"""
    first = {}
    for c in sorted(F.cases(), key=lambda c: c["key"]["n_commitments"]):
        if not c["words"]:
            first.setdefault(c["kind"], c)
    assert len(first) >= 25
    for kind, c in first.items():
        assert R.groth16_verify(*F.ref_args(c)) == c["want"] == judge(c["key"]["vk"], F.verify_input(c)), c["name"]


@pytest.mark.parametrize("n_commitments", [0, 1, 2, 3])
def test_honest_toy_proofs_three_judges_agree(judge, n_commitments):
    """a proof of a real (toy) circuit: pyref.trapdoor_check, the exponent rule over the same trapdoor, the host half"""
    case = V.toy_case(n_commitments)
    cs, td, exps, q = case["cs"], case["td"], case["exps"], r
    assert P.trapdoor_check(cs, td, exps, case["toy_proof"], case["r"], case["s"])
    nbp, w = cs.nb_public, cs.wires
    kg = lambda j: exps["K"][j] * td.delta % q * P.fr_inv(td.gamma) % q
    priv = list(range(nbp, cs.nb_wires))
    commits = [(priv[3 * k: 3 * k + 2], priv[3 * k + 2]) for k in range(n_commitments)]          # as verify_cases.toy_case lays them out
    key = {"exps": {"alpha": td.alpha, "beta": td.beta, "gamma": td.gamma, "delta": td.delta,
                    "k": [kg(j) for j in range(nbp)] + [kg(cw) for _, cw in commits], "sigma": case["sigmas"]},
           "vk": case["vk"], "nb_public": nbp, "n_commitments": n_commitments, "id": "toy"}
    assert [F.g1(e) for e in key["exps"]["k"]] == case["vk"]["k"] and F.g2(td.gamma) == case["vk"]["gamma2"]
    cm = [sum(w[j] * kg(j) for j in wires) % q for wires, _ in commits]
    # the logs of the prover's own Ar, Bs, Krs, as pyref.trapdoor_check derives them from (W, h, r, s); Krs without the K points of the
    # committed wires
    A, B, K, Z = exps["A"], exps["B"], exps["K"], exps["Z"]
    a = (td.alpha + sum(w[j] * A[j] for j in range(cs.nb_wires)) + case["r"] * td.delta) % q
    b = (td.beta + sum(w[j] * B[j] for j in range(cs.nb_wires)) + case["s"] * td.delta) % q
    h_nat = P.bit_reverse_perm(case["toy_proof"]["h"])
    committed = [j for wires, cw in commits for j in wires + [cw]]
    krs = (sum(w[j] * K[j] for j in range(nbp, cs.nb_wires) if j not in committed) + sum(h_nat[i] * Z[i] for i in range(len(Z) - 1))
           + case["s"] * a + case["r"] * b - case["r"] * case["s"] * td.delta) % q
    rec = {"key": key, "pub": case["public_inputs"], "cm": cm, "cv": case["commitment_values"], "fold": case["fold_challenge"], "a": a, "b": b,
           "krs": krs, "pok": F.pok_of(key, cm, case["fold_challenge"]), "points": {}, "words": [], "malformed": None, "name": "toy"}
    pts = F.case_points(rec)
    assert (pts["ar"], pts["bs"], pts["krs"]) == tuple(case["proof"]) and pts["cm"] == case["commitments"] and pts["pok"] == case["pok"]
    assert F.verdict_in_exponent(key, rec) == R.OK
    assert judge(case["vk"], V.proof_dict(case)) == R.OK
    assert np.array_equal(F.verify_input(rec)["raw"], V.proof_dict(case)["raw"])
    bad = F.but(rec, pub=[(rec["pub"][0] + 1) % q] + rec["pub"][1:])
    assert F.verdict_in_exponent(key, bad) == R.PAIRING and judge(case["vk"], F.verify_input(bad)) == R.PAIRING


def test_point_checks_refuse_words_that_are_not_reduced(emu):
    """x + p is the same element to the arithmetic (2 p < 2^256) and (p, p) compares unequal to (0, 0): the range check says no to both"""
    mp = cref.int_to_limbs(p)

    def plus_p(arr, i):
        a = arr.copy(); rows = a.reshape(-1, 4)
        v = cref.limbs_to_int(rows[i]) + p
        assert p <= v < 1 << 256
        rows[i] = cref.int_to_limbs(v)
        return a

    g = g1_arr([P.G1_GEN])
    assert emu.emu_g1_reduced(V.p_(g)) == 1 and emu.emu_g1_on_curve(V.p_(g)) == 1
    for i in range(2):
        assert emu.emu_g1_reduced(V.p_(plus_p(g, i))) == 0 and emu.emu_g1_on_curve(V.p_(plus_p(g, i))) == 0, i
    inf2 = np.array([mp + mp], np.uint64)
    assert emu.emu_g1_reduced(V.p_(inf2)) == 0 and emu.emu_g1_on_curve(V.p_(inf2)) == 0
    assert emu.emu_g1_on_curve(V.p_(g1_arr([None]))) == 1
    ones = np.full((1, 8), (1 << 64) - 1, np.uint64)
    assert emu.emu_g1_on_curve(V.p_(ones)) == 0
    edge = np.array([cref.int_to_limbs(p - 1) + cref.int_to_limbs(p - 1)], np.uint64)     # the largest reduced words: in range, off the curve
    assert emu.emu_g1_reduced(V.p_(edge)) == 1
    h = g2_arr([P.G2_GEN])
    assert emu.emu_g2_reduced(V.p_(h)) == 1 and emu.emu_g2_in_subgroup(V.p_(h)) == 1
    for i in range(4):
        assert emu.emu_g2_reduced(V.p_(plus_p(h, i))) == 0, i
    assert emu.emu_g2_reduced(V.p_(np.array([mp * 4], np.uint64))) == 0 and emu.emu_g2_reduced(V.p_(g2_arr([None]))) == 1

"""CPU suite: the wave-per-pairing text of gnark-whir_amd/csrc/fp12_wave.cuh and pairing_wave.cuh in its host build (tests/emu/
emu_pairing_wave.cpp, -DMI_CHECK_NOWRAP, the 64 lanes of a phase run as a loop) against the one-lane bodies of fp12.cuh, pairing.cuh and
pairing_ops.cuh in theirs (tests/emu/emu_pairing.cpp): every Fp result is fully reduced, so another order of evaluation must give the
same words, and every comparison here is exact.  One pair also goes through the definitional reference (tests/pairing_ref.py), the
verdicts of tests/verify_forge.py's cases through the verdict computed in the exponent, and a stand-alone program runs the phases under
AddressSanitizer over an image of exactly the declared size."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import pairing_ref as R
import verify_cases as V
import verify_forge as F
from helpers import g1_arr, g2_arr
from gpu_common import ROOT

p = R.p
ONE_OPERAND = (V.F12_SQR, V.F12_INV, V.F12_FROB1, V.F12_FROB2, V.F12_FROB3, V.F12_CYCLO_SQR, V.F12_CONJ, V.F12_EASY)
ALIASED = ONE_OPERAND + (V.F12_MUL, V.F12_MUL_LINE, V.F12_ADD, V.F12_SUB)     # the ops with one call of fp12_wave.cuh behind them


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return C.CDLL(V.build_emu(str(tmp_path_factory.mktemp("emu") / "libemu_pairing.so")))


@pytest.fixture(scope="module")
def wave(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu_wave") / "libemu_pairing_wave.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DMI_CHECK_NOWRAP", "-shared", "-fPIC", "-o", so, os.path.join(V.HERE, "emu", "emu_pairing_wave.cpp")])
    return C.CDLL(so)


def _ref_op(emu, op, X, Y):
    Z = np.zeros_like(X)
    assert emu.emu_fp12_op(C.c_int(op), V.p_(Z), V.p_(X), V.p_(Y), C.c_size_t(len(X))) == 0
    return Z


def _wave_op(wave, op, X, Y, alias=0):
    Z = np.zeros_like(X)
    assert wave.emu_wave_fp12_op(C.c_int(op), V.p_(Z), V.p_(X), V.p_(Y), C.c_size_t(len(X)), C.c_int(alias)) == 0, (op, alias)
    return Z


def _operands():
    """the operand set of test_gpu_verify.py's test_fp12_ops_equal_the_host_build_and_the_reference: all-zero, one, all p - 1, seeded"""
    rng = np.random.default_rng(77 + 65)
    edge = [[0] * 12, [1] + [0] * 11, [p - 1] * 12]
    xs = edge + [[int.from_bytes(rng.bytes(31), "little") for _ in range(12)] for _ in range(9)]
    X = V.gt_arr(xs)
    return X, np.ascontiguousarray(X[::-1])


def test_every_op_equals_the_one_lane_build(emu, wave):
    X, Y = _operands()
    for op in range(V.F12_OP_END):
        if op == V.F12_CYCLO_SQR:
            continue
        assert np.array_equal(_wave_op(wave, op, X, Y), _ref_op(emu, op, X, Y)), op
    assert wave.emu_wave_fp12_op(C.c_int(V.F12_OP_END), V.p_(X), V.p_(X), V.p_(Y), C.c_size_t(1), C.c_int(0)) == -1
    assert wave.emu_wave_image_bytes() == 102 * 64


def test_cyclotomic_squaring_after_the_easy_part(emu, wave):
    X, Y = _operands()
    E = _ref_op(emu, V.F12_EASY, X[3:], None)
    got = _wave_op(wave, V.F12_CYCLO_SQR, E, None)
    assert np.array_equal(got, _ref_op(emu, V.F12_CYCLO_SQR, E, None)) and np.array_equal(got, _ref_op(emu, V.F12_SQR, E, None))
    assert np.array_equal(_wave_op(wave, V.F12_CYCLO_SQR, E, None, alias=1), got)


def test_outputs_may_alias_each_input(emu, wave):
    X, Y = _operands()
    for op in ALIASED:
        if op == V.F12_CYCLO_SQR:
            continue
        want = _ref_op(emu, op, X, Y)
        for alias in (1,) if op in ONE_OPERAND else (1, 2):
            assert np.array_equal(_wave_op(wave, op, X, Y, alias), want), (op, alias)


@pytest.mark.parametrize("seed", [11, 12])
def test_miller_values_and_pairings_of_seeded_pairs(emu, wave, seed):
    """infinity in G1 first and in G2 last"""
    ps, qs = V.seeded_pairs(5, seed)
    assert ps[0] is None and qs[-1] is None
    pa, qa = g1_arr(ps), g2_arr(qs)
    for flags in (0, 1):
        want = np.zeros((5, 48), np.uint64); got = np.zeros_like(want)
        assert emu.emu_pairing(V.p_(pa), V.p_(qa), C.c_size_t(5), V.p_(want), C.c_uint(flags)) == 0
        assert wave.emu_wave_pairing(V.p_(pa), V.p_(qa), C.c_size_t(5), V.p_(got), C.c_uint(flags)) == 0
        assert np.array_equal(got, want), flags
    one = V.gt_arr([R.to_tower(R.ONE)])[0]
    assert np.array_equal(got[0], one) and np.array_equal(got[-1], one) and not np.array_equal(got[1], one)
    if seed == 11:
        assert V.gt_vals(got[2:3]) == [R.pairing_tower(ps[2], qs[2])]


def test_bs_check_is_the_answer_of_the_multiplication_by_r(emu, wave):
    for Q in (V.P.G2_GEN, None, V.twist_point_outside_subgroup(), ((1, 2), (3, 4)), V.P.g2_mul(V.P.G2_GEN, 0x1234567)):
        a = g2_arr([Q])
        assert wave.emu_wave_bs_in_subgroup(V.p_(a)) == emu.emu_g2_in_subgroup(V.p_(a)) == int(R.g2_in_subgroup(Q)), Q


def _judges(emu, wave):
    keys = {}

    def run(lib_fn, vk, inp):
        if id(vk) not in keys:
            d, nbp, ped = V.vk_arrays(vk)
            eab = np.zeros((1, 48), np.uint64)
            assert emu.emu_pairing(V.p_(d["alpha1"]), V.p_(d["beta2"]), C.c_size_t(1), V.p_(eab), C.c_uint(1)) == 0
            keys[id(vk)] = (vk, d, nbp, ped, eab)
        _, d, nbp, ped, eab = keys[id(vk)]
        a = {n: (None if inp.get(n) is None else np.ascontiguousarray(inp[n], np.uint64)) for n in
             ("raw", "commitments", "pok", "public_inputs", "commitment_values", "fold_challenge")}
        return lib_fn(V.p_(d["k"]), V.p_(d["gamma2"]), V.p_(d["delta2"]), V.p_(ped), C.c_uint(nbp), C.c_uint(0 if ped is None else len(ped)),
                      V.p_(eab), V.p_(a["raw"]), V.p_(a["commitments"]), V.p_(a["pok"]), V.p_(a["public_inputs"]), V.p_(a["commitment_values"]),
                      V.p_(a["fold_challenge"]))
    return run


def _two_commitment_cases():
    """verify_forge's list has keys of 0, 1, 3 and 16 commitments; the same kinds for a key of two"""
    key = F.forge_key(2, 2)
    h = F.honest(key, 120)
    out = [("honest", h)]
    for which in ("krs", "pub", "cv", "cm", "pok", "fold"):
        out.append((f"{which} + 1", F._tweaked(h, which)[0]))
    out.append(("Bs = infinity", F.but(h, b=0)))
    out.append(("Bs outside the r-torsion and pok + 1", F.but(h, pok=(h["pok"] + 1) % F.r, points={"bs": V.twist_point_outside_subgroup()}, malformed="outside the r-torsion")))
    out.append(("Bs off the twist", F.but(h, points={"bs": ((1, 2), (3, 4))}, malformed="off the twist")))
    out.append(("Krs.y + p", F.but(h, words=[("raw", F.RAW["Krs.y"], F.p)])))
    return [dict(c, name=f"{key['id']}: {name}") for name, c in out]


def test_wave_verdicts_are_the_verdicts_in_the_exponent(emu, wave):
    """accepted, rejected, edge and non-reduced cases of tests/verify_forge.py for keys of 0, 1 and 3 commitments, and the same kinds
    for a key of 2, through the wave's Bs check, Miller loops and judgement"""
    run = _judges(emu, wave)
    cases = [c for c in F.cases() if c["key"]["n_commitments"] <= 3] + _two_commitment_cases()
    assert {c["key"]["n_commitments"] for c in cases} == {0, 1, 2, 3}
    bad, seen = [], set()
    for c in cases:
        want = F.verdict_in_exponent(c["key"], c)
        got = run(wave.emu_wave_verify_assemble, c["key"]["vk"], F.verify_input(c))
        seen.add(want)
        if got != want:
            bad.append((c["name"], got, want))
    assert not bad, bad
    assert seen == {R.OK, R.PAIRING, R.PEDERSEN, R.MALFORMED}


def test_wave_verdict_equals_the_one_lane_judgement_on_a_key_of_sixteen_commitments(emu, wave):
    run = _judges(emu, wave)
    mine = [c for c in F.cases() if c["key"]["n_commitments"] == 16][:3]
    assert mine
    for c in mine:
        inp = F.verify_input(c)
        assert run(wave.emu_wave_verify_assemble, c["key"]["vk"], inp) == run(emu.emu_verify_assemble, c["key"]["vk"], inp) == c["want"], c["name"]


def test_the_phases_never_trip_a_sanitizer():
    """tests/cpp/pairing_wave_asan.cpp, its own main, -fsanitize=address,undefined -DMI_CHECK_NOWRAP on the host: one product, one line
    product, one Miller loop and one final exponentiation over a heap image of exactly MI_WAVE_IMAGE_RECORDS records"""
    pkg = os.path.join(ROOT, "gnark-whir_amd")
    subprocess.check_call(["make", "-C", pkg, "-s", "sanitize-pairing-wave"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([os.path.join(pkg, "build", "pairing_wave_asan")], capture_output=True, text=True, env=env, timeout=600)
    assert res.returncode == 0 and not res.stderr.strip(), f"rc {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-6000:]}"
    assert res.stdout.split()[-2:] == ["4", "checked"]

"""CPU suite: the key audit's table of relations (include/mi355x_groth16_keyaudit.h) in Python integers (tests/keyaudit_ref.py) over
pyref.toy_setup keys of setup_cases.toy_r1cs circuits: an honest key passes, every tamper of tests/test_gpu_keyaudit.py flips exactly
its bits, and the coefficients have to differ per index.  The library's symbols are looked up first, so that the file fails where
the audit does not exist; tests/cpp/keyaudit_host.cpp runs the host-only bookkeeping under the sanitizers."""
import copy
import os
import subprocess
import pytest
import pyref as P
import setup_cases as S
import keyaudit_ref as KR
from gpu_common import load_binding, ROOT

R = P.R_MOD
SEEDS = [bytes([s]) * 32 for s in (1, 2, 3)]


@pytest.fixture(scope="module", autouse=True)
def library_has_the_audit():
    lib = load_binding().load()
    assert hasattr(lib, "mi_key_audit") and hasattr(lib, "mi_key_claim_from_streams")


def circuit(nc, n_commitments, seed=11):   # (a seed whose A holds wires of all three classes)
    cs = P.ToyR1CS(nc, 3, seed, 0.4)
    td = P.ToyTrapdoor(seed + 40)
    r1cs = S.toy_r1cs(cs)
    r1cs["commitments"] = [([4, 6], 8), ([5], 9)][:n_commitments]
    _, exps, dom = P.toy_setup(cs, td)
    sigma = [(17 + 3 * k) % R for k in range(n_commitments)]
    key = KR.honest_key(r1cs, td.tau, td.alpha, td.beta, td.gamma, td.delta, sigma, abc=(exps["A"], exps["B"], exps["C"]))
    return cs, td, r1cs, key, KR.srs_exps(td.tau, td.alpha, td.beta, dom.n), sigma


@pytest.fixture(scope="module", params=[0, 1, 2])
def case(request):
    return circuit(5, request.param)


def test_the_model_s_own_columns_are_toy_setup_s():
    cs, td, r1cs, _, _, _ = circuit(5, 1)
    _, exps, _ = P.toy_setup(cs, td)
    assert KR.column_exps(r1cs, td.tau) == [exps["A"], exps["B"], exps["C"]]
    assert td.gamma != 1 and td.delta != 1


def test_an_honest_key_passes_for_three_seeds(case):
    _, _, r1cs, key, srs, _ = case
    for seed in SEEDS:
        assert KR.audit(r1cs, srs, key, seed) == 0


def test_every_tamper_flips_exactly_its_bits(case):
    _, _, r1cs, key, srs, _ = case
    for name, change, bits in KR.tampers(key, len(r1cs["commitments"])):
        for seed in SEEDS[:2]:
            assert KR.audit(r1cs, srs, change(key), seed) == bits, name


def test_equal_coefficients_let_a_cancelling_pair_pass(case):
    """why the coefficients are hashed per index"""
    _, _, r1cs, key, srs, _ = case
    pair = [change for name, change, _ in KR.tampers(key, 0) if name == "a cancelling pair in A"][0]
    assert KR.audit(r1cs, srs, pair(key), SEEDS[0], coeff=lambda seed, k: 7) == 0
    assert KR.audit(r1cs, srs, pair(key), SEEDS[0]) == KR.A


@pytest.mark.parametrize("cls,bits", [(KR.CLS_P, KR.A | KR.K_PRIVATE), (KR.CLS_V, KR.A | KR.K_PUBLIC), (KR.CLS_C, KR.A | KR.BASIS)])
def test_the_key_of_a_circuit_with_another_coefficient(cls, bits):
    """one coefficient of A changed at a wire of class P, V, C: A and the relation of that class (BasisExpSigma follows Basis, so SIGMA holds)"""
    cs, td, r1cs, _, srs, sigma = circuit(5, 1)
    other = copy.deepcopy(cs)
    classes = KR.wire_classes(r1cs)
    row, wire = next((i, j) for i, r in enumerate(other.rows) for j in sorted(r[0]) if classes[j] == cls)
    other.rows[row][0][wire] = (other.rows[row][0][wire] + 1) % R
    r2 = S.toy_r1cs(other); r2["commitments"] = r1cs["commitments"]
    key = KR.honest_key(r2, td.tau, td.alpha, td.beta, td.gamma, td.delta, sigma)
    assert key["inf_a"] == KR.honest_key(r1cs, td.tau, td.alpha, td.beta, td.gamma, td.delta, sigma)["inf_a"]
    assert KR.audit(r1cs, srs, key, SEEDS[0]) == bits


def test_an_srs_of_another_tau_fails_all_but_small_and_sigma():
    _, td, r1cs, key, _, _ = circuit(5, 1)
    srs = KR.srs_exps((td.tau + 1) % R, td.alpha, td.beta, 8)
    assert KR.audit(r1cs, srs, key, SEEDS[0]) == KR.ALL & ~(KR.SMALL | KR.SIGMA)


def test_coefficient_is_the_first_half_of_the_digest_little_endian():
    import hashlib
    seed = bytes(range(32))
    d = hashlib.sha256(b"mi355x-ceremony-coeff" + seed + (5).to_bytes(8, "little")).digest()
    assert KR.coefficient(seed, 5) == sum(d[i] << (8 * i) for i in range(16)) < 1 << 128


def test_host_bookkeeping_under_the_sanitizers():
    """make sanitize-keyaudit: the wire classes, the slot lists, the shape refusals and the index permutation (csrc/keyaudit_ops.cuh) as a
    CPU build with AddressSanitizer and UndefinedBehaviorSanitizer, run as a program of its own"""
    src = os.path.join(ROOT, "gnark-whir_amd")
    r = subprocess.run(["make", "-C", src, "sanitize-keyaudit"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(src, "build", "keyaudit_host_asan")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "keyaudit host: ok" in r.stdout, r.stdout + r.stderr

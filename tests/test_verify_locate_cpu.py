"""CPU suite: the locating batch verifier (include/mi355x_groth16_verify_locate.h) in the host build of its own text
(tests/emu/emu_verify_locate.cpp, -DMI_CHECK_NOWRAP: coefficients, per-proof points, both kinds of tree, column sums per node, assembly,
Miller loops, node products, judgement, the descent, the per-proof body; naive MSMs) against the verdicts and the descent computed in the
exponent (tests/verify_locate_ref.py), and the descent alone under AddressSanitizer (tests/cpp/verify_locate_asan.cpp)."""
import ctypes as C
import os
import subprocess
import pytest
import pairing_ref as R
import verify_forge as F
import verify_combine_ref as CR
import verify_locate_ref as LR
import verify_locate_cases as LC
from gpu_common import ROOT


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return C.CDLL(LC.build_emu(str(tmp_path_factory.mktemp("emu") / "libemu_verify_locate.so")))


def _run(emu, name, key, cases, inputs, seed, cap=None, crafted=False):
    """the host build against the model; every 1 or 2 against the host build's per-proof verifier alone"""
    want, want_stats = LR.model(key, cases, seed, cap)
    got, stats = LC.emu_verify_locate(emu, key["vk"], inputs, seed, cap)
    assert got == want, (name, cap)
    assert stats == want_stats, (name, cap, stats, want_stats)
    if not crafted:
        assert got == LR.expected_each(key, cases), (name, cap)
    named = [i for i, v in enumerate(got) if v in (R.PAIRING, R.PEDERSEN)]
    if named:
        alone = LC.emu_verify_each(emu, key["vk"], [inputs[i] for i in named])
        assert alone == [got[i] for i in named], (name, cap)
    return got, stats


def test_model_of_the_descent_on_the_issue_s_figures():
    """130 -> 17 -> 3 -> 1; one bad proof at 0 under the default budget: the root, then the 17 nodes of level 1, then 8 proofs alone"""
    assert LR.level_counts(130) == [130, 17, 3, 1] and LR.level_counts(1) == [1, 1] and LR.level_counts(8) == [8, 1] and LR.level_counts(9) == [9, 2, 1]
    for bad, alone in ((0, 8), (129, 2)):
        sus, st = LR.descend(130, [True] * 130, lambda l, j: bad in LR.node_range(130, l, j), 64)
        assert sus == list(LR.node_range(130, 1, bad // 8)) and len(sus) == alone and st == {"rounds": 2, "nodes_tested": 18}
    sus, st = LR.descend(130, [True] * 130, lambda l, j: 0 in LR.node_range(130, l, j), 1)
    assert sus == list(range(8)) and st == {"rounds": 3, "nodes_tested": 1 + 3 + 8}


@pytest.mark.parametrize("n", [1, 2, 8, 9, 65, 130])
def test_an_honest_batch_costs_one_node_test(emu, n):
    key, cases = LC.honest_130()
    got, stats = _run(emu, f"{n} honest", key, list(cases[:n]), list(LC.inputs_130()[:n]), CR.SEED_B)
    assert got == [R.OK] * n
    assert stats == {"rounds": 1, "nodes_tested": 1, "judged_alone": 0, "malformed": 0, "rejected": 0}


@pytest.mark.parametrize("cap", LC.CAPS)
@pytest.mark.parametrize("which", LC.BAD_POSITION_NAMES)
def test_bad_positions_of_130(emu, which, cap):
    name, key, cases, inputs = LC.bad_position_cases()[which]
    got, stats = _run(emu, name, key, cases, inputs, CR.SEED_A, cap)
    assert stats["rejected"] == sum(v != R.OK for v in LR.expected_each(key, cases)) == (1 if which in "ab" else 2)
    if cap is None and which == "a":
        assert stats["judged_alone"] == 8 and stats["nodes_tested"] == 18
    if cap is None and which == "b":
        assert stats["judged_alone"] == 2


def test_precedence_of_the_verdicts(emu):
    key, cases = LC.precedence_batch()
    got, _ = _run(emu, "precedence", key, cases, [F.verify_input(c) for c in cases], CR.SEED_A)
    assert got[2] == R.PAIRING and got[7] == R.PEDERSEN and got.count(R.OK) == 7


@pytest.mark.parametrize("shape", [(3, 1), (3, 3)])
def test_malformed_proofs_do_not_end_the_batch(emu, shape):
    key = F.forge_key(*shape)
    cases = F.distinct_batch(key, 70, 700 + shape[1])
    want = LR.expected_each(key, cases)
    assert [i for i, v in enumerate(want) if v == R.MALFORMED] == [0, 63, 69] and want[31] == R.PAIRING and want[64] == R.PEDERSEN
    for cap in (None, 1):
        got, stats = _run(emu, "70 distinct", key, cases, [F.verify_input(c) for c in cases], CR.SEED_A, cap)
        assert got == want and stats["malformed"] == 3 and stats["rejected"] == 2


def test_nodes_reuse_the_coefficients_of_the_batch(emu):
    for name, key, cases, seed, crafted in LC.crafted_batches():
        got, stats = _run(emu, name, key, cases, [F.verify_input(c) for c in cases], seed, None, crafted)
        each = LR.expected_each(key, cases)
        if len(cases) == 2:
            assert got == [R.OK, R.OK] and stats["rounds"] == 1 and R.OK not in each
        elif crafted:
            assert [got[3], got[5], got[17]] == [R.OK, R.OK, R.PAIRING] and each[3] != R.OK and each[5] != R.OK
        else:
            assert got == each and got[3] != R.OK and got[5] != R.OK and got[17] == R.PAIRING


def test_descent_under_address_sanitizer():
    """tests/cpp/verify_locate_asan.cpp, its own main, -fsanitize=address,undefined on the host: LocatePlan (csrc/pairing_ops.cuh) over
    exactly-sized heap arrays for n in {1, 2, 8, 9, 64, 65, 130, 513}, every budget in {1, 2, 8, 64}, failing sets at the first, the last
    and the lone last node, with and without malformed proofs; the suspects and the counts are checked inside the program"""
    pkg = os.path.join(ROOT, "gnark-whir_amd")
    subprocess.check_call(["make", "-C", pkg, "-s", "sanitize-locate"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([os.path.join(pkg, "build", "verify_locate_asan")], capture_output=True, text=True, env=env, timeout=300)
    assert res.returncode == 0 and not res.stderr.strip(), f"rc {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-6000:]}"
    assert int(res.stdout.split()[-1]) == 8 * 4 * 4 * 2

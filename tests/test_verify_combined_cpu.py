"""CPU suite: the combined batch verifier (include/mi355x_groth16_verify_combined.h) in the host build of its own text
(tests/emu/emu_verify_combined.cpp, -DMI_CHECK_NOWRAP: coefficients, scalar combination, scaling, assembly, Miller loops, product,
judgement; naive MSMs) against the verdict computed in the exponent (tests/verify_combine_ref.py) on the keys of verify_forge.KEY_SHAPES."""
import ctypes as C
import pytest
import pairing_ref as R
import verify_forge as F
import verify_combine_ref as CR
import verify_combined_cases as VC


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return C.CDLL(VC.build_emu(str(tmp_path_factory.mktemp("emu") / "libemu_verify_combined.so")))


def _run(emu, batches):
    bad = []
    for b in batches:
        want = CR.combined_verdict_in_exponent(b["key"], b["cases"], b["seed"])
        assert want == b["want"], b["name"]          # the list is written down, the rule computes
        got = VC.emu_verify_combined(emu, b["key"]["vk"], [F.verify_input(c) for c in b["cases"]], b["seed"])
        if got != want:
            bad.append((b["name"], got, want))
    assert not bad, bad


@pytest.mark.parametrize("n", [1, 70])
def test_coefficients_are_the_header_s_hash(emu, n):
    for seed in (CR.SEED_A, CR.SEED_B):
        rs = VC.emu_coefficients(emu, seed, n)
        assert rs == CR.coefficients(seed, n) and all(0 <= x < 1 << 128 for x in rs)
    assert VC.emu_coefficients(emu, CR.SEED_A, n) != VC.emu_coefficients(emu, CR.SEED_B, n)
    assert CR.coefficients(CR.SEED_A, 70)[0] != CR.coefficients(CR.SEED_A, 1)[0]       # n is hashed


def test_accepted_edge_cases_as_one_batch_per_key(emu):
    batches = CR.accepted_batches()
    assert {(b["key"]["nb_public"], b["key"]["n_commitments"]) for b in batches} == set(F.KEY_SHAPES)
    assert sum(len(b["cases"]) for b in batches) >= 30 and all(len(b["cases"]) >= 2 for b in batches)
    _run(emu, batches)


def test_accepted_edge_cases_alone(emu):
    _run(emu, CR.single_batches())


def test_cancelling_and_weighted_defects(emu):
    """+t and -t: each proof is rejected alone and the unweighted sum is zero -- the batch is rejected.  r_1 t and -r_0 t: accepted under
    the seed the r_i come from (that is the equation, pinned to the header's derivation), rejected under another"""
    batches = CR.cancelling_batches()
    assert [b["want"][0] for b in batches].count(R.OK) == 5 and {b["want"][0] for b in batches} == {R.OK, R.PAIRING, R.PEDERSEN}
    _run(emu, batches)


def test_distinct_batch_verdicts_and_precedence(emu):
    batches = CR.distinct_batches()
    assert [b["want"] for b in batches[:5]] == [(3, 0), (1, 67), (2, 66), (0, 65), (3, 40)]
    _run(emu, batches)

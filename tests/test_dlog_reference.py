"""CPU suite: the proof-in-the-exponent reference of tests/dlog_keys.py.

It is pinned twice: on pyref's toy circuits it must give the discrete logs the Groth16 verification equation accepts (the same equation
pyref.trapdoor_check evaluates), and on planted known-discrete-log keys at N = 2^8..2^12 the oracle's prove (oracle/groth16_ref.c)
must land on exactly g^ar, g2^bs, g^krs -- which checks the oracle itself on keys with equal and opposite points, points at infinity in
pk.G1.K, committed twins and witness values at the signed-digit edges.
"""
import os
import sys
import numpy as np
import pytest
import pyref as P
import cref
from helpers import fr_arr
import dlog_keys as D

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import wire_census  # noqa: E402

CENSUS_MASKS = wire_census.census_masks_permille()


def _toy_exps(cs, td, pk, exps):
    return {"log_n": pk["log_n"], "nb_wires": cs.nb_wires, "nb_public": cs.nb_public,
            "alpha": fr_arr([td.alpha])[0], "beta": fr_arr([td.beta])[0], "delta": fr_arr([td.delta])[0], "tau": fr_arr([td.tau])[0],
            "A": fr_arr(exps["A"]), "B": fr_arr(exps["B"]), "K": fr_arr(exps["K"]),
            "infinity_a": np.array(pk["inf_a"], np.uint8), "infinity_b": np.array(pk["inf_b"], np.uint8),
            "committed": np.zeros(0, np.int64), "plants": None, "seed": 0}


@pytest.mark.parametrize("nc,npub,seed", [(13, 3, 21), (64, 5, 22), (200, 9, 23)])
def test_reference_satisfies_the_groth16_equation_on_toy_circuits(nc, npub, seed):
    """pyref toy circuit with its trapdoor: the reference's (ar, bs, krs) satisfy ar bs = alpha beta + sum_pub W_j (beta A_j + alpha B_j
    + C_j) + krs delta, and are the discrete logs of pyref's own toy proof (which trapdoor_check accepts)"""
    cs = P.ToyR1CS(nc, npub, seed)
    td = P.ToyTrapdoor(seed)
    pk, exps, dom = P.toy_setup(cs, td)
    w, a, b, c = cs.solve()
    r, s = 0x1234567 + seed, 0x89ABCDEF + seed
    e = _toy_exps(cs, td, pk, exps)
    ar, bs, krs = D.expected_proof_exps(e, fr_arr(w), fr_arr(a), fr_arr(b), fr_arr([r])[0], fr_arr([s])[0])
    R = P.R_MOD
    pub = sum(w[j] * (td.beta * exps["A"][j] + td.alpha * exps["B"][j] + exps["C"][j]) for j in range(cs.nb_public)) % R
    assert (ar * bs - td.alpha * td.beta - pub - krs * td.delta) % R == 0
    proof = P.toy_prove(cs, pk, dom, r, s)
    assert P.trapdoor_check(cs, td, exps, proof, r, s)
    assert proof["ar"] == P.g1_mul(P.G1_GEN, ar) and proof["bs"] == P.g2_mul(P.G2_GEN, bs) and proof["krs"] == P.g1_mul(P.G1_GEN, krs)


def test_reference_vector_helpers():
    """the product-tree inversion, the powers and the bit-reversal against plain integer arithmetic"""
    x = cref.gen_scalars(37, 5, 0)
    inv = D.batch_inv(x)
    xs, ys = D.fr_vals(x), D.fr_vals(inv)
    assert all(a * b % P.R_MOD == 1 for a, b in zip(xs, ys))
    g = fr_arr([7])[0]
    assert D.fr_vals(D.powers(g, 19)) == [pow(7, i, P.R_MOD) for i in range(19)]
    assert D.fr_vals(D.fr_sum(x).reshape(1, 4))[0] == sum(xs) % P.R_MOD
    assert list(D.bitrev_index(5)) == [P.bitrev(i, 5) for i in range(32)]


def test_edge_values_recode_to_the_edge_digits():
    """the planted W values really sit on the signed-digit edges: every c in EDGE_WIDTHS has a value all of whose low digits are -2^(c-1)"""
    vals = set(D.edge_values())
    assert {0, 1, P.R_MOD - 1} <= vals and all(0 <= v < P.R_MOD for v in vals)
    for c in D.EDGE_WIDTHS:
        def digits(v):
            out, carry = [], 0
            for w in range((256 + c - 1) // c):
                d = ((v >> (w * c)) & ((1 << c) - 1)) + carry
                carry = int(d >= 1 << (c - 1))
                out.append(d - (carry << c))
            return out
        m = 253 // c
        assert any(digits(v)[:m] == [-(1 << (c - 1))] * m for v in vals), c
        assert any(digits(v)[:m] == [(1 << (c - 1)) - 1] * m for v in vals), c


def _case(log_n, masks, seed):
    N = 1 << log_n
    nb_public = 1 + (N >> 6)
    e = D.make_exps(log_n, N - 7, nb_public, N >> 5, masks, True, seed)
    W = D.witness(e, 1, seed + 10)
    a, b, c = D.constraint_values(N - 3, 1, seed + 20)
    r, s = cref.gen_scalars(2, seed + 30, 0)
    return e, W, a, b, c, r, s


def test_plants_are_what_the_docstring_says():
    e, W, *_ = _case(12, CENSUS_MASKS, 5)
    pl = e["plants"]
    K, A = e["K"], e["A"]
    assert len(pl["unused"]) >= 200 and not K[pl["unused"]].any() and W[pl["unused"]].any(axis=1).all()
    assert e["infinity_a"][pl["unused"]].all() and e["infinity_b"][pl["unused"]].all()
    assert not np.isin(pl["unused"], e["committed"]).any()
    assert max(n for _, n, _ in pl["runs"]) >= 100 and any(ng for _, _, ng in pl["runs"])
    d, s, ng = pl["dst"], pl["src"], pl["neg"]
    assert np.array_equal(W[d], W[s]) and np.array_equal(A[d[~ng]], A[s[~ng]]) and np.array_equal(A[d[ng]], D.neg(A[s[ng]]))
    assert (W[pl["w_one"]] == D.ONE).all()
    com = np.isin(d, e["committed"]) != np.isin(s, e["committed"])
    assert com.sum() == pl["committed_pairs"] >= 2 and len(e["committed"]) == (1 << 12) >> 5
    assert np.array_equal(W[0], D.ONE)
    # outside the planted wires the masks are the census's
    rest = np.ones(e["nb_wires"], bool)
    rest[np.concatenate([d, s, pl["unused"], pl["edge"]])] = False
    assert abs(1000 * (e["infinity_a"][rest] == 0).mean() - CENSUS_MASKS[0]) < 50
    assert abs(1000 * (e["infinity_b"][rest] == 0).mean() - CENSUS_MASKS[1]) < 50


@pytest.mark.parametrize("masks", [(900, 500), CENSUS_MASKS], ids=["bench-masks", "census-masks"])
@pytest.mark.parametrize("log_n", [8, 10, 12])
def test_oracle_prove_equals_the_exponent_reference(log_n, masks):
    """cref.prove on a planted known-discrete-log key (copies, negations, infinity K points, committed twins, edge witness values):
    Ar, Bs, Krs are g^ar, g2^bs, g^krs of the exponent reference"""
    e, W, a, b, c, r, s = _case(log_n, masks, 100 + log_n)
    pk = D.points_from_exps(e)
    assert not pk["g1_k"][np.searchsorted(D.k_rows(e), e["plants"]["unused"])].any(), "unused wires are (0, 0) in pk.G1.K"
    proof = cref.prove(pk, W, a, b, c, r, s)
    D.check_proof(proof, D.expected_proof_exps(e, W, a, b, r, s))


def test_chunked_reference_equals_whole_vectors():
    """the chunked forms (what the 2^27 proof uses) equal the whole-vector ones: Z in stored order, and the proof's exponents with
    chunks that do not divide the wire or constraint counts"""
    e = D.make_exps(10, 1000, 17, 32, (900, 500), True, 77)
    for cb in (3, 7, 10, 22):
        assert np.array_equal(D.z_exps_bitrev(e, chunk_bits=cb), D.z_exps(e)[D.bitrev_index(10)])
    W = D.witness(e, 1, 78)
    a, b, _ = D.constraint_values(900, 1, 79)
    r, s = cref.gen_scalars(2, 80, 0)
    want = D.expected_proof_exps(e, W, a, b, r, s, chunk=1 << 20)
    assert D.expected_proof_exps(e, W, a, b, r, s, chunk=37) == want
    assert D.expected_proof_exps(e, W, a, b, r, s, chunk=256) == want

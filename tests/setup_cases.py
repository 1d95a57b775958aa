"""Inputs and host references for the device Setup (include/mi355x_groth16_setup.h), shared by tests/test_gpu_setup.py and
tools/setup_probe.py.  Nothing here calls the code under test: the references run on cref.field_op (the oracle's Montgomery Fr, OpenMP)
through the vector helpers of tests/dlog_keys.py, and on Python integers.

An R1CS is the dict gnark_whir_amd binding.Context.setup takes: n_constraints, nb_wires, nb_public, A / B / C = (row_ptr, col, coeff) in
CSR, coeffs (n, 4) Montgomery rows, commitments = [(committed wires, commitment wire)].
"""
import numpy as np
import pyref as P
import cref
import dlog_keys as D
from helpers import fr_arr, fr_vals

ADD, SUB, MUL, INV = 0, 1, 2, 3
_op, _bc, _int = D._op, D._bc, D._int


# ---------------------------------------------------------------------------------------------------- pyref's toy circuits as CSR
def toy_r1cs(cs):
    """pyref.ToyR1CS -> R1CS dict; the coefficients are interned in order of first use"""
    table, mats = {}, []
    for k in range(3):
        rp, col, cf = [0], [], []
        for row in cs.rows:
            for j, v in row[k].items():
                col.append(j); cf.append(table.setdefault(v % P.R_MOD, len(table)))
            rp.append(len(col))
        mats.append((np.array(rp, np.uint64), np.array(col, np.uint32), np.array(cf, np.uint32)))
    coeffs = fr_arr(sorted(table, key=table.get)) if table else np.zeros((0, 4), np.uint64)
    return {"n_constraints": cs.nb_constraints, "nb_wires": cs.nb_wires, "nb_public": cs.nb_public, "A": mats[0], "B": mats[1], "C": mats[2],
            "coeffs": coeffs, "commitments": []}


def toy_trapdoor(td):
    return {n: fr_arr([getattr(td, n)])[0] for n in ("tau", "alpha", "beta", "gamma", "delta")}


# ---------------------------------------------------------------------------------------------------- seeded synthetic R1CS
def synth_r1cs(n_constraints, nb_wires, nb_public, seed, per_row=4, n_coeffs=1 << 16, n_heavy=0, heavy_len=1 << 10, skew=True,
               n_empty_cols=64, commitments=0, n_committed=0):
    """A fixed number of entries per live row (so the reference vectorises) in each of A, B, C; about 3 % of the rows are empty.
    skew: wire `hot` (the last public wire) sits in every live row of A, wire 0 in every second live row of B; n_heavy private wires own
    heavy_len entries each, spread over the three matrices; every eighth row of each matrix repeats a column (duplicates add up); the last
    n_empty_cols wires are in no constraint.  Keeps the dense (rows, per_row) form under "dense" for the reference."""
    rng = np.random.default_rng(seed)
    live = rng.random(n_constraints) >= 0.03
    rows = np.nonzero(live)[0]
    nl = len(rows)
    used = nb_wires - n_empty_cols
    assert used > nb_public + n_heavy + 8 and per_row >= 3
    hot = nb_public - 1
    heavy = nb_public + np.arange(n_heavy)
    dense = {}
    for k, name in enumerate("ABC"):
        col = rng.integers(0, used, (nl, per_row), dtype=np.uint32)
        cf = rng.integers(0, n_coeffs, (nl, per_row), dtype=np.uint32)
        if n_heavy:
            share = heavy_len // 3 + (k < heavy_len % 3)
            pos = rng.choice(nl * (per_row - 2), n_heavy * share, replace=False)     # slots 2.. of the rows: 0 and 1 carry the skew
            col[pos // (per_row - 2), 2 + pos % (per_row - 2)] = np.repeat(heavy, share).astype(np.uint32)
        if skew and name == "A":
            col[:, 0] = hot
        if skew and name == "B":
            col[0::2, 1] = 0
        col[0::8, per_row - 1] = col[0::8, per_row - 2]
        dense[name] = (col, cf)
    mats = {}
    rp = np.zeros(n_constraints + 1, np.uint64)
    rp[1:] = np.cumsum(live.astype(np.uint64) * np.uint64(per_row))
    for name in "ABC":
        mats[name] = (rp, np.ascontiguousarray(dense[name][0].reshape(-1)), np.ascontiguousarray(dense[name][1].reshape(-1)))
    coeffs = cref.gen_scalars(n_coeffs, seed + 7, 0)
    coeffs[0] = D.ONE   # coefficient 1 is the common one in a real table
    com = []
    if commitments:
        pool = rng.choice(np.arange(nb_public + n_heavy, used), commitments * (n_committed + 1), replace=False).astype(np.uint32)
        for c in range(commitments):
            part = pool[c * (n_committed + 1):(c + 1) * (n_committed + 1)]
            com.append((np.ascontiguousarray(part[1:]), int(part[0])))
    return {"n_constraints": n_constraints, "nb_wires": nb_wires, "nb_public": nb_public, "A": mats["A"], "B": mats["B"], "C": mats["C"],
            "coeffs": coeffs, "commitments": com, "dense": dense, "live_rows": rows, "hot": hot, "heavy": heavy, "per_row": per_row}


def synth_trapdoor(seed, n_sigma=0):
    v = cref.gen_scalars(5 + n_sigma, seed, 0)
    td = {n: v[i] for i, n in enumerate(("tau", "alpha", "beta", "gamma", "delta"))}
    td["sigma"] = [v[5 + k] for k in range(n_sigma)]
    return td


# ---------------------------------------------------------------------------------------------------- the reference
def lagrange_rows(n_constraints, tau):
    """L_i(tau) = (tau^N - 1) / N * w^i / (tau - w^i) for i < n_constraints, Montgomery rows; tau a Montgomery row"""
    dom = P.Domain(n_constraints)
    lam = (pow(_int(tau), dom.n, P.R_MOD) - 1) * dom.card_inv % P.R_MOD
    wp = D.powers(fr_arr([dom.gen])[0], n_constraints)
    lw = _op(MUL, wp, D.batch_inv(_op(SUB, _bc(tau, n_constraints), wp)))
    return _op(MUL, lw, _bc(fr_arr([lam])[0], n_constraints)), dom


def check_identity(r1cs, name, L, got, rho):
    """sum_j rho_j M_j == sum_i L_i (M rho)_i for the matrix `name` of a synth_r1cs"""
    col, cf = r1cs["dense"][name]
    acc = np.zeros((col.shape[0], 4), np.uint64)
    for k in range(col.shape[1]):
        acc = _op(ADD, acc, _op(MUL, r1cs["coeffs"][cf[:, k]], rho[col[:, k]]))
    rhs = D.fr_dot(acc, L[r1cs["live_rows"]])
    lhs = D.fr_dot(rho, got)
    assert _int(lhs) == _int(rhs), f"matrix {name}: sum_j rho_j M_j differs from sum_i L_i (M rho)_i"


def column_by_integers(r1cs, name, L, j):
    """M_j entry by entry in Python integers"""
    rp, col, cf = r1cs[name]
    e = np.nonzero(col == np.uint32(j))[0]
    if not len(e):
        return 0
    rows = np.searchsorted(rp, e.astype(np.uint64), side="right") - 1
    # Montgomery rows as Python integers (object arrays): sum (a R)(b R) = R^2 sum a b
    total = int((_mont_ints(L[rows]) * _mont_ints(r1cs["coeffs"][cf[e]])).sum())
    return total * _R_INV * _R_INV % P.R_MOD


_R_INV = pow(1 << 256, -1, P.R_MOD)


def _mont_ints(rows):
    r = np.asarray(rows, np.uint64).astype(object)
    return r[:, 0] | (r[:, 1] << 64) | (r[:, 2] << 128) | (r[:, 3] << 192)


def sample_wires(r1cs, seed, n=64):
    """at least n wires to recompute exactly: the heaviest column of each matrix, the skewed and heavy ones, the ends, empty columns, random"""
    rng = np.random.default_rng(seed)
    nw = r1cs["nb_wires"]
    pick = [0, 1, nw - 1, nw - 2, r1cs.get("hot", 0)]
    for name in "ABC":
        pick.append(int(np.argmax(np.bincount(r1cs[name][1], minlength=nw))))
    pick += [int(x) for x in r1cs.get("heavy", [])[:4]]
    pick += [int(x) for x in rng.integers(0, nw, n)]
    return sorted(set(pick))


def check_exponents(r1cs, td, got, seed, wires=None):
    """checks (a), (b), (c) of a synthetic R1CS's device exponents `got` (setup_exponents' dict); returns L"""
    nw = r1cs["nb_wires"]
    L, dom = lagrange_rows(r1cs["n_constraints"], td["tau"])
    rho = cref.gen_scalars(nw, seed + 99, 0)
    for name, key in (("A", "a"), ("B", "b"), ("C", "c")):
        check_identity(r1cs, name, L, got[key], rho)
    R = P.R_MOD
    al, be, ga, de = (_int(td[k]) for k in ("alpha", "beta", "gamma", "delta"))
    for j in (sample_wires(r1cs, seed) if wires is None else wires):
        want = [column_by_integers(r1cs, name, L, j) for name in "ABC"]
        have = [_int(got[key][j]) for key in ("a", "b", "c")]
        assert have == want, f"wire {j}: A_j, B_j, C_j differ from the entry-by-entry sums"
        t = (be * want[0] + al * want[1] + want[2]) % R
        assert _int(got["k"][j]) == t * P.fr_inv(de) % R and _int(got["k_gamma"][j]) == t * P.fr_inv(ga) % R, f"wire {j}: t_j / delta or t_j / gamma"
    # the element-wise part on every wire, vectorised
    t = _op(ADD, _op(ADD, _op(MUL, got["a"], _bc(td["beta"], nw)), _op(MUL, got["b"], _bc(td["alpha"], nw))), got["c"])
    assert np.array_equal(got["k"], _op(MUL, t, _bc(fr_arr([P.fr_inv(de)])[0], nw))), "K is not t / delta"
    assert np.array_equal(got["k_gamma"], _op(MUL, t, _bc(fr_arr([P.fr_inv(ga)])[0], nw))), "k_gamma is not t / gamma"
    # (c) masks follow the exponents; a column without entries is at infinity
    assert np.array_equal(got["infinity_a"], (~got["a"].any(axis=1)).astype(np.uint8)), "infinity_a"
    assert np.array_equal(got["infinity_b"], (~got["b"].any(axis=1)).astype(np.uint8)), "infinity_b"
    for name, key in (("A", "infinity_a"), ("B", "infinity_b")):
        empty = np.bincount(r1cs[name][1], minlength=nw) == 0
        assert empty.any() and got[key][empty].all(), f"an empty column of {name} is not at infinity"
    return L, dom


def check_z(td, log_n, z):
    """the Z exponents in stored order against dlog_keys.z_exps_bitrev"""
    want = D.z_exps_bitrev({"log_n": log_n, "tau": td["tau"], "delta": td["delta"]})
    assert np.array_equal(z, want), "Z exponents"


def dlog_exps(r1cs, td, got, log_n):
    """setup_exponents' output as the `exps` dict of tests/dlog_keys.py (expected_proof_exps, k_rows)"""
    removed = sorted(int(w) for ws, c in r1cs["commitments"] for w in list(ws) + [c])
    return {"log_n": log_n, "nb_wires": r1cs["nb_wires"], "nb_public": r1cs["nb_public"], "alpha": td["alpha"], "beta": td["beta"],
            "delta": td["delta"], "tau": td["tau"], "A": got["a"], "B": got["b"], "K": got["k"], "infinity_a": got["infinity_a"],
            "infinity_b": got["infinity_b"], "committed": np.array(removed, np.int64), "plants": None, "seed": 0}

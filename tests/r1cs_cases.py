"""Inputs and host references for the device-resident R1CS (include/mi355x_groth16_r1cs.h), shared by tests/test_r1cs_abi.py,
tests/test_gpu_r1cs.py and tools/r1cs_probe.py.  Nothing here calls the code under test: the row-wise product runs on cref.field_op
(the oracle's Montgomery Fr) through the vector helpers of tests/dlog_keys.py, and on Python integers.

An R1CS is the dict of tests/setup_cases.py (what binding.Context.setup and r1cs_load take).
"""
import numpy as np
import pyref as P
import cref
import dlog_keys as D
import setup_cases as S
from helpers import fr_arr

ADD, SUB, MUL = 0, 1, 2
_op = D._op
U64_MAX = (1 << 64) - 1
# what the library documents: a row of more than SHORT entries is cut into pieces of CHUNK entries
SHORT, CHUNK = 16, 512
LONG_LENS = (16, 17, 64, 511, 512, 513, 5000, 100_003)
REF_DENSE = 64      # the reference's own split, unrelated to the device's: rows up to this length are summed slot by slot over all rows


# ---------------------------------------------------------------------------------------------------- the generator
def skewed_r1cs(n_constraints, nb_wires, nb_public, seed, long_lens=LONG_LENS, n_coeffs=4096, commitments=0, n_committed=0):
    """Row lengths 0..4 (a tenth of the rows empty) in each of A, B, C, with one row of every length in long_lens planted per matrix;
    every eighth row of two or more entries repeats its first column in its last slot (duplicates add up).  The coefficient table starts
    0, 1, -1, 2, r - 1 (the last two spellings of one value: two table slots), the rest is random; 60 % of the entries take one of the
    five.  Keeps the row lengths under "lens" and the planted rows under "long_at"."""
    rng = np.random.default_rng(seed)
    mats, lens_of, long_at = {}, {}, {}
    for name in "ABC":
        lens = rng.choice(5, n_constraints, p=[.10, .35, .30, .15, .10]).astype(np.int64)
        rows = rng.choice(n_constraints, len(long_lens), replace=False)
        lens[rows] = long_lens
        rp = np.zeros(n_constraints + 1, np.uint64)
        rp[1:] = np.cumsum(lens).astype(np.uint64)
        nnz = int(rp[-1])
        col = rng.integers(0, nb_wires, nnz, dtype=np.uint32)
        dup = np.nonzero(lens >= 2)[0][::8]
        col[rp[dup + 1].astype(np.int64) - 1] = col[rp[dup].astype(np.int64)]
        cf = np.where(rng.random(nnz) < 0.6, rng.integers(0, 5, nnz), rng.integers(5, n_coeffs, nnz)).astype(np.uint32)
        mats[name], lens_of[name], long_at[name] = (rp, col, cf), lens, dict(zip(long_lens, (int(x) for x in rows)))
    coeffs = cref.gen_scalars(n_coeffs, seed + 7, 0)
    coeffs[:5] = fr_arr([0, 1, -1, 2, P.R_MOD - 1])
    com = []
    if commitments:
        pool = rng.choice(np.arange(nb_public, nb_wires), commitments * (n_committed + 1), replace=False).astype(np.uint32)
        for c in range(commitments):
            part = pool[c * (n_committed + 1):(c + 1) * (n_committed + 1)]
            com.append((np.ascontiguousarray(part[1:]), int(part[0])))
    return {"n_constraints": n_constraints, "nb_wires": nb_wires, "nb_public": nb_public, "A": mats["A"], "B": mats["B"], "C": mats["C"],
            "coeffs": coeffs, "commitments": com, "lens": lens_of, "long_at": long_at}


def witness(nb_wires, seed):
    """wire values of the WHIR mix with the constant wire 1 and dlog_keys.edge_values() planted at random places"""
    W = cref.gen_scalars(nb_wires, seed, 1)
    edge = fr_arr(D.edge_values())
    pos = np.random.default_rng(seed).choice(np.arange(1, nb_wires), len(edge), replace=False)
    W[pos] = edge
    W[0] = D.ONE
    return W


def split_counts(r1cs, names="ABC"):
    """(rows longer than SHORT, pieces of CHUNK entries they are cut into) over the matrices in names"""
    n_long = n_pieces = 0
    for name in names:
        rp = np.asarray(r1cs[name][0], np.uint64).astype(np.int64)
        lens = rp[1:] - rp[:-1]
        big = lens[lens > SHORT]
        n_long += len(big); n_pieces += int(((big + CHUNK - 1) // CHUNK).sum())
    return n_long, n_pieces


# ---------------------------------------------------------------------------------------------------- the reference
def eval_rows(r1cs, name, W):
    """(M W)[i] = sum_e coeffs[coeff[e]] W[col[e]] over the entries of row i, for the matrix `name`: (n_constraints, 4) Montgomery rows.
    One vector multiplication over all entries; rows of up to REF_DENSE entries are then added slot by slot over all rows at once (the
    dense form), longer ones by dlog_keys.fr_sum."""
    rp, col, cf = r1cs[name]
    rp = np.asarray(rp, np.uint64).astype(np.int64)
    n = len(rp) - 1
    out = np.zeros((n, 4), np.uint64)
    if rp[-1] == 0:
        return out
    prod = _op(MUL, np.ascontiguousarray(r1cs["coeffs"][np.asarray(cf, np.int64)]), np.ascontiguousarray(W[np.asarray(col, np.int64)]))
    lens = rp[1:] - rp[:-1]
    dense = lens <= REF_DENSE
    for k in range(int(lens[dense].max(initial=0))):
        sel = np.nonzero(dense & (lens > k))[0]
        out[sel] = _op(ADD, np.ascontiguousarray(out[sel]), np.ascontiguousarray(prod[rp[sel] + k]))
    for i in np.nonzero(~dense)[0]:
        out[i] = D.fr_sum(prod[rp[i]:rp[i + 1]])
    return out


def eval_all(r1cs, W):
    return tuple(eval_rows(r1cs, name, W) for name in "ABC")


def row_by_integers(r1cs, name, W, i):
    """(M W)[i] entry by entry in Python integers (canonical value)"""
    rp, col, cf = r1cs[name]
    lo, hi = int(rp[i]), int(rp[i + 1])
    if lo == hi:
        return 0
    # Montgomery rows as Python integers (object arrays): sum (a R)(b R) = R^2 sum a b
    total = int((S._mont_ints(r1cs["coeffs"][np.asarray(cf[lo:hi], np.int64)]) * S._mont_ints(W[np.asarray(col[lo:hi], np.int64)])).sum())
    return total * S._R_INV * S._R_INV % P.R_MOD


def check_rows(a, b, c):
    """(rows with a b != c, the lowest of them or 2^64 - 1) of three (n, 4) Montgomery arrays"""
    bad = np.nonzero((_op(MUL, a, b) != c).any(axis=1))[0]
    return len(bad), (int(bad[0]) if len(bad) else U64_MAX)


def r1cs_bytes(r1cs):
    """device bytes of a resident R1CS by DESIGN.md 4c's formula: per matrix 8 B per entry and 4 B per row offset, 16 B per long row
    and 8 B per piece of its plan; the coefficient table once"""
    total = 32 * len(r1cs["coeffs"])
    for name in "ABC":
        rp = np.asarray(r1cs[name][0], np.uint64)
        n_long, n_pieces = split_counts(r1cs, name)
        total += 8 * int(rp[-1]) + 4 * len(rp) + 16 * n_long + 8 * n_pieces
    return total


def solved_r1cs(n_constraints, nb_wires_ab, nb_public, seed, commitments=0, n_committed=0):
    """A skewed R1CS that HAS a solution: A and B as skewed_r1cs over the first nb_wires_ab wires; row i of C is the single entry
    1 * wire (nb_wires_ab + i), and that wire's value is (A W)_i (B W)_i.  Returns (r1cs, W, a, b, c)."""
    r1cs = skewed_r1cs(n_constraints, nb_wires_ab, nb_public, seed, commitments=commitments, n_committed=n_committed)
    r1cs["nb_wires"] = nb_wires_ab + n_constraints
    r1cs["C"] = (np.arange(n_constraints + 1, dtype=np.uint64), (nb_wires_ab + np.arange(n_constraints)).astype(np.uint32),
                 np.ones(n_constraints, np.uint32))          # coefficient table slot 1 holds 1
    r1cs["lens"]["C"] = np.ones(n_constraints, np.int64)
    W = np.zeros((r1cs["nb_wires"], 4), np.uint64)
    W[:nb_wires_ab] = witness(nb_wires_ab, seed + 1)
    a, b = eval_rows(r1cs, "A", W), eval_rows(r1cs, "B", W)
    c = _op(MUL, a, b)
    W[nb_wires_ab:] = c
    return r1cs, W, a, b, c

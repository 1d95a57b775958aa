"""Inputs and host references for the device-resident R1CS (include/mi355x_groth16_r1cs.h), shared by tests/test_r1cs_abi.py,
tests/test_gpu_r1cs.py, tests/sparse_cases.py (the cases of tests/test_gpu_sparse_sums.py) and tools/r1cs_probe.py.  Nothing here calls the code under test: the row-wise product runs on cref.field_op
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


ROW_LEN_P = [.10, .35, .30, .15, .10]      # the share of rows with 0, 1, 2, 3, 4 entries
HEAVY, ONE, NONE = "heavy", "one", "none"


def _csr_of_lens(lens):
    rp = np.zeros(len(lens) + 1, np.uint64)
    rp[1:] = np.cumsum(lens).astype(np.uint64)
    return rp


def many_long_r1cs(n_long, roles=(HEAVY, ONE, NONE), n_constraints=None, nb_wires=4096, nb_public=33, seed=0, n_double=40, one_len=1025,
                   coeffs=None, shares=None):
    """Row lengths 0..4 as in skewed_r1cs.  A matrix whose role is HEAVY also has n_long rows of exactly SHORT + 1 = 17 entries (one piece
    each) and n_double rows of CHUNK + 1 = 513 (two pieces each): n_long + n_double long rows, n_long + 2 n_double pieces.  A matrix whose
    role is ONE has exactly one long row, of one_len entries; one whose role is NONE has none.  roles names the role of A, B, C.
    coeffs: the coefficient table (Montgomery rows) with shares, the probability of each of its slots; without them the table and the
    mix of skewed_r1cs.  The planted rows are kept as arrays under "planted": name -> (rows, their lengths), in the order planted."""
    rng = np.random.default_rng(seed)
    nc = n_long + n_double + 600 if n_constraints is None else n_constraints
    assert nc >= n_long + n_double and len(roles) == 3 and set(roles) <= {HEAVY, ONE, NONE}
    if coeffs is None:
        n_coeffs = 4096
        coeffs = cref.gen_scalars(n_coeffs, seed + 7, 0)
        coeffs[:5] = fr_arr([0, 1, -1, 2, P.R_MOD - 1])
    else:
        n_coeffs = len(coeffs)
        assert shares is not None and len(shares) == n_coeffs
    mats, lens_of, planted = {}, {}, {}
    for name, role in zip("ABC", roles):
        lens = rng.choice(5, nc, p=ROW_LEN_P).astype(np.int64)
        if role == HEAVY:
            rows = rng.choice(nc, n_long + n_double, replace=False).astype(np.int64)
            want = np.concatenate([np.full(n_long, SHORT + 1, np.int64), np.full(n_double, CHUNK + 1, np.int64)])
        elif role == ONE:
            rows, want = rng.choice(nc, 1).astype(np.int64), np.array([one_len], np.int64)
        else:
            rows, want = np.zeros(0, np.int64), np.zeros(0, np.int64)
        lens[rows] = want
        rp = _csr_of_lens(lens)
        nnz = int(rp[-1])
        col = rng.integers(0, nb_wires, nnz, dtype=np.uint32)
        if shares is None:
            cf = np.where(rng.random(nnz) < 0.6, rng.integers(0, 5, nnz), rng.integers(5, n_coeffs, nnz)).astype(np.uint32)
        else:
            cf = rng.choice(n_coeffs, nnz, p=shares).astype(np.uint32)
        mats[name], lens_of[name], planted[name] = (rp, col, cf), lens, (rows, want)
    return {"n_constraints": nc, "nb_wires": nb_wires, "nb_public": nb_public, "A": mats["A"], "B": mats["B"], "C": mats["C"],
            "coeffs": coeffs, "commitments": [], "lens": lens_of, "planted": planted, "roles": tuple(roles)}


def transposed(r1cs):
    """the R1CS whose matrices are the transposes of r1cs's: rows become columns, by a stable argsort of col"""
    nc, nw = r1cs["n_constraints"], r1cs["nb_wires"]
    out = {"n_constraints": nw, "nb_wires": nc, "nb_public": r1cs["nb_public"], "coeffs": r1cs["coeffs"], "commitments": []}
    for name in "ABC":
        rp, col, cf = r1cs[name]
        rp = np.asarray(rp, np.uint64).astype(np.int64)
        row_of = np.repeat(np.arange(nc, dtype=np.uint32), rp[1:] - rp[:-1])
        order = np.argsort(col, kind="stable")
        trp = np.zeros(nw + 1, np.uint64)
        trp[1:] = np.cumsum(np.bincount(col, minlength=nw)).astype(np.uint64)
        out[name] = (trp, np.ascontiguousarray(row_of[order]), np.ascontiguousarray(cf[order]))
    return out


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


def check_columns(r1cs, td, got, wires_of, seed):
    """Setup's A_j, B_j, C_j (setup_exponents' dict `got`) for an R1CS without a dense form: the wires of wires_of[name] entry by entry in
    Python integers (setup_cases.column_by_integers), and the whole vector by sum_j rho_j M_j == sum_i L_i (M rho)_i for a random rho,
    the right side through eval_rows."""
    nw = r1cs["nb_wires"]
    L, _ = S.lagrange_rows(r1cs["n_constraints"], td["tau"])
    rho = cref.gen_scalars(nw, seed, 0)
    for name, key in (("A", "a"), ("B", "b"), ("C", "c")):
        lens = np.bincount(r1cs[name][1], minlength=nw)
        for j in sorted(int(x) for x in wires_of[name]):
            assert S._int(got[key][j]) == S.column_by_integers(r1cs, name, L, j), f"{name}_{j} ({lens[j]} entries)"
        lhs, rhs = D.fr_dot(rho, got[key]), D.fr_dot(eval_rows(r1cs, name, rho), L)
        assert S._int(lhs) == S._int(rhs), f"matrix {name}: sum_j rho_j M_j differs from sum_i L_i (M rho)_i"


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


def satisfied_r1cs_long_c(n_constraints=1061, nb_wires_ab=700, nb_public=9, seed=0, n_coeffs=512):
    """An R1CS that HAS a solution and whose A, B AND C carry long rows.  A and B are rows of 0..4 entries over the first nb_wires_ab
    wires; row i of C is 0..4 such entries and then 1 * slack_i, the wire nb_wires_ab + i, which occurs nowhere else, with
    W[slack_i] = (A W)_i (B W)_i - (the rest of C's row i): adding 1 to W[slack_i] makes row i, and only row i, bad.  Long rows
    (the length counts C's slack entry), with m = n_constraints // 2 and n = n_constraints - 1:
        A   row 0: 513, row 1: 17, row n: 1025        adjacent rows, the first and the last
        B   row n: 512                                 one long row
        C   row 0: 17, row m: 1025, row n: 512         first, middle, last; row n is long in all three
    One more wire, the last, occurs exactly once in the whole system: as entry 1024 of A's row n, the only entry of that row's third
    piece.  Returns (r1cs, W, a, b, c); the r1cs keeps "long_at" (name -> {row: length}), "slack0" (= nb_wires_ab) and
    "once" = (the wire, its row)."""
    rng = np.random.default_rng(seed)
    nc, nab = n_constraints, nb_wires_ab
    mid, last = nc // 2, nc - 1
    long_at = {"A": {0: CHUNK + 1, 1: SHORT + 1, last: 2 * CHUNK + 1}, "B": {last: CHUNK}, "C": {0: SHORT + 1, mid: 2 * CHUNK + 1, last: CHUNK}}
    once = nab + nc
    coeffs = cref.gen_scalars(n_coeffs, seed + 7, 0)
    coeffs[:5] = fr_arr([0, 1, -1, 2, P.R_MOD - 1])
    mats, lens_of = {}, {}
    for name in "ABC":
        lens = rng.choice(5, nc, p=ROW_LEN_P).astype(np.int64) + (name == "C")
        for row, n in long_at[name].items():
            lens[row] = n
        rp = _csr_of_lens(lens)
        nnz = int(rp[-1])
        col = rng.integers(0, nab, nnz, dtype=np.uint32)
        cf = np.where(rng.random(nnz) < 0.6, rng.integers(0, 5, nnz), rng.integers(5, n_coeffs, nnz)).astype(np.uint32)
        ends = rp[1:].astype(np.int64) - 1
        if name == "C":
            col[ends] = (nab + np.arange(nc)).astype(np.uint32)
            cf[ends] = 1                                        # coefficient table slot 1 holds 1
        if name == "A":
            col[ends[last]] = once
            cf[ends[last]] = 5                                  # a random value, not 0
        mats[name], lens_of[name] = (rp, col, cf), lens
    r1cs = {"n_constraints": nc, "nb_wires": once + 1, "nb_public": nb_public, "A": mats["A"], "B": mats["B"], "C": mats["C"],
            "coeffs": coeffs, "commitments": [], "lens": lens_of, "long_at": long_at, "slack0": nab, "once": (once, last)}
    W = np.zeros((once + 1, 4), np.uint64)
    W[:nab] = witness(nab, seed + 1)
    W[once] = cref.gen_scalars(1, seed + 2, 0)[0]
    a, b = eval_rows(r1cs, "A", W), eval_rows(r1cs, "B", W)
    c = _op(MUL, a, b)
    W[nab:once] = _op(SUB, c, eval_rows(r1cs, "C", W))          # the slack wires are still 0 here
    return r1cs, W, a, b, c


def with_slack(r1cs, W):
    """Any R1CS made solvable: one wire more per row, slack_i = nb_wires + i, appended to row i of C with coefficient 1 (a table slot of
    its own, the last), and W extended by W[slack_i] = (A W)_i (B W)_i - (C W)_i.  Every row of C grows by one entry: a row of 17 stays
    one piece, one of 513 two.  Returns (r1cs', W', a, b, c); "slack0" is the first slack wire."""
    nc, nw = r1cs["n_constraints"], r1cs["nb_wires"]
    rp, col, cf = r1cs["C"]
    rp = np.asarray(rp, np.uint64).astype(np.int64)
    one_slot = len(r1cs["coeffs"])
    out = {k: v for k, v in r1cs.items() if k not in ("lens", "planted", "long_at")}
    out["coeffs"] = np.concatenate([r1cs["coeffs"], D.ONE.reshape(1, 4)])
    out["C"] = ((rp + np.arange(nc + 1)).astype(np.uint64), np.insert(col, rp[1:], (nw + np.arange(nc)).astype(np.uint32)),
                np.insert(cf, rp[1:], np.uint32(one_slot)))
    out["nb_wires"], out["slack0"] = nw + nc, nw
    a, b = eval_rows(r1cs, "A", W), eval_rows(r1cs, "B", W)
    c = _op(MUL, a, b)
    W2 = np.concatenate([W, _op(SUB, c, eval_rows(r1cs, "C", W))])
    return out, W2, a, b, c


def bumped(W, wires):
    """a copy of W with 1 added to each of the wires"""
    W2 = W.copy()
    idx = np.asarray(sorted(set(int(w) for w in wires)), np.int64)
    W2[idx] = _op(ADD, np.ascontiguousarray(W[idx]), D._bc(D.ONE, len(idx)))
    return W2

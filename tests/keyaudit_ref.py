"""A Python-integer model of the key audit (include/mi355x_groth16_keyaudit.h): the table of relations IN THE EXPONENT, and its sums as
pyref points.  Nothing here calls the code under test.

A key is a dict of exponents (discrete logarithms to g1 / g2, integers mod r; None = the point at infinity inside an array):
    nb_wires, inf_a, inf_b (lists of bool), a, b1, b2, k, z (stored order), vk_k, basis / bes (a list per commitment),
    alpha1, beta1, delta1, beta2, delta2 (the proving key's), vk_alpha1, vk_beta2, vk_gamma2, vk_delta2, g / g_sigma_neg (a value per commitment)
An SRS is a dict of exponent rows: tau_g1 (2 N), alpha_tau_g1, beta_tau_g1, tau_g2 (N), beta_g2.
A circuit is the R1CS dict binding.Context.setup takes (tests/setup_cases.py).
A pairing relation e(P, Q) = e(P', Q') reads p q = p' q' mod r.

The inverse transform is written out from its DEFINITION, p_k = (1 / N) sum_i u_i w^(-i k) with w = fft.NewDomain's generator: index i
means w^i.  The coefficient stream is restated from its specification (SHA-256).
"""
import hashlib
import pyref as P
from helpers import fr_vals

R = P.R_MOD
SMALL, A, B1, B2, K_PRIVATE, K_PUBLIC, BASIS, SIGMA, Z = 1, 2, 4, 8, 16, 32, 64, 128, 256
ALL = 511
CLS_P, CLS_V, CLS_C = 0, 1, 2


def coefficient(seed: bytes, k: int) -> int:
    """r_k: the little-endian integer of the first 16 bytes of SHA-256("mi355x-ceremony-coeff" | seed | le64(k))"""
    assert len(seed) == 32
    return int.from_bytes(hashlib.sha256(b"mi355x-ceremony-coeff" + seed + k.to_bytes(8, "little")).digest()[:16], "little")


def rows_of(r1cs):
    """the three matrices as lists of rows of (wire, coefficient) pairs, in Python integers"""
    co = fr_vals(r1cs["coeffs"]) if len(r1cs["coeffs"]) else []
    out = []
    for name in "ABC":
        rp, col, cf = r1cs[name]
        out.append([[(int(col[e]), co[int(cf[e])]) for e in range(int(rp[i]), int(rp[i + 1]))] for i in range(r1cs["n_constraints"])])
    return out


def wire_classes(r1cs):
    cls = [CLS_V if j < r1cs["nb_public"] else CLS_P for j in range(r1cs["nb_wires"])]
    for ws, cw in r1cs["commitments"]:
        for j in ws:
            cls[int(j)] = CLS_C
        cls[int(cw)] = CLS_V
    return cls


def domain_of(r1cs):
    return P.Domain(r1cs["n_constraints"])


def inverse_transform(dom, v):
    """p_k = (1 / N) sum_i v_i w^(-i k), v padded with zeros to N"""
    v = list(v) + [0] * (dom.n - len(v))
    return [x * dom.card_inv % R for x in P.dft_definition(v, dom.gen_inv)]


def srs_exps(tau, alpha, beta, n):
    pw = [pow(tau, k, R) for k in range(2 * n)]
    return {"tau_g1": pw, "alpha_tau_g1": [alpha * x % R for x in pw[:n]], "beta_tau_g1": [beta * x % R for x in pw[:n]], "tau_g2": pw[:n], "beta_g2": beta}


def column_exps(r1cs, tau):
    """A_j, B_j, C_j = sum_i M[i][j] L_i(tau), by the definition of mi355x_groth16_setup.h"""
    dom = domain_of(r1cs)
    L = P.lagrange_at(dom, tau)
    out = []
    for m in rows_of(r1cs):
        col = [0] * r1cs["nb_wires"]
        for i, row in enumerate(m):
            for j, c in row:
                col[j] = (col[j] + c * L[i]) % R
        out.append(col)
    return out


def honest_key(r1cs, tau, alpha, beta, gamma, delta, sigma=(), abc=None):
    """the key mi_groth16_setup makes, in the exponent.  abc: A_j, B_j, C_j from elsewhere (pyref.toy_setup's), else column_exps"""
    dom = domain_of(r1cs)
    n = dom.n
    Aj, Bj, Cj = abc if abc is not None else column_exps(r1cs, tau)
    cls = wire_classes(r1cs)
    nw = r1cs["nb_wires"]
    t = [(beta * Aj[j] + alpha * Bj[j] + Cj[j]) % R for j in range(nw)]
    gi, di = P.fr_inv(gamma), P.fr_inv(delta)
    pt = lambda x: x if x else None
    zt = (pow(tau, n, R) - 1) * di % R
    basis = [[pt(t[int(j)] * gi % R) for j in ws] for ws, _ in r1cs["commitments"]]
    return {"nb_wires": nw, "inf_a": [x == 0 for x in Aj], "inf_b": [x == 0 for x in Bj],
            "a": [x for x in Aj if x], "b1": [x for x in Bj if x], "b2": [x for x in Bj if x],
            "k": [pt(t[j] * di % R) for j in range(nw) if cls[j] == CLS_P],
            "z": P.bit_reverse_perm([zt * pow(tau, i, R) % R for i in range(n)]),
            "vk_k": [pt(t[j] * gi % R) for j in range(nw) if cls[j] == CLS_V],
            "basis": basis, "bes": [[None if x is None else x * s % R for x in b] for b, s in zip(basis, sigma)],
            "alpha1": alpha, "beta1": beta, "delta1": delta, "beta2": beta, "delta2": delta,
            "vk_alpha1": alpha, "vk_beta2": beta, "vk_gamma2": gamma, "vk_delta2": delta,
            "g": [1] * len(basis), "g_sigma_neg": [(-s) % R for s in sigma]}


def _dot(coeffs, exps):
    return sum(c * (0 if e is None else e) for c, e in zip(coeffs, exps)) % R


def sums(r1cs, srs, key, seed, coeff=coefficient):
    """both sides of every relation before pairing, as exponents: {name: (the key's side, the SRS's side)}, "sigma": [(over Basis_k,
    over BasisExpSigma_k)]"""
    dom = domain_of(r1cs)
    n, nw, nc = dom.n, r1cs["nb_wires"], r1cs["n_constraints"]
    r = [coeff(seed, j) for j in range(nw)]
    q = [coeff(seed, nw + i) for i in range(n)]
    cls = wire_classes(r1cs)
    mats = rows_of(r1cs)
    masked = lambda x: [r[j] if cls[j] == x else 0 for j in range(nw)]
    prod = lambda m, v: [sum(c * v[j] for j, c in row) % R for row in mats[m]]
    S = lambda v, row: _dot(inverse_transform(dom, v), row[:n])
    T = lambda v: (S(prod(0, v), srs["beta_tau_g1"]) + S(prod(1, v), srs["alpha_tau_g1"]) + S(prod(2, v), srs["tau_g1"])) % R
    slots = lambda mask: [r[j] for j in range(nw) if not mask[j]]
    out = {"a": (_dot(slots(key["inf_a"]), key["a"]), S(prod(0, r), srs["tau_g1"])),
           "b1": (_dot(slots(key["inf_b"]), key["b1"]), S(prod(1, r), srs["tau_g1"])),
           "b2": (_dot(slots(key["inf_b"]), key["b2"]), S(prod(1, r), srs["tau_g2"])),
           "k_private": (_dot([r[j] for j in range(nw) if cls[j] == CLS_P], key["k"]), T(masked(CLS_P))),
           "k_public": (_dot([r[j] for j in range(nw) if cls[j] == CLS_V], key["vk_k"]), T(masked(CLS_V))),
           "z": (_dot([q[P.bitrev(m, dom.log_n)] for m in range(n)], key["z"]), (_dot(q, srs["tau_g1"][n:2 * n]) - _dot(q, srs["tau_g1"][:n])) % R)}
    sig = []
    for (ws, _), b, e in zip(r1cs["commitments"], key["basis"], key["bes"]):
        rc = [r[int(j)] for j in ws]
        sig.append((_dot(rc, b), _dot(rc, e)))
    out["basis"] = (sum(x for x, _ in sig) % R, T(masked(CLS_C)))
    out["sigma"] = sig
    return out


def audit(r1cs, srs, key, seed, coeff=coefficient):
    """the mask of relations that do not hold"""
    s = sums(r1cs, srs, key, seed, coeff)
    mask = 0
    small = (key["alpha1"] == key["vk_alpha1"] == srs["alpha_tau_g1"][0] and key["beta1"] == srs["beta_tau_g1"][0] and
             key["beta2"] == key["vk_beta2"] == srs["beta_g2"] and key["delta2"] == key["vk_delta2"] and key["delta1"] == key["delta2"])
    if not small:
        mask |= SMALL
    for name, bit in (("a", A), ("b1", B1), ("b2", B2)):
        if s[name][0] != s[name][1]:
            mask |= bit
    for name, bit, q in (("k_private", K_PRIVATE, key["delta2"]), ("k_public", K_PUBLIC, key["vk_gamma2"]), ("basis", BASIS, key["vk_gamma2"]),
                         ("z", Z, key["delta2"])):
        if s[name][0] * q % R != s[name][1]:
            mask |= bit
    for (b, e), g, gsn in zip(s["sigma"], key["g"], key["g_sigma_neg"]):
        if (b * gsn + e * g) % R:
            mask |= SIGMA
    return mask


def sum_points(s):
    """sums()' exponents as pyref points: {name: (key side, SRS side)}; b2 in G2"""
    g1 = lambda x: P.g1_mul(P.G1_GEN, x) if x else None
    g2 = lambda x: P.g2_mul(P.G2_GEN, x) if x else None
    out = {n: (g1(s[n][0]), g1(s[n][1])) for n in ("a", "b1", "k_private", "k_public", "basis", "z")}
    out["b2"] = (g2(s["b2"][0]), g2(s["b2"][1]))
    out["sigma"] = [(g1(b), g1(e)) for b, e in s["sigma"]]
    return out


# ---------------------------------------------------------------------------------------------------- tampers, in the exponent
def tampers(key, n_commitments):
    """[(name, a function that changes a copy of the key, the bits it flips)]: the list of tests/test_gpu_keyaudit.py"""
    import copy

    def make(f):
        def run(k):
            k = copy.deepcopy(k)
            f(k)
            return k
        return run

    def one_a(k): k["a"][1] = (k["a"][1] + 5) % R
    def pair_a(k): k["a"][0] = (k["a"][0] + 12345) % R; k["a"][2] = (k["a"][2] - 12345) % R
    def flag_a(k):
        j = [j for j in range(k["nb_wires"]) if not k["inf_a"][j]][1]
        k["inf_a"][j] = True
        del k["a"][1]
    def one_b2(k): k["b2"][0] = (k["b2"][0] + 1) % R
    def scale_k(k): k["k"] = [None if x is None else x * 3 % R for x in k["k"]]
    def one_vk(k): k["vk_k"][0] = ((k["vk_k"][0] or 0) + 9) % R
    def swap_z(k): k["z"][0], k["z"][1] = k["z"][1], k["z"][0]
    def delta(k): k["delta1"] = k["delta2"] = (k["delta2"] * 7 + 1) % R   # the proving key's; the verifying key keeps its own
    out = [("one point of A", make(one_a), A), ("a cancelling pair in A", make(pair_a), A), ("a wire of A flagged infinite", make(flag_a), A),
           ("one point of G2.B", make(one_b2), B2), ("K scaled", make(scale_k), K_PRIVATE), ("one point of vk.K", make(one_vk), K_PUBLIC),
           ("two points of Z swapped", make(swap_z), Z), ("another delta", make(delta), SMALL | K_PRIVATE | Z)]
    if n_commitments:
        def one_basis(k): k["basis"][0][0] = ((k["basis"][0][0] or 0) + 4) % R
        def other_sigma(k): k["bes"][0] = [None if x is None else x * 11 % R for x in k["basis"][0]]
        out += [("one point of Basis", make(one_basis), BASIS | SIGMA), ("BasisExpSigma of another sigma", make(other_sigma), SIGMA)]
    return out

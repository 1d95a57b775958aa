"""Inputs shared by tests/test_pairing_cpu.py, tests/test_gpu_verify.py and tools/gen_pairing_golden.py: toy Groth16 proofs with their
verifying keys (pyref.toy_setup keys, so every discrete log is known and pyref.trapdoor_check can judge the same proof), their conversion
to the binding's arrays, the pairs of a proof in the order csrc/pairing_ops.cuh lays them out, and a twist point outside the r-torsion.
Nothing here calls the code under test."""
import ctypes as C
import os
import subprocess
import numpy as np
import pyref as P
import pairing_ref as R
from helpers import fr_arr, fp_arr, fp_vals, g1_arr, g2_arr

HERE = os.path.dirname(os.path.abspath(__file__))
F12_MUL, F12_SQR, F12_INV, F12_FROB1, F12_FROB2, F12_FROB3, F12_CYCLO_SQR, F12_CONJ, F12_EASY, F12_FINAL_EXP, F12_MUL_LINE = range(11)
F12_ADD, F12_SUB, F12_FP6_MUL, F12_FP6_SQR, F12_FP6_INV, F12_OP_END = 11, 12, 13, 14, 15, 16


def build_emu(so):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DMI_CHECK_NOWRAP", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "emu", "emu_pairing.cpp")])
    return so


def p_(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def gt_arr(towers):
    """lists of 12 canonical Fp coefficients in the tower order -> (n, 48) uint64 Montgomery records"""
    return np.stack([fp_arr(t).reshape(48) for t in towers]) if len(towers) else np.zeros((0, 48), np.uint64)


def gt_vals(arr):
    return [fp_vals(row.reshape(12, 4)) for row in np.asarray(arr).reshape(-1, 48)]


def seeded_pairs(n, seed, inf_first_last=True):
    """n (P, Q) pairs of subgroup points from small known multiples of the generators (cheap in Python), infinity in G1 at the first and
    in G2 at the last index"""
    rng = np.random.default_rng(seed)
    ks = rng.integers(1, 1 << 20, (n, 2))
    base1 = [P.g1_mul(P.G1_GEN, int(k)) for k in range(1, 18)]
    base2 = [P.g2_mul(P.G2_GEN, int(k)) for k in range(1, 18)]
    ps = [base1[int(a) % 17] for a, _ in ks]
    qs = [base2[int(b) % 17] for _, b in ks]
    if inf_first_last and n:
        ps[0] = None
        if n > 1:
            qs[-1] = None
    return ps, qs


# ---------------------------------------------------------------------------------------------------- a twist point of the wrong order
def fp2_sqrt(a):
    """a square root of a in Fp2 = Fp[u]/(u^2+1), or None (p = 3 mod 4)"""
    p = P.Q_MOD
    a0, a1 = a
    if a1 == 0:
        s = pow(a0, (p + 1) // 4, p)
        if s * s % p == a0:
            return (s, 0)
        s = pow(-a0 % p, (p + 1) // 4, p)
        return (0, s) if s * s % p == -a0 % p else None
    n = (a0 * a0 + a1 * a1) % p
    s = pow(n, (p + 1) // 4, p)
    if s * s % p != n:
        return None
    for sg in (s, -s % p):
        h = (a0 + sg) * pow(2, -1, p) % p
        x0 = pow(h, (p + 1) // 4, p)
        if x0 and x0 * x0 % p == h:
            x1 = a1 * pow(2 * x0, -1, p) % p
            if P.fp2_sqr((x0, x1)) == (a0 % p, a1 % p):
                return (x0, x1)
    return None


def twist_point_outside_subgroup():
    """the first x = (k, 1), k = 1, 2, ... with a point on y^2 = x^3 + 3/(9+u) whose order does not divide r (the twist has a cofactor)"""
    for k in range(1, 200):
        x = (k, 1)
        y = fp2_sqrt(P.fp2_add(P.fp2_mul(P.fp2_sqr(x), x), P.G2_B))
        if y is not None:
            Q = (x, y)
            assert P.g2_is_on_curve(Q)
            if P.g2_mul(Q, P.R_MOD) is not None:
                return Q
    raise AssertionError("no point found")


# ---------------------------------------------------------------------------------------------------- toy proofs with known discrete logs
def toy_case(n_commitments, nb_constraints=12, nb_public=3, seed=7):
    """A toy circuit, its key under a known trapdoor, its proof, and what a verifier is given.  With commitments: commitment k commits to
    two private wires and owns a third (the wire whose value plays the hash: the library is hash-free, the caller defines it), Basis =
    (t_j / gamma) g1 and pok = sigma_k C_k as mi_groth16_setup defines them; Krs loses the K points of those wires, as a key loaded with
    committed_wires makes it."""
    cs = P.ToyR1CS(nb_constraints, nb_public, seed, 0.3)
    td = P.ToyTrapdoor(seed + 1)
    pk, exps, dom = P.toy_setup(cs, td)
    r, s = 0x1234567 + seed, 0x7654321 + seed
    proof = P.toy_prove(cs, pk, dom, r, s)
    w = cs.wires
    q = P.R_MOD
    kg = lambda j: exps["K"][j] * td.delta % q * P.fr_inv(td.gamma) % q        # t_j / gamma
    g1 = lambda e: P.g1_mul(P.G1_GEN, e % q)
    sigmas = [(0xABCDEF + 977 * k) % q for k in range(n_commitments)]
    priv = list(range(nb_public, cs.nb_wires))
    commits = [(priv[3 * k: 3 * k + 2], priv[3 * k + 2]) for k in range(n_commitments)]
    krs = proof["krs"]
    cpts, cvals = [], []
    for wires, cw in commits:
        for j in wires + [cw]:
            krs = P.g1_add(krs, P.g1_neg(g1(w[j] * exps["K"][j])))
        cpts.append(g1(sum(w[j] * kg(j) for j in wires)))
        cvals.append(w[cw])
    ch = 0x5EED5EED
    pok = None
    for k, c in enumerate(cpts):
        pok = P.g1_add(pok, P.g1_mul(c, sigmas[k] * pow(ch, k, q) % q))
    vk = {"alpha1": pk["alpha1"], "beta2": pk["beta2"], "gamma2": P.g2_mul(P.G2_GEN, td.gamma), "delta2": pk["delta2"],
          "k": [g1(kg(j)) for j in range(nb_public)] + [g1(kg(cw)) for _, cw in commits], "nb_public": nb_public,
          "ped": R.pedersen_vk(sigmas)}
    return {"cs": cs, "td": td, "exps": exps, "r": r, "s": s, "toy_proof": proof, "vk": vk, "proof": (proof["ar"], proof["bs"], krs),
            "public_inputs": list(w[1:nb_public]), "commitments": cpts, "commitment_values": cvals, "pok": pok, "fold_challenge": ch,
            "sigmas": sigmas}


def ref_verdict(case, **over):
    c = dict(case, **over)
    return R.groth16_verify(c["vk"], c["proof"], c["public_inputs"], c["commitments"], c["commitment_values"], c["pok"], c["fold_challenge"])


def vk_arrays(vk):
    """pairing_ref's vk dict -> (the dict binding.Context.vk_load takes, nb_public, ped (n, 2, 16) or None)"""
    d = {"alpha1": g1_arr([vk["alpha1"]])[0], "beta2": g2_arr([vk["beta2"]])[0], "gamma2": g2_arr([vk["gamma2"]])[0],
         "delta2": g2_arr([vk["delta2"]])[0], "k": g1_arr(vk["k"])}
    ped = np.stack([g2_arr([g, gs]) for g, gs in vk["ped"]]) if vk["ped"] else None
    return d, vk["nb_public"], ped


def proof_dict(case, **over):
    """what binding.VerifyingKey.verify takes"""
    c = dict(case, **over)
    ar, bs, krs = c["proof"]
    d = {"raw": np.concatenate([g1_arr([ar])[0], g2_arr([bs])[0], g1_arr([krs])[0]]), "public_inputs": fr_arr(c["public_inputs"])}
    if c["commitments"]:
        d.update(commitments=g1_arr(c["commitments"]), pok=g1_arr([c["pok"]])[0], commitment_values=fr_arr(c["commitment_values"]),
                 fold_challenge=fr_arr([c["fold_challenge"]])[0])
    return d


def emu_pairs(case, **over):
    """(P (n, 8), Q (n, 16), n_ped) of one proof in the order of csrc/pairing_ops.cuh, kSum and the folded commitments by pyref"""
    c = dict(case, **over)
    vk = c["vk"]
    ar, bs, krs = c["proof"]
    ks = R.k_sum(vk, c["public_inputs"], c["commitment_values"], c["commitments"])
    ps, qs = [ar, P.g1_neg(ks), P.g1_neg(krs)], [bs, vk["gamma2"], vk["delta2"]]
    if c["commitments"]:
        ps.append(c["pok"]); qs.append(vk["ped"][0][0])
        for k, cm in enumerate(c["commitments"]):
            ps.append(P.g1_mul(cm, pow(c["fold_challenge"], k, P.R_MOD))); qs.append(vk["ped"][k][1])
    return g1_arr(ps), g2_arr(qs), len(ps) - 3

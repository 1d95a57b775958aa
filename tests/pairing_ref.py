"""Definitional BN254 pairing in Python integers, the reference of the pairing / verifier tests.  It shares no formula with
gnark-whir_amd/csrc/fp12.cuh / pairing.cuh: Fp12 is the one-step extension Fp[w]/(w^12 - 18 w^6 + 82), a G2 point is untwisted into E(Fp12),
the Miller loop uses the generic affine chord-and-tangent lines of y^2 = x^3 + 3 over Fp12, and the final exponentiation is ONE pow(f, d')
with the exponent the device header states,
    d' = s (p^12 - 1) / r,   s = 2 x0 (6 x0^2 + 3 x0 + 1)        (s is coprime to r).
Values cross to the device as 12 Fp coefficients in the tower order C0.B0.A0, C0.B0.A1, C0.B1.A0, ... C1.B2.A1 of
Fp2 = Fp[u]/(u^2+1), Fp6 = Fp2[v]/(v^3 - (9+u)), Fp12 = Fp6[w]/(w^2 - v): to_tower / from_tower write that basis change out."""
import pyref as P

p = P.Q_MOD
r = P.R_MOD
X0 = 4965661367192848881
ATE_LOOP = 6 * X0 + 2
S_COFACTOR = 2 * X0 * (6 * X0 * X0 + 3 * X0 + 1)
assert (p ** 12 - 1) % r == 0 and S_COFACTOR % r != 0
D_PRIME = S_COFACTOR * ((p ** 12 - 1) // r)
assert p == 36 * X0 ** 4 + 36 * X0 ** 3 + 24 * X0 ** 2 + 6 * X0 + 1 and r == 36 * X0 ** 4 + 36 * X0 ** 3 + 18 * X0 ** 2 + 6 * X0 + 1


# ---------------------------------------------------------------- Fp12 = Fp[w]/(w^12 - 18 w^6 + 82): a tuple of 12 ints, index = power of w
ZERO = (0,) * 12
ONE = (1,) + (0,) * 11


def f_add(a, b):
    return tuple((x + y) % p for x, y in zip(a, b))


def f_sub(a, b):
    return tuple((x - y) % p for x, y in zip(a, b))


def f_neg(a):
    return tuple(-x % p for x in a)


def f_mul(a, b):
    t = [0] * 23
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                t[i + j] += x * y
    for k in range(22, 11, -1):    # w^12 = 18 w^6 - 82
        c = t[k]
        t[k - 6] += 18 * c
        t[k - 12] -= 82 * c
    return tuple(x % p for x in t[:12])


def f_pow(a, e):
    out = ONE
    for bit in bin(e)[2:]:
        out = f_mul(out, out)
        if bit == "1":
            out = f_mul(out, a)
    return out


def f_inv(a):
    """a^-1 by solving a x = 1 as a 12 x 12 linear system over Fp: definitional, independent of every tower formula, and cheaper than
    the 3000 squarings of a^(p^12 - 2)"""
    rows = []
    for j in range(12):     # column j of the multiplication-by-a matrix = a * w^j
        col = f_mul(a, tuple(1 if k == j else 0 for k in range(12)))
        rows.append(col)
    m = [[rows[j][i] for j in range(12)] + [1 if i == 0 else 0] for i in range(12)]
    for c in range(12):
        piv = next(i for i in range(c, 12) if m[i][c])
        m[c], m[piv] = m[piv], m[c]
        inv = pow(m[c][c], -1, p)
        m[c] = [v * inv % p for v in m[c]]
        for i in range(12):
            if i != c and m[i][c]:
                k = m[i][c]
                m[i] = [(v - k * w) % p for v, w in zip(m[i], m[c])]
    return tuple(m[i][12] for i in range(12))


def f_scalar(k):
    return (k % p,) + (0,) * 11


W2 = tuple(1 if k == 2 else 0 for k in range(12))
W3 = tuple(1 if k == 3 else 0 for k in range(12))


def fp2_embed(a):
    """a0 + a1 u with u = w^6 - 9"""
    return tuple(((a[0] - 9 * a[1]) % p if k == 0 else (a[1] % p if k == 6 else 0)) for k in range(12))


def to_tower(f):
    """the 12 tower coefficients [C_i.B_j.A_k at index 6 i + 2 j + k] of f = sum_m f[m] w^m.
    C_i.B_j = a0 + a1 u multiplies w^i v^j = w^(i + 2 j) =: w^e, and u = w^6 - 9, so a0 + a1 u -> (a0 - 9 a1) w^e + a1 w^(e+6):
    a1 = f[e + 6], a0 = f[e] + 9 f[e + 6]."""
    out = [0] * 12
    for i in range(2):
        for j in range(3):
            e = i + 2 * j
            out[6 * i + 2 * j + 1] = f[e + 6] % p
            out[6 * i + 2 * j] = (f[e] + 9 * f[e + 6]) % p
    return out


def from_tower(t):
    f = [0] * 12
    for i in range(2):
        for j in range(3):
            e = i + 2 * j
            a0, a1 = t[6 * i + 2 * j], t[6 * i + 2 * j + 1]
            f[e] = (a0 - 9 * a1) % p
            f[e + 6] = a1 % p
    return tuple(f)


# ---------------------------------------------------------------- E(Fp12): y^2 = x^3 + 3, affine, None = infinity
def untwist(Q):
    """(x', y') on the twist y^2 = x^3 + 3/(9+u) -> (x' w^2, y' w^3) on E(Fp12)   (w^6 = 9 + u)"""
    if Q is None:
        return None
    return (f_mul(fp2_embed(Q[0]), W2), f_mul(fp2_embed(Q[1]), W3))


def embed_g1(Pt):
    return None if Pt is None else (f_scalar(Pt[0]), f_scalar(Pt[1]))


def e12_on_curve(Pt):
    x, y = Pt
    return f_mul(y, y) == f_add(f_mul(f_mul(x, x), x), f_scalar(3))


def _line_and_sum(T, Q, Pt):
    """the line through T and Q (the tangent when T == Q) evaluated at Pt, and T + Q.  A vertical line contributes 1 (its value lies in a
    proper subfield of Fp12 and dies in the final exponentiation) and the sum is infinity."""
    (x1, y1), (x2, y2) = T, Q
    if x1 == x2:
        if y1 != y2 or y1 == ZERO:
            return ONE, None
        lam = f_mul(f_mul(f_scalar(3), f_mul(x1, x1)), f_inv(f_add(y1, y1)))
    else:
        lam = f_mul(f_sub(y2, y1), f_inv(f_sub(x2, x1)))
    x3 = f_sub(f_sub(f_mul(lam, lam), x1), x2)
    y3 = f_sub(f_mul(lam, f_sub(x1, x3)), y1)
    xp, yp = Pt
    line = f_sub(f_sub(yp, y1), f_mul(lam, f_sub(xp, x1)))
    return line, (x3, y3)


def frob_point(Pt):
    """the p-power Frobenius of E(Fp12)"""
    return (f_pow(Pt[0], p), f_pow(Pt[1], p))


def miller_loop(Pt, Q):
    """optimal ate: f_{6 x0 + 2, Q}(P) l_{[6x0+2]Q, pi(Q)}(P) l_{[6x0+2]Q + pi(Q), -pi^2(Q)}(P); 1 when either point is infinity"""
    if Pt is None or Q is None:
        return ONE
    Pe, Qe = embed_g1(Pt), untwist(Q)
    assert e12_on_curve(Qe)
    f, T = ONE, Qe
    for bit in bin(ATE_LOOP)[3:]:
        line, T2 = _line_and_sum(T, T, Pe)
        f = f_mul(f_mul(f, f), line)
        T = T2
        if bit == "1":
            line, T = _line_and_sum(T, Qe, Pe)
            f = f_mul(f, line)
    Q1 = frob_point(Qe)
    Q2 = frob_point(Q1)
    Q2 = (Q2[0], f_neg(Q2[1]))
    line, T = _line_and_sum(T, Q1, Pe)
    f = f_mul(f, line)
    line, T = _line_and_sum(T, Q2, Pe)
    return f_mul(f, line)


def final_exp(f):
    return f_pow(f, D_PRIME)


def pairing(Pt, Q):
    """e(P, Q)^s in the w-power basis"""
    return final_exp(miller_loop(Pt, Q))


def pairing_tower(Pt, Q):
    return to_tower(pairing(Pt, Q))


def g2_in_subgroup(Q):
    return Q is None or (P.g2_is_on_curve(Q) and P.g2_mul(Q, r) is None)


# ---------------------------------------------------------------- Groth16 + BSB22 verification by the two equations
OK, PAIRING, PEDERSEN, MALFORMED = 0, 1, 2, 3


def pedersen_vk(sigmas):
    return [(P.G2_GEN, P.g2_mul(P.G2_GEN, (r - s) % r)) for s in sigmas]


def k_sum(vk, public_inputs, commitment_values, commitments):
    nb_public = vk["nb_public"]
    assert len(public_inputs) == nb_public - 1 and len(vk["k"]) == nb_public + len(commitments)
    acc = vk["k"][0]
    for i, v in enumerate(public_inputs):
        acc = P.g1_add(acc, P.g1_mul(vk["k"][1 + i], v % r))
    for k, v in enumerate(commitment_values):
        acc = P.g1_add(acc, P.g1_mul(vk["k"][nb_public + k], v % r))
    for c in commitments:
        acc = P.g1_add(acc, c)
    return acc


def groth16_verify(vk, proof, public_inputs, commitments=(), commitment_values=(), pok=None, fold_challenge=1):
    """vk: dict alpha1, beta2, gamma2, delta2, k (list), nb_public, ped (list of (G, GSigmaNeg)); proof = (Ar, Bs, Krs).
    0: both equations hold; 1: e(Ar,Bs) != e(alpha,beta) e(kSum,gamma) e(Krs,delta); 2: prod_k e(c^k C_k, GSigmaNeg_k) e(pok, G) != 1;
    3: a point off its curve, or Bs outside the r-torsion.  The order of the checks is 3, 1, 2."""
    ar, bs, krs = proof
    g1s = [ar, krs, pok] + list(commitments)
    if any(q is not None and not P.g1_is_on_curve(q) for q in g1s) or not g2_in_subgroup(bs):
        return MALFORMED
    ks = k_sum(vk, public_inputs, commitment_values, commitments)
    lhs = f_mul(f_mul(miller_loop(ar, bs), miller_loop(P.g1_neg(ks), vk["gamma2"])), miller_loop(P.g1_neg(krs), vk["delta2"]))
    if final_exp(lhs) != pairing(vk["alpha1"], vk["beta2"]):
        return PAIRING
    if commitments:
        f, ck = miller_loop(pok, vk["ped"][0][0]), 1
        for k, c in enumerate(commitments):
            f = f_mul(f, miller_loop(P.g1_mul(c, ck), vk["ped"][k][1]))
            ck = ck * fold_challenge % r
        if final_exp(f) != ONE:
            return PEDERSEN
    return OK

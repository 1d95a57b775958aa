"""Replays the value / limb bounds of the 29-bit-limb arithmetic (gnark-whir_amd/csrc/curve29.cuh, curve29_g2.cuh) with worst-case interval
arithmetic and checks every precondition of the primitives in field29.cuh.  V = value bound in multiples of p, L = limb bound in bits
(limbs 0..7).  Run: python tools/f29_bounds.py

The accumulator invariants below (G1_ACC, G1_LOADED, G2_ACC, G2_STORED) are what the header comments claim; replay() proves that the
group steps keep them, and tests/test_device_headers_on_host.py builds its adversarial states from the same numbers."""
import math

P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
WEAK = math.log2(2 ** 29 + 8)
EPS = 2 ** 233 / P                  # what f29_condsub's top-limb test cannot see (field29.cuh), in multiples of p
TWO256 = 2 ** 256 / P               # a packed coordinate (8 x u32) holds any representative below 2^256 ~ 5.29 p

# accumulator invariants: coordinate -> (V, L)
G1_ACC = {"X": (5.7, WEAK), "Y": (1.8, 29), "ZZ": (1.04, 29), "ZZZ": (1.04, 29)}      # curve29.cuh, the running sum
G1_LOADED = {"X": (4.02, 29), "Y": (1.8, 29), "ZZ": (1.04, 29), "ZZZ": (1.04, 29)}   # what g1x29_load_rp returns
G2_ACC = {"X": (2.1, WEAK), "Y": (3.6, 29), "ZZ": (1.1, 29), "ZZZ": (1.1, 29)}       # curve29_g2.cuh, per Fp component
G2_STORED = {"X": (2.1, 29), "Y": (3.6, 29), "ZZ": (1.1, 29), "ZZZ": (1.1, 29)}      # a packed G2 partial sum, unpacked (normalised)


class B:
    def __init__(self, V, L, name):
        self.V, self.L, self.name = V, L, name


def _cols(pairs, name):
    """a product column: 9 multiplications per operand pair and 9 reduction terms m_i p_j (< 2^58), plus the carry (< 2^35)"""
    s = sum(9 * 2 ** (a.L + b.L) for a, b in pairs) + 9 * 2 ** 58 + 2 ** 35
    assert s < 2 ** 64, (name, math.log2(s))


def mul(x, y, name):
    assert x.L + y.L <= 60.0 + 1e-6, (name, x.L, y.L)          # 9 * 2^60 + 9 * 2^58 + carry < 2^64
    _cols([(x, y)], name)
    V = x.V * y.V / 128 + 1
    assert V < 64, name                                         # the top limb of the result stays below 2^29
    return B(V, 29, name)


def sqr(x, name):
    assert 2 * x.L <= 60.0 + 1e-6, (name, x.L)                  # f29_sqr doubles limbs: x_i < 2^31
    return mul(x, x, name)


def mul2(a, b, c, d, name):
    assert a.L + b.L <= 59.0 + 1e-6 and c.L + d.L <= 59.0 + 1e-6, name   # 18 * 2^59 + 9 * 2^58 < 2^64
    _cols([(a, b), (c, d)], name)
    V = (a.V * b.V + c.V * d.V) / 128 + 1
    assert V < 64, name
    return B(V, 29, name)


def mul4(a, b, c, d, e, f, g, h, name):
    ops = (a, b, c, d, e, f, g, h)
    assert all(o.L <= WEAK + 1e-9 for o in ops), (name, [o.L for o in ops])   # every operand weakly normalised: 45 (2^29+8)^2 + 2^35 < 2^63.5
    _cols([(a, b), (c, d), (e, f), (g, h)], name)
    V = (a.V * b.V + c.V * d.V + e.V * f.V + g.V * h.V) / 128 + 1
    assert V < 64, name
    return B(V, 29, name)


def add(x, y, name):
    L = math.log2(2 ** x.L + 2 ** y.L)
    assert L <= 32, name
    return B(x.V + y.V, L, name)


def sub(x, y, K, name):
    assert y.L <= WEAK + 1e-9 and y.V < K - 0.01, (name, y.L, y.V, K)   # borrowed K p: limbs >= 2^30 - 2, top limb = (K p >> 232) - 2
    L = math.log2(2 ** x.L + 2 ** 30.59)
    assert L <= 32, name
    return B(x.V + K, L, name)


def wnorm(x, name=None):
    assert x.L <= 32
    return B(x.V, WEAK, name or x.name)


def norm(x, name=None):
    assert x.L <= 31, (name, x.L)                               # f29_norm: limbs < 2^31, one carry pass
    return B(x.V, 29, name or x.name)


def condsub(x, K, name):
    """f29_condsub(x, K p): subtracts when the top limb says x > K p; afterwards < max(V - K, K + EPS).  Input weak; result limbs < 2^30"""
    assert x.L <= WEAK + 1e-9, (name, x.L)
    assert x.V - K <= K + EPS + 1e-12, (name, x.V, K)           # one subtraction must bring it below K p (almost)
    return B(max(x.V - K, K + EPS), 30, name)


def below_2p(x, name):
    """f29_below_2p: condsub 4p, wnorm, condsub 2p, wnorm"""
    return wnorm(condsub(wnorm(condsub(x, 4, name)), 2, name))


def to_std(x, name):
    assert x.V <= 128, (name, x.V)                               # mul'(x, to_std) < 2p: one exact subtraction
    return mul(x, B(1, 29, "to_std"), name)


def packed(x, name):
    """a value written with f29_pack: normalised and below 2^256"""
    assert x.L <= 29 + 1e-9 and x.V < TWO256, (name, x.L, x.V)
    return B(x.V, 29, name)


def special_case_g1(PP):
    assert PP.L <= 29 and PP.V < 2, ("G1: PP in {0, p} decides P = 0 only if PP < 2p", PP.V)


def special_case_g2(PP):
    for c in PP:
        assert c.L <= 29 and c.V < 3, ("G2: each PP component in {0, p, 2p} decides P = 0 only if it is < 3p", c.V)


# ---- G1 (curve29.cuh)
def g1_madd(X, Y, ZZ, ZZZ):
    x2 = B(1, 29, "x2"); y2 = B(1, 29, "y2")
    U2 = mul(x2, ZZ, "U2"); S2 = mul(y2, ZZZ, "S2")
    Pp = wnorm(sub(U2, X, 8, "P")); R = wnorm(sub(S2, Y, 8, "R"))
    PP = sqr(Pp, "PP"); special_case_g1(PP)
    PPP = mul(Pp, PP, "PPP"); Q = mul(X, PP, "Q")
    T = wnorm(add(add(PPP, Q, "T"), Q, "T"))
    RR = sqr(R, "RR")
    X3 = wnorm(sub(RR, T, 4, "X3"))
    D = wnorm(sub(Q, X3, 8, "D"))
    nY = wnorm(sub(B(0, 0, "0"), Y, 8, "nY"))
    Y3 = mul2(R, D, nY, PPP, "Y3")
    return X3, Y3, mul(ZZ, PP, "ZZ3"), mul(ZZZ, PPP, "ZZZ3")


def g1_add(a, b):
    """g1x29_add: a = running sum, b = a loaded partial sum"""
    (Xa, Ya, ZZa, ZZZa), (Xb, Yb, ZZb, ZZZb) = a, b
    U1 = mul(Xa, ZZb, "U1"); U2 = mul(Xb, ZZa, "U2"); S1 = mul(Ya, ZZZb, "S1"); S2 = mul(Yb, ZZZa, "S2")
    Pp = wnorm(sub(U2, U1, 2, "P")); R = wnorm(sub(S2, S1, 2, "R"))
    PP = sqr(Pp, "PP"); special_case_g1(PP)
    PPP = mul(Pp, PP, "PPP"); Q = mul(U1, PP, "Q")
    T = wnorm(add(add(PPP, Q, "T"), Q, "T")); RR = sqr(R, "RR")
    X3 = wnorm(sub(RR, T, 4, "X3")); D = wnorm(sub(Q, X3, 8, "D")); nS1 = wnorm(sub(B(0, 0, "0"), S1, 2, "nS1"))
    return X3, mul2(R, D, nS1, PPP, "Y3"), mul(mul(ZZa, ZZb, "ZZab"), PP, "ZZ3"), mul(mul(ZZZa, ZZZb, "ZZZab"), PPP, "ZZZ3")


def g1_store_load(X, Y, ZZ, ZZZ):
    """g1x29_store_rp: X below 4p + 2^233 (condsub 4p, norm), every coordinate packed; g1x29_load_rp unpacks (normalised)"""
    x = packed(norm(condsub(X, 4, "stored X")), "stored X")
    return x, packed(Y, "stored Y"), packed(ZZ, "stored ZZ"), packed(ZZZ, "stored ZZZ")


# ---- G2 (curve29_g2.cuh): an Fp2 value is a pair of bounds
def f2(V, L, name):
    return (B(V, L, name + ".a0"), B(V, L, name + ".a1"))


def f2_wnorm(x):
    return (wnorm(x[0]), wnorm(x[1]))


def f2_add(x, y, name):
    return (add(x[0], y[0], name), add(x[1], y[1], name))


def f2_sub(x, y, K, name):
    return (wnorm(sub(x[0], y[0], K, name)), wnorm(sub(x[1], y[1], K, name)))


def f2_mul(x, y, K, name):
    """f2_29_mul(x, y, K p): c0 = x0 y0 + x1 (K p - y1), c1 = x0 y1 + x1 y0; needs K > V(y.a1)"""
    n1 = wnorm(sub(B(0, 0, "0"), y[1], K, name + " (K p - y1)"))
    return (mul2(x[0], y[0], x[1], n1, name), mul2(x[0], y[1], x[1], y[0], name))


def f2_sqr(x, name):
    """f2_29_sqr: (a0 + a1)(a0 + 8p - a1), a0 (2 a1)"""
    s = wnorm(add(x[0], x[1], name)); d = wnorm(sub(x[0], x[1], 8, name))
    return (mul(s, d, name), mul(x[0], add(x[1], x[1], name), name))


def f2_mul_sub(x, y, Ky, z, w, Kw, name):
    """f2_29_mul_sub: x y - z w, one reduction per component (f29_mul4)"""
    ny1 = wnorm(sub(B(0, 0, "0"), y[1], Ky, name)); nw0 = wnorm(sub(B(0, 0, "0"), w[0], Kw, name)); nw1 = wnorm(sub(B(0, 0, "0"), w[1], Kw, name))
    return (mul4(x[0], y[0], x[1], ny1, z[0], nw0, z[1], w[1], name), mul4(x[0], y[1], x[1], y[0], z[0], nw1, z[1], nw0, name))


def f2_below_2p(x, name):
    return (below_2p(x[0], name), below_2p(x[1], name))


def g2_madd(X, Y, ZZ, ZZZ):
    x2 = f2(1, 29, "x2"); y2 = f2(1, 29, "y2")
    U2 = f2_mul(ZZ, x2, 2, "U2"); S2 = f2_mul(ZZZ, y2, 2, "S2")
    Pp = f2_sub(U2, X, 4, "P")
    PP = f2_sqr(Pp, "PP"); special_case_g2(PP)
    PPP = f2_mul(Pp, PP, 4, "PPP"); Q = f2_mul(X, PP, 4, "Q")
    ZZ3 = f2_mul(ZZ, PP, 4, "ZZ3"); ZZZ3 = f2_mul(ZZZ, PPP, 2, "ZZZ3")
    R = f2_sub(S2, Y, 4, "R"); RR = f2_sqr(R, "RR")
    T = f2_wnorm(f2_add(f2_add(PPP, Q, "T"), Q, "T"))
    X3 = f2_below_2p(f2_sub(RR, T, 4, "X3"), "X3")
    D = f2_sub(Q, X3, 4, "D")
    Y3 = f2_mul_sub(R, D, 8, Y, PPP, 2, "Y3")
    return X3, Y3, ZZ3, ZZZ3


def g2_add(a, b):
    (Xa, Ya, ZZa, ZZZa), (Xb, Yb, ZZb, ZZZb) = a, b
    U1 = f2_mul(Xa, ZZb, 2, "U1")
    Pp = f2_sub(f2_mul(Xb, ZZa, 2, "U2"), U1, 2, "P")
    PP = f2_sqr(Pp, "PP"); special_case_g2(PP)
    ZZ3 = f2_mul(f2_mul(ZZa, ZZb, 2, "ZZab"), PP, 2, "ZZ3")
    PPP = f2_mul(Pp, PP, 2, "PPP"); Q = f2_mul(U1, PP, 2, "Q")
    S1 = f2_mul(Ya, ZZZb, 2, "S1")
    R = f2_sub(f2_mul(Yb, ZZZa, 2, "S2"), S1, 2, "R")
    ZZZ3 = f2_mul(f2_mul(ZZZa, ZZZb, 2, "ZZZab"), PPP, 2, "ZZZ3")
    RR = f2_sqr(R, "RR")
    T = f2_wnorm(f2_add(f2_add(PPP, Q, "T"), Q, "T"))
    X3 = f2_below_2p(f2_sub(RR, T, 4, "X3"), "X3")
    D = f2_sub(Q, X3, 4, "D")
    return X3, f2_mul_sub(R, D, 8, S1, PPP, 2, "Y3"), ZZ3, ZZZ3


def g2_store(X, Y, ZZ, ZZZ):
    """f2_29_pack: f29_norm per component, packed below 2^256"""
    return tuple((packed(norm(c[0]), "stored"), packed(norm(c[1]), "stored")) for c in (X, Y, ZZ, ZZZ))


def _within(state, inv, what):
    for b, (name, (V, L)) in zip(state, inv.items()):
        for c in (b if isinstance(b, tuple) else (b,)):
            assert c.V <= V and c.L <= L + 1e-9, (what, name, c.V, c.L, V, L)


def _g(inv):
    return tuple(B(V, L, k) for k, (V, L) in inv.items())


def _g2(inv):
    return tuple(f2(V, L, k) for k, (V, L) in inv.items())


def replay(rounds=12):
    """every step of both curves from the first point on and from the invariants themselves; returns the fixed points"""
    out = {}
    # G1: from the first point (x2, y2 unpacked, ZZ = ZZZ = one) to the fixed point, and one step from the invariant itself
    st = (B(1, 29, "X"), B(1, 29, "Y"), B(1.01, 29, "ZZ"), B(1.01, 29, "ZZZ"))
    for _ in range(rounds):
        st = g1_madd(*st)
        _within(st, G1_ACC, "g1x29_madd")
    _within(g1_madd(*_g(G1_ACC)), G1_ACC, "g1x29_madd from the invariant")
    out["g1_madd"] = st
    _within(g1_store_load(*_g(G1_ACC)), G1_LOADED, "g1x29_store_rp / load_rp")
    run = _g(G1_ACC)
    for _ in range(rounds):
        run = g1_add(run, _g(G1_LOADED))
        _within(run, G1_ACC, "g1x29_add")
    _within(g1_add(_g(G1_LOADED), _g(G1_LOADED)), G1_ACC, "g1x29_add of two loaded sums")
    out["g1_add"] = run
    for b in _g(G1_ACC):
        to_std(b, "g1x29_to_std")
    # G2: the same for the mixed addition, the stored partial sums and the full addition
    st = (f2(1, 29, "X"), f2(1, 29, "Y"), f2(1.01, 29, "ZZ"), f2(1.01, 29, "ZZZ"))
    for _ in range(rounds):
        st = g2_madd(*st)
        _within(st, G2_ACC, "g2x29_madd")
    _within(g2_madd(*_g2(G2_ACC)), G2_ACC, "g2x29_madd from the invariant")
    out["g2_madd"] = st
    _within(g2_store(*_g2(G2_ACC)), G2_STORED, "f2_29_pack")
    run = _g2(G2_ACC)
    for _ in range(rounds):
        run = g2_add(run, _g2(G2_STORED))
        _within(run, G2_ACC, "g2x29_add")
    _within(g2_add(_g2(G2_STORED), _g2(G2_STORED)), G2_ACC, "g2x29_add of two stored sums")
    out["g2_add"] = run
    for b in _g2(G2_ACC):
        to_std(b[0], "f2_29_to_std"); to_std(b[1], "f2_29_to_std")
    return out


def _fmt(state):
    flat = []
    for b in state:
        c = b if not isinstance(b, tuple) else max(b, key=lambda x: x.V)
        flat.append(f"V < {c.V:.3f} (L {c.L:.2f})")
    return ", ".join(f"{n} {f}" for n, f in zip(("X", "Y", "ZZ", "ZZZ"), flat))


if __name__ == "__main__":
    res = replay()
    print("G1 fixed point of g1x29_madd:", _fmt(res["g1_madd"]))
    print("G1 g1x29_add keeps the accumulator invariant:", _fmt(res["g1_add"]))
    print("G2 fixed point of g2x29_madd:", _fmt(res["g2_madd"]))
    print("G2 g2x29_add keeps the accumulator invariant:", _fmt(res["g2_add"]))
    print("all preconditions hold (products, f29_mul4, subtractions, conditional subtractions, special cases, store / load, to_std)")

"""Records of gnark-whir_amd/csrc/limb29_ops.cuh for the 29-bit-limb tests (host: tests/emu, device: mi_debug_limb29_op_dev): accumulator
states at the edges of the invariants tools/f29_bounds.py replays, group-step cases with their pyref answers, random edge operands of the
products, and a runner that executes records on the host build in a child process (a trap becomes a failed test naming the case).

Run as a script it is that child: python limb29_cases.py <libemu.so> <op> <in.npy> <out.npy> <progress.npy>"""
import os
import subprocess
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

IN_W, OUT_W, OPERAND, FLAGS, OUT_INF = 144, 80, 72, 136, 72
MUL, MUL2, SUB8, SUB4, SUB2, WNORM, CONDSUB4, CONDSUB2, SQR, MUL4, NORM, UNPACK, PACK, TO_STD, FROM_STD, BELOW_2P, F2_IS_ZERO = range(17)
G1_MADD, G1_ADD, G1_STORE, G2_MADD, G2_ADD, G2_STORE = range(20, 26)
M29 = (1 << 29) - 1


def build_emu(so=os.path.join(HERE, "emu", "libemu.so")):
    src = os.path.join(HERE, "emu", "emu.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DMI_CHECK_NOWRAP", "-shared", "-fPIC", "-o", so, src])
    return so


def bounds():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import f29_bounds
    finally:
        sys.path.pop(0)
    return f29_bounds


# ---- limbs
def val(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


def limbs_of(v):
    return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]


def weak_limbs(v):
    """a weakly normalised representation of v (limbs 0..7 up to 2^29 + 7) wherever a limb allows it, else the normalised one"""
    l = limbs_of(v)
    for i in range(7, -1, -1):
        if l[i] <= 7 and l[i + 1] > 0:
            l[i + 1] -= 1; l[i] += 1 << 29
    assert val(l) == v
    return l


def words_of(v):
    assert 0 <= v < 1 << 256
    return [(v >> (32 * k)) & 0xFFFFFFFF for k in range(8)]


def words_val(w):
    return sum(int(x) << (32 * k) for k, x in enumerate(w))


# ---- values in the R' form (x * 2^261 mod p)
def _P():
    import pyref
    return pyref


def rp(v):
    P = _P()
    return v * (1 << 261) % P.Q_MOD


def unrp(v):
    P = _P()
    return v * pow(1 << 261, -1, P.Q_MOD) % P.Q_MOD


def top_rep(r, V):
    """the largest representative r + k p below V p"""
    P = _P()
    return r + int((V * P.Q_MOD - r) // P.Q_MOD) * P.Q_MOD if r < V * P.Q_MOD else r


def std_words(v):
    """canonical standard Montgomery form (v * 2^256 mod p) in 8 x u32"""
    P = _P()
    return words_of(P.fp_to_mont(v))


# ---- accumulator states: a point (x, y) as X = x l^2, Y = y l^3, ZZ = l^2, ZZZ = l^3, every coordinate pushed up by multiples of p to the
# invariant (top = True) or left canonical
def _lam(rng, pred):
    P = _P()
    for _ in range(20000):
        l = int(rng.integers(1, 1 << 62)) * int(rng.integers(1, 1 << 62)) * int(rng.integers(1, 1 << 62)) % P.Q_MOD
        if l and pred(l):
            return l
    raise AssertionError("no scale factor found")


def g1_state(pt, rng, inv, top=True, weak_x=True):
    """pt = pyref affine G1 point; inv = {coord: (V, L)}; returns 36 limbs"""
    P = _P(); p = P.Q_MOD
    # ZZ and ZZZ both below (V - 1) p in the R' form, so that their top representatives reach the invariant
    lim = {k: (inv[k][0] - 1) * p for k in ("ZZ", "ZZZ")}
    l = _lam(rng, lambda l: not top or (rp(l * l % p) < lim["ZZ"] and rp(l * l * l % p) < lim["ZZZ"]))
    zz = l * l % p; zzz = zz * l % p
    vals = {"X": rp(pt[0] * zz % p), "Y": rp(pt[1] * zzz % p), "ZZ": rp(zz), "ZZZ": rp(zzz)}
    out = []
    for k in ("X", "Y", "ZZ", "ZZZ"):
        v = top_rep(vals[k], inv[k][0]) if top else vals[k]
        out += weak_limbs(v) if (k == "X" and weak_x and inv[k][1] > 29) else limbs_of(v)
    return out


def g2_state(pt, rng, inv, top=True, weak_x=True):
    """pt = pyref affine G2 point ((x0, x1), (y0, y1)); returns 72 limbs (component c: a0 | a1)"""
    P = _P(); p = P.Q_MOD
    lim = {k: (inv[k][0] - 1) * p for k in ("ZZ", "ZZZ")}
    def ok(l):
        zz = P.fp2_sqr(l); zzz = P.fp2_mul(zz, l)
        return all(rp(c) < lim["ZZ"] for c in zz) and all(rp(c) < lim["ZZZ"] for c in zzz)
    for _ in range(200000):
        l = (int(rng.integers(0, 1 << 62)) ** 4 % p, int(rng.integers(0, 1 << 62)) ** 4 % p)
        if l != (0, 0) and (not top or ok(l)):
            break
    else:
        raise AssertionError("no scale factor found")
    zz = P.fp2_sqr(l); zzz = P.fp2_mul(zz, l)
    vals = {"X": P.fp2_mul(pt[0], zz), "Y": P.fp2_mul(pt[1], zzz), "ZZ": zz, "ZZZ": zzz}
    out = []
    for k in ("X", "Y", "ZZ", "ZZZ"):
        for c in vals[k]:
            v = top_rep(rp(c), inv[k][0]) if top else rp(c)
            out += weak_limbs(v) if (k == "X" and weak_x and inv[k][1] > 29) else limbs_of(v)
    return out


def g1_affine_of(limbs36):
    P = _P(); p = P.Q_MOD
    X, Y, ZZ, ZZZ = (unrp(val(limbs36[9 * k: 9 * k + 9])) for k in range(4))
    return (X * P.fp_inv(ZZ) % p, Y * P.fp_inv(ZZZ) % p)


def g2_affine_of(limbs72):
    P = _P()
    c = [(unrp(val(limbs72[18 * k: 18 * k + 9])), unrp(val(limbs72[18 * k + 9: 18 * k + 18]))) for k in range(4)]
    return (P.fp2_mul(c[0], P.fp2_inv(c[2])), P.fp2_mul(c[1], P.fp2_inv(c[3])))


def packed_state(limbs, ncomp):
    """limbs of normalised coordinates below 2^256 -> the packed words of a stored partial sum"""
    out = []
    for k in range(ncomp):
        out += words_of(val(limbs[9 * k: 9 * k + 9]))
    return out


def record(state=(), operand=(), inf=False, negate=False):
    r = np.zeros(IN_W, np.uint32)
    r[:len(state)] = state
    r[OPERAND:OPERAND + len(operand)] = operand
    r[FLAGS] = int(inf) | (int(negate) << 1)
    return r


# ---- group-step cases: (name, op, record, expected affine point or None)
def group_cases(seed=5, per_kind=4):
    import cref
    from helpers import g1_pts, g2_pts
    P = _P(); fb = bounds()
    rng = np.random.default_rng(seed)
    cases = []
    g1 = g1_pts(cref.gen_g1(4 * per_kind + 4, seed + 100))
    g2 = g2_pts(cref.gen_g2(4 * per_kind + 4, seed + 200))
    for curve, pts, st_fn, inv, inv_b, madd, add, ng, addf, ncomp, pk in (
            ("g1", g1, g1_state, fb.G1_ACC, fb.G1_LOADED, G1_MADD, G1_ADD, P.g1_neg, P.g1_add, 4, lambda pt: [w for c in pt for w in words_of(rp(c))]),
            ("g2", g2, g2_state, fb.G2_ACC, fb.G2_STORED, G2_MADD, G2_ADD, P.g2_neg, P.g2_add, 8,
             lambda pt: [w for c in (pt[0][0], pt[0][1], pt[1][0], pt[1][1]) for w in words_of(rp(c))])):
        for i in range(per_kind):
            A, Q = pts[2 * i], pts[2 * i + 1]
            top = i % 2 == 0 or i == per_kind - 1
            sa = st_fn(A, rng, inv, top=top, weak_x=i != 1)
            # mixed additions: generic, negated operand, equal x (doubling, and doubling through a negation), opposite (cancellation, both ways),
            # an infinite operand, an infinite accumulator
            for nm, q, neg, want in (("generic", Q, False, addf(A, Q)), ("negated", Q, True, addf(A, ng(Q))),
                                     ("doubling", A, False, addf(A, A)), ("doubling_negated", ng(A), True, addf(A, A)),
                                     ("cancel", ng(A), False, None), ("cancel_negated", A, True, None),
                                     ("inf_operand", None, False, A)):
                cases.append((f"{curve}_madd_{nm}_{i}", madd, record(sa, [] if q is None else pk(q), negate=neg), want))
            cases.append((f"{curve}_madd_inf_acc_{i}", madd, record([0] * (9 * ncomp), pk(Q), inf=True), Q))
            cases.append((f"{curve}_madd_inf_acc_negated_{i}", madd, record([0] * (9 * ncomp), pk(Q), inf=True, negate=True), ng(Q)))
            # full additions of a loaded / stored partial sum (normalised, at its own invariant)
            def stored(pt):
                return packed_state(st_fn(pt, rng, inv_b, top=top, weak_x=False), ncomp)
            for nm, b, want in (("generic", Q, addf(A, Q)), ("negated", ng(Q), addf(A, ng(Q))), ("doubling", A, addf(A, A)),
                                ("cancel", ng(A), None), ("inf_operand", None, A)):
                cases.append((f"{curve}_add_{nm}_{i}", add, record(sa, [0] * (8 * ncomp) if b is None else stored(b)), want))
            cases.append((f"{curve}_add_inf_acc_{i}", add, record([0] * (9 * ncomp), stored(Q), inf=True), Q))
            # the partial sum a level stores
            store = G1_STORE if curve == "g1" else G2_STORE
            cases.append((f"{curve}_store_{i}", store, record(sa), A))
        cases.append((f"{curve}_store_inf", G1_STORE if curve == "g1" else G2_STORE, record([0] * (9 * ncomp), inf=True), None))
    return cases


# ---- random edge operands of the product primitives (vectorised): limbs 0..7 drawn from {0, random, 2^29 - 1, the limb cap}, the top limb
# from {0, random, its maximum under the value bound V}
def edge_operands(rng, n, cap, V):
    import pyref
    top_max = (V * pyref.Q_MOD >> 232) - 1 - (cap >> 29)     # value < 2^232 (top + 1 + cap / 2^29) <= V p
    kind = rng.integers(0, 4, (n, 8))
    low = np.where(kind == 0, 0, np.where(kind == 1, rng.integers(0, cap + 1, (n, 8)), np.where(kind == 2, M29, cap)))
    tk = rng.integers(0, 3, n)
    top = np.where(tk == 0, 0, np.where(tk == 1, rng.integers(0, top_max + 1, n), top_max))
    return np.concatenate([low, top[:, None]], axis=1).astype(np.uint32)


def product_records(op, n, seed):
    """n records of op (MUL, SQR, MUL2, MUL4) whose operands sit on the edges of the product's contract (field29.cuh)"""
    rng = np.random.default_rng(seed)
    W = (1 << 29) + 7
    r = np.zeros((n, IN_W), np.uint32)
    if op == MUL:       # L + L <= 60: weak x weak, or limbs < 2^31 x normalised (either side); V up to 8 x 8
        half = n // 2
        r[:half, 0:9] = edge_operands(rng, half, W, 8); r[:half, 9:18] = edge_operands(rng, half, W, 8)
        big, nrm = edge_operands(rng, n - half, (1 << 31) - 1, 8), edge_operands(rng, n - half, M29, 8)
        sw = rng.integers(0, 2, n - half).astype(bool)[:, None]
        r[half:, 0:9] = np.where(sw, big, nrm); r[half:, 9:18] = np.where(sw, nrm, big)
    elif op == SQR:     # 2 L <= 60: limbs < 2^30
        r[:, 0:9] = edge_operands(rng, n, (1 << 30) - 1, 8)
    elif op == MUL2:    # L + L <= 59 per pair: limbs < 2^30 x normalised, or weak x weak
        for k in range(2):
            a, b = 18 * k, 18 * k + 9
            sw = rng.integers(0, 3, n)[:, None]
            x30, x29, w1, w2 = (edge_operands(rng, n, c, 8) for c in ((1 << 30) - 1, M29, W, W))
            r[:, a:a + 9] = np.where(sw == 0, x30, np.where(sw == 1, x29, w1))
            r[:, b:b + 9] = np.where(sw == 0, x29, np.where(sw == 1, x30, w2))
    elif op == MUL4:    # every operand weakly normalised
        for k in range(8):
            r[:, 9 * k:9 * k + 9] = edge_operands(rng, n, W, 8)
    else:
        raise ValueError(op)
    return r


def product_value(op, rec):
    """what the result of a product record must equal mod p"""
    import pyref
    p = pyref.Q_MOD; ri = pow(1 << 261, -1, p)
    o = [val(rec[9 * k: 9 * k + 9]) for k in range(8)]
    s = {MUL: o[0] * o[1], SQR: o[0] * o[0], MUL2: o[0] * o[1] + o[2] * o[3], MUL4: o[0] * o[1] + o[2] * o[3] + o[4] * o[5] + o[6] * o[7]}[op]
    return s * ri % p, s


def _limb_ok(limbs, L):
    cap = M29 + 8 if L > 29 else M29
    return all(int(x) <= cap for x in limbs[:8])


def check_group_outputs(cases, outs):
    """every group-step output against pyref (affine), inside the accumulator invariant of tools/f29_bounds.py; failures name the case"""
    fb = bounds(); P = _P()
    bad = []
    for (name, op, rec, want), out in zip(cases, outs):
        out = [int(x) for x in out]
        try:
            if op in (G1_STORE, G2_STORE):
                nc = 4 if op == G1_STORE else 8
                words = out[40:72] if op == G1_STORE else out[0:64]
                if rec[FLAGS] & 1:
                    assert not any(words), "stored infinity is not all zero"
                    continue
                for k in range(nc):
                    assert words_val(words[8 * k: 8 * k + 8]) % P.Q_MOD == val(rec[9 * k: 9 * k + 9]) % P.Q_MOD, f"stored coordinate {k}"
                if op == G1_STORE:
                    assert not out[OUT_INF] and g1_affine_of(out[:36]) == want
                    for k, (c, (V, L)) in enumerate(fb.G1_LOADED.items()):
                        assert val(out[9 * k: 9 * k + 9]) < V * P.Q_MOD and _limb_ok(out[9 * k:], 29), f"loaded {c}"
                continue
            if want is None:
                assert out[OUT_INF] == 1, "expected the point at infinity"
                continue
            assert out[OUT_INF] == 0, "unexpected infinity"
            g2 = op in (G2_MADD, G2_ADD)
            got = g2_affine_of(out[:72]) if g2 else g1_affine_of(out[:36])
            assert got == want, "affine result differs from pyref"
            inv = fb.G2_ACC if g2 else fb.G1_ACC
            per = 2 if g2 else 1
            for k, (c, (V, L)) in enumerate(inv.items()):
                for j in range(per):
                    o = 9 * (per * k + j)
                    assert val(out[o:o + 9]) < V * P.Q_MOD and _limb_ok(out[o:], L), f"{c} leaves the invariant"
        except AssertionError as e:
            bad.append(f"{name}: {e}")
    return bad


def run_group_cases(so, cases):
    outs = np.zeros((len(cases), OUT_W), np.uint32)
    for op in sorted({c[1] for c in cases}):
        idx = [i for i, c in enumerate(cases) if c[1] == op]
        out, err = run_emu(so, op, np.stack([cases[i][2] for i in idx]), [cases[i][0] for i in idx])
        assert err is None, f"host build trapped or failed: {err}"
        outs[idx] = out
    return outs


# ---- fixed edge records of the primitives (ops 0..16): what test_limb29_primitives_at_their_documented_bounds checks on the host, as records
def primitive_edge_records():
    import pyref
    p = pyref.Q_MOD
    W = (1 << 29) + 7
    def weak_max(V):
        l = [W] * 8 + [0]
        l[8] = (V * p - val(l)) >> 232
        return l
    def rec(*ops):
        r = np.zeros(IN_W, np.uint32)
        for k, o in enumerate(ops):
            r[9 * k: 9 * k + len(o)] = o
        return r
    big = [(1 << 31) - 1] * 8 + [1 << 20]
    e8 = [weak_max(8), limbs_of(8 * p - 1), limbs_of(0), limbs_of(p), limbs_of(7 * p), limbs_of(1)]
    out = {}
    out[MUL] = [rec(a, b) for a in e8 for b in e8] + [rec(big, limbs_of(8 * p - 1)), rec(limbs_of(2 * p), big)]
    out[SQR] = [rec(a) for a in e8] + [rec([(1 << 30) - 1] * 8 + [1 << 20])]
    out[MUL2] = [rec(a, b, b, a) for a in e8 for b in e8]
    out[MUL4] = [rec(*([a, b] * 4)) for a in e8 for b in e8] + [rec(*[limbs_of(k * p) for k in range(1, 9)])]
    out[SUB8] = [rec(a, b) for a in e8 for b in (weak_max(7), limbs_of(0), limbs_of(7 * p))]
    out[SUB4] = [rec(a, b) for a in e8 for b in (weak_max(3), limbs_of(0), limbs_of(3 * p))]
    out[SUB2] = [rec(a, b) for a in e8 for b in (weak_max(1), limbs_of(0), limbs_of(p))]
    out[WNORM] = [rec([(1 << 31) - 1] * 9), rec(weak_max(8))]
    out[NORM] = [rec(big), rec([M29 + 1] * 8 + [5]), rec(weak_max(8))]
    out[CONDSUB4] = [rec(limbs_of(v)) for v in (0, p, 4 * p - 1, 4 * p, 4 * p + (1 << 233), 8 * p - 1)] + [rec(weak_max(8))]
    out[CONDSUB2] = [rec(limbs_of(v)) for v in (0, p, 2 * p - 1, 2 * p, 2 * p + (1 << 233), 4 * p - 1)] + [rec(weak_max(4))]
    words = [(1 << 256) - 1, 0, p, p - 1, 5 * p, (1 << 232) - 1, 1 << 232, 1 << 255]
    out[UNPACK] = [rec(words_of(v)) for v in words]
    out[PACK] = [rec(limbs_of(v)) for v in words]
    out[TO_STD] = [rec(weak_max(128)), rec(limbs_of(128 * p - 1)), rec(limbs_of(0)), rec(limbs_of(p)), rec(weak_max(1))]
    out[FROM_STD] = [rec(words_of(v)) for v in (0, 1, p - 1, p // 2)]
    out[BELOW_2P] = [rec(limbs_of(v)) for v in (0, 2 * p, 4 * p - 1, 4 * p, 6 * p, int(6.1 * p) - 1, 2 * p + (1 << 232))] + [rec(weak_max(6))]
    zn = [limbs_of(v) for v in (0, p, 2 * p, 1, p + 1, 2 * p - 1, int(2.09 * p))]
    out[F2_IS_ZERO] = [rec(a, b) for a in zn for b in zn]
    return {op: np.stack(v) for op, v in out.items()}


# ---- the host build, one record at a time, in a child process
def run_emu(so, op, recs, names=None):
    """(outputs, None) or (outputs so far, name of the record that trapped / failed)"""
    import tempfile
    recs = np.ascontiguousarray(recs, dtype=np.uint32).reshape(-1, IN_W)
    with tempfile.TemporaryDirectory() as td:
        fi, fo, fp = (os.path.join(td, f) for f in ("in.npy", "out.npy", "progress.npy"))
        np.save(fi, recs)
        np.save(fo, np.zeros((len(recs), OUT_W), np.uint32)); np.save(fp, np.zeros(1, np.int64))
        res = subprocess.run([sys.executable, os.path.abspath(__file__), so, str(op), fi, fo, fp], capture_output=True, text=True, timeout=600)
        out = np.load(fo); done = int(np.load(fp)[0])
    if res.returncode == 0 and done == len(recs):
        return out, None
    bad = names[done] if names is not None and done < len(recs) else f"record {done}"
    return out, f"{bad} (op {op}, exit status {res.returncode}: {res.stderr.strip()[-300:]})"


def _child(so, op, fi, fo, fp):
    import ctypes as C
    lib = C.CDLL(so)
    recs = np.load(fi)
    out = np.load(fo, mmap_mode="r+"); prog = np.load(fp, mmap_mode="r+")
    row = np.zeros(OUT_W, np.uint32)
    for i in range(len(recs)):
        r = np.ascontiguousarray(recs[i])
        if lib.emu_limb29_op(C.c_int(op), row.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), C.c_size_t(1)) != 0:
            sys.exit(3)
        out[i] = row
        prog[0] = i + 1
    out.flush(); prog.flush()


if __name__ == "__main__":
    _child(sys.argv[1], int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5])

"""Records of gnark-whir_amd/csrc/shape_ops.cuh -- the field arithmetic on operands the compiler can see through (literal factors, limbs
that are provably zero, one value in two places, results over inputs, chains that start at a literal) -- for the host build (tests/emu
emu_field_shape, overflow traps on) and the device (mi_debug_field_shape_dev), and their reference.

The reference never calls the code under test.  Field shapes come from Python integers on the raw Montgomery residues: with R = 2^256 a
product is x y / R mod p (pow, %), fe_mul_lazy the exact integer (x y + m p) / R, the 29-bit products the exact (s + m p) / 2^261; the
curve, Fp2 and Fp12 shapes come from oracle/pyref.py and tests/pairing_ref.py on the canonical values.

Per shape RECORDS = 130 records.  Field shapes: the pairs of adversarial_mont_pairs (tests/test_device_headers_on_host.py: limbs of
0xFFFFFFFF where a column's first product sits), every pair out of 0, 1, p - 1, p - 2 and the largest value below p whose low seven words
are all 0xFFFFFFFF (so that the words a shape keeps are all ones), and seeded random values; u and v walk the same pool.  Curve shapes:
seeded points with infinity, equal and opposite operands among them.  29-bit shapes: limb29_cases.edge_operands (weakly normalised limbs,
values up to 8 p).

Run as a script it is the child process of run_emu: python shape_cases.py <libemu.so> <shape> <in.npy> <out.npy> <progress.npy>"""
import os
import subprocess
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
IN_W, OUT_W = 32, 32
RECORDS = 130
R_ = 1 << 256

# the enums of shape_ops.cuh, in order
GENERIC = ["mul_one", "mul_r2", "mul_unit", "mul_u32", "mul_pm1", "zero_lo1", "zero_lo2", "zero_lo4", "zero_hi4", "zero_mid1", "u128_chain",
           "sqr", "inplace", "mul2_same", "mul2_lit", "mul_sub_same", "lazy_lit", "pow5", "inv", "lagrange",
           "add_lit", "sub_lit", "lazy_add_lit", "lazy_x"]
ZERO_FORMS = ["zero_lo1", "zero_lo2", "zero_lo4", "zero_hi4", "zero_mid1"]
GENERIC += [f"{f}_alone_{s}" for f in ZERO_FORMS for s in ("left", "right", "both", "to_mont")]   # SHG_ZERO_ALONE + 4 f + s
TYPED = ["g1_madd", "g2_madd", "g1_inf_add", "g2_inf_add", "g1_dbl_inf", "g2_dbl_inf", "g1x29_chain",
         "fp2_half_zero", "fp2_mul_one", "fp2_xi", "fp2_real", "fp2_sqr", "fp2_mul_sub",
         "f29_one", "f29_zero_upper", "f29_twice", "fp12_mul_one", "fp12_line_first", "fp12_sqr_one"]
SHG_END, SHT_END = len(GENERIC), len(TYPED)
OP_END = 2 * SHG_END + SHT_END
NAMES = [f"fr-{g}" for g in GENERIC] + [f"fp-{g}" for g in GENERIC] + TYPED
KEEP = {"zero_lo1": (0, 1), "zero_lo2": (0, 2), "zero_lo4": (0, 4), "zero_hi4": (4, 8), "zero_mid1": (3, 4)}


def shape_id(name):
    return NAMES.index(name)


def build_emu(so):
    src = os.path.join(HERE, "emu", "emu.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DMI_CHECK_NOWRAP", "-shared", "-fPIC", "-o", so, src])
    return so


def _P():
    import pyref
    return pyref


def words_of(v):
    assert 0 <= v < R_
    return [(v >> (32 * k)) & 0xFFFFFFFF for k in range(8)]


def words_val(w):
    return sum(int(x) << (32 * k) for k, x in enumerate(w))


# ---------------------------------------------------------------------------------------------------- field shapes
def all_ones_below(mod):
    """the largest value below mod whose low seven words are all 0xFFFFFFFF"""
    v = (((mod >> 224) - 1) << 224) | ((1 << 224) - 1)
    assert v < mod
    return v


def field_operands(mod, seed):
    """RECORDS tuples (x, y, u, v) of raw Montgomery residues below mod"""
    from test_device_headers_on_host import adversarial_mont_pairs
    P = _P()
    xs, ys = adversarial_mont_pairs(mod, seed, n_per=5)
    assert len(xs) == 65
    edge = [0, 1, mod - 1, mod - 2, all_ones_below(mod)]
    for a in edge:
        for b in edge:
            xs.append(a); ys.append(b)
    rng = P.SplitMix64(1000 + seed)
    while len(xs) < RECORDS:
        xs.append(rng.fr() % mod); ys.append(rng.fr() % mod)
    n = len(xs)
    assert n == RECORDS and all(0 <= v < mod for v in xs + ys)
    return [(xs[i], ys[i], xs[(7 * i + 3) % n], ys[(11 * i + 5) % n]) for i in range(n)]


def ref_generic(name, mod, x, y, u, v):
    """-> up to four integers, the results o0 .. o3"""
    ri = pow(R_, -1, mod)
    one, r2 = R_ % mod, R_ * R_ % mod
    mm = lambda a, b: a * b * ri % mod
    def lazy(a, b):
        m = (-a * b * pow(mod, -1, R_)) % R_
        t = a * b + m * mod
        assert t % R_ == 0 and t // R_ < 2 * mod
        return t // R_
    minv = lambda a: r2 * pow(a, -1, mod) % mod if a else 0   # the Montgomery form of 1 / (a / R); 0 -> 0 as fe_inv
    if name == "mul_one":
        return [mm(x, one), mm(one, x), 0, 0]
    if name == "mul_r2":
        return [mm(x, r2)] * 3
    if name == "mul_unit":
        return [mm(x, 1)] * 3
    if name == "mul_u32":
        k = {c: mm(c, r2) for c in (2, 3, 9)}
        return [mm(x, k[2]), mm(x, k[3]), mm(x, k[9]), mm(k[3], k[9])]
    if name == "mul_pm1":
        return [mm(x, mod - 1), mm(mod - 1, x), mm(mod - 1, mod - 1)]
    if name in KEEP or "_alone_" in name:
        lo, hi = KEEP[name.split("_alone_")[0]]
        mask = ((1 << (32 * hi)) - 1) ^ ((1 << (32 * lo)) - 1)
        kx, ky = x & mask, y & mask
        res = [mm(kx, y), mm(y, kx), mm(kx, ky), mm(kx, r2)]
        return res if name in KEEP else [res[("left", "right", "both", "to_mont").index(name.split("_alone_")[1])]]
    if name == "u128_chain":
        pw = mm(x & ((1 << 128) - 1), r2)
        out = []
        for _ in range(3):
            out.append(mm(pw, 1)); pw = mm(pw, y)
        return out + [pw]
    if name == "sqr":
        return [mm(x, x)] * 2
    if name == "inplace":
        c = x
        for _ in range(3):
            c = mm(c, c)
        return [mm(x, y), mm(x, y), c]
    if name == "mul2_same":
        return [2 * x * y * ri % mod, 2 * x * x * ri % mod, 2 * x * y * ri % mod]
    if name == "mul2_lit":
        return [mm(x, y), (x * y + u * one) * ri % mod, mm(x, y)]
    if name == "mul_sub_same":
        return [0, (x * x - y * y) * ri % mod]
    if name == "lazy_lit":
        return [lazy(x, one), lazy(x, mod - 1), lazy(x, r2)]
    if name == "pow5":
        return [pow(x, 5, mod) * pow(ri, 4, mod) % mod]
    if name == "inv":
        return [minv(x)]
    if name == "lagrange":
        d = [(x - t) % mod for t in (y, u, v)]
        if not all(d):   # the run's product is zero: fe_inv gives 0 and every row comes out 0
            return [0, 0, 0, 0]
        return [minv(t) for t in d] + [one]
    if name == "add_lit":
        return [x, (x + one) % mod, (mod - 1 + x) % mod, 2 * x % mod]
    if name == "sub_lit":
        return [-x % mod, 0, 0, mod]
    if name == "lazy_add_lit":
        return [x, 2 * mod, 0, 0]
    if name == "lazy_x":
        return [x, x, 2 * x, 3 * x % mod]
    raise ValueError(name)


# ---------------------------------------------------------------------------------------------------- curve shapes
def _mont(c):
    return c * R_ % _P().Q_MOD


def _g1_words(pt):
    return [0] * 16 if pt is None else words_of(_mont(pt[0])) + words_of(_mont(pt[1]))


def _g2_words(pt):
    return [0] * 32 if pt is None else sum((words_of(_mont(c)) for c in (pt[0][0], pt[0][1], pt[1][0], pt[1][1])), [])


def _g1_rp_words(pt):
    q = _P().Q_MOD
    return [0] * 16 if pt is None else words_of(pt[0] * (1 << 261) % q) + words_of(pt[1] * (1 << 261) % q)


def _points(seed, n, g2=False):
    P = _P()
    rng = P.SplitMix64(seed)
    return [(P.g2_mul(P.G2_GEN, 1 + rng.below(1 << 40)) if g2 else P.g1_mul(P.G1_GEN, 1 + rng.below(1 << 62))) for _ in range(n)]


def _g1_pairs(seed):
    """RECORDS pairs (a, b): infinity on either side and on both, b = a, b = -a, and distinct points"""
    P = _P()
    pts = _points(seed, RECORDS + 1)
    out = []
    for i in range(RECORDS):
        a, b = pts[i], pts[i + 1]
        kind = i % 13 if i < 65 else 12
        out.append({0: (None, None), 1: (None, b), 2: (a, None), 3: (a, a), 4: (a, P.g1_neg(a))}.get(kind, (a, b)))
    return out


def _g2_singles(seed):
    pts = _points(seed, 12, g2=True)
    return [None if i % 16 == 0 else pts[i % len(pts)] for i in range(RECORDS)]


def typed_records(name):
    """-> (in records, expected out records) of a typed shape"""
    P = _P(); q = P.Q_MOD
    rin = np.zeros((RECORDS, IN_W), np.uint32)
    want = np.zeros((RECORDS, OUT_W), np.uint32)
    if name in ("g1_madd", "g1x29_chain"):
        for i, (a, b) in enumerate(_g1_pairs(31 if name == "g1_madd" else 37)):
            enc = _g1_words if name == "g1_madd" else _g1_rp_words
            rin[i] = enc(a) + enc(b)
            want[i, :16] = _g1_words(P.g1_add(a, b))
    elif name == "g1_inf_add":
        rng = P.SplitMix64(41)
        for i, a in enumerate(_points(43, RECORDS)):
            if i % 16 == 0:      # infinity: ZZ = 0, as XYZZ::inf() writes it and as all zero words
                rin[i] = (words_of(_mont(1)) * 2 + [0] * 16) if i % 32 == 0 else [0] * 32
                continue
            l = 1 if i % 16 == 1 else 1 + rng.fr() % (q - 1)
            zz, zzz = l * l % q, l * l * l % q
            rin[i] = sum((words_of(_mont(c)) for c in (a[0] * zz % q, a[1] * zzz % q, zz, zzz)), [])
            want[i, :16] = _g1_words(P.g1_add(a, a))
    elif name == "g1_dbl_inf":
        other = _g1_words(_points(48, 1)[0])
        for i, a in enumerate(_points(47, RECORDS)):
            a = None if i % 16 == 0 else a
            rin[i, :16] = _g1_words(a)
            rin[i, 16:] = other   # u | v are not read
            want[i, 16:] = _g1_words(a)
    elif name in ("g2_madd", "g2_inf_add", "g2_dbl_inf"):
        memo = {}
        for i, a in enumerate(_g2_singles({"g2_madd": 51, "g2_inf_add": 53, "g2_dbl_inf": 57}[name])):
            rin[i] = _g2_words(a)
            if a not in memo:
                a2 = P.g2_add(a, a)
                memo[a] = {"g2_madd": P.g2_add(a2, a), "g2_inf_add": a2, "g2_dbl_inf": a}[name]
            want[i] = _g2_words(memo[a])
    elif name.startswith("fp2_") or name.startswith("fp12_"):
        ri = pow(R_, -1, q)
        for i, (x, y, u, v) in enumerate(field_operands(q, 61)):
            rin[i] = words_of(x) + words_of(y) + words_of(u) + words_of(v)
            cx, cy, cu, cv = (t * ri % q for t in (x, y, u, v))
            res = _ref_tower(name, cx, cy, cu, cv)
            want[i, :8 * len(res)] = sum((words_of(_mont(c)) for c in res), [])
    elif name.startswith("f29_"):
        import limb29_cases as L29
        rng = np.random.default_rng(71 + TYPED.index(name))
        W = (1 << 29) + 7
        a, b = L29.edge_operands(rng, RECORDS, W, 8), L29.edge_operands(rng, RECORDS, W, 8)
        a[0] = 0; b[1] = 0; a[2] = L29.limbs_of(q - 1); b[2] = L29.limbs_of(q - 1)
        rin[:, 0:9] = a; rin[:, 9:18] = b
        one = (1 << 261) % q
        def prod(s):   # the exact representative a product leaves: (s + m p) / 2^261, m = -s / p mod 2^261, normalised limbs
            m = (-s * pow(q, -1, 1 << 261)) % (1 << 261)
            t = s + m * q
            assert t % (1 << 261) == 0
            z = t >> 261
            assert z >> 232 < 1 << 29
            return L29.limbs_of(z)
        for i in range(RECORDS):
            va, vb = L29.val(a[i]), L29.val(b[i])
            ka = L29.val(list(a[i][:4]) + [0] * 5)
            res = {"f29_one": (va * one, one * va, one * one), "f29_zero_upper": (ka * vb, vb * ka, ka * ka),
                   "f29_twice": (va * va, va * va, ka * ka)}[name]
            want[i, :27] = sum((prod(s) for s in res), [])
    else:
        raise ValueError(name)
    return rin, want


def _ref_tower(name, x, y, u, v):
    """Fp2 / Fp12 shapes on canonical values -> the canonical Fp results in output order"""
    import pairing_ref as PR
    P = _P(); q = P.Q_MOD
    X, Y = (x, y), (u, v)
    flat = lambda *es: [c for e in es for c in e]
    if name == "fp2_half_zero":
        return flat(P.fp2_mul(X, (u, 0)), P.fp2_mul(X, (0, v)))
    if name == "fp2_mul_one":
        return flat(P.fp2_mul(X, P.FP2_ONE), P.fp2_mul(P.FP2_ONE, X))
    if name == "fp2_xi":
        return flat(P.fp2_mul(X, (9, 1)), (9, 1))
    if name == "fp2_real":
        return [x * x % q, 0, pow(x, -1, q) if x else 0, 0]
    if name == "fp2_sqr":
        return flat(P.fp2_mul(X, X), P.fp2_sqr(X))
    if name == "fp2_mul_sub":
        return flat(P.fp2_sub(P.fp2_mul(X, Y), P.fp2_mul(X, X)), (0, 0))
    fold = lambda z, k: [sum(z[j::k]) % q for j in range(k)]
    if name == "fp12_mul_one":
        f = [x, y, u, v, y, x, v, u, x, u, y, v]
        return fold(PR.to_tower(PR.f_mul(PR.from_tower(f), PR.ONE)), 4)
    if name == "fp12_line_first":
        line = [x, y, 0, 0, 0, 0, u, v, y, u, 0, 0]   # l0 at C0.B0, l3 at C1.B0, l4 at C1.B1
        return fold(PR.to_tower(PR.f_mul(PR.ONE, PR.from_tower(line))), 4)
    if name == "fp12_sqr_one":
        z = PR.to_tower(PR.f_mul(PR.ONE, PR.ONE))
        return fold(z, 2) * 2
    raise ValueError(name)


# ---------------------------------------------------------------------------------------------------- records
_CACHE = {}


def records(shape):
    """-> (in records (RECORDS, 32) uint32, expected out records (RECORDS, 32) uint32), built once per shape, read-only"""
    if shape not in _CACHE:
        P = _P()
        if shape < 2 * SHG_END:
            field, g = divmod(shape, SHG_END)
            mod = (P.R_MOD, P.Q_MOD)[field]
            ops = field_operands(mod, 77 + field)
            rin = np.zeros((RECORDS, IN_W), np.uint32)
            want = np.zeros((RECORDS, OUT_W), np.uint32)
            for i, (x, y, u, v) in enumerate(ops):
                rin[i] = words_of(x) + words_of(y) + words_of(u) + words_of(v)
                res = ref_generic(GENERIC[g], mod, x, y, u, v)
                want[i, :8 * len(res)] = sum((words_of(r) for r in res), [])
        else:
            rin, want = typed_records(TYPED[shape - 2 * SHG_END])
        assert rin.shape == (RECORDS, IN_W) and want.shape == (RECORDS, OUT_W)
        rin.setflags(write=False); want.setflags(write=False)
        _CACHE[shape] = (rin, want)
    return _CACHE[shape]


def describe(shape, rin, idx):
    return [f"{NAMES[shape]} record {int(i)}: in = {' '.join(f'{int(w):08x}' for w in rin[int(i)])}" for i in idx]


# ---------------------------------------------------------------------------------------------------- the host build, in a child process
def run_emu(so, shape, recs):
    """(outputs, None) or (outputs so far, (index of the record that trapped / failed, how))"""
    import tempfile
    recs = np.ascontiguousarray(recs, dtype=np.uint32).reshape(-1, IN_W)
    with tempfile.TemporaryDirectory() as td:
        fi, fo, fp = (os.path.join(td, f) for f in ("in.npy", "out.npy", "progress.npy"))
        np.save(fi, recs)
        np.save(fo, np.zeros((len(recs), OUT_W), np.uint32)); np.save(fp, np.zeros(1, np.int64))
        res = subprocess.run([sys.executable, os.path.abspath(__file__), so, str(shape), fi, fo, fp], capture_output=True, text=True, timeout=600)
        out = np.load(fo); done = int(np.load(fp)[0])
    if res.returncode == 0 and done == len(recs):
        return out, None
    return out, (done, f"record {done} (shape {NAMES[shape]}, exit status {res.returncode}: {res.stderr.strip()[-300:]})")


def _child(so, shape, fi, fo, fp):
    import ctypes as C
    lib = C.CDLL(so)
    recs = np.load(fi)
    out = np.load(fo, mmap_mode="r+"); prog = np.load(fp, mmap_mode="r+")
    row = np.zeros(OUT_W, np.uint32)
    for i in range(len(recs)):
        r = np.ascontiguousarray(recs[i])
        if lib.emu_field_shape(C.c_int(shape), row.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), C.c_size_t(1)) != 0:
            sys.exit(3)
        out[i] = row
        prog[0] = i + 1
    out.flush(); prog.flush()


if __name__ == "__main__":
    _child(sys.argv[1], int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5])

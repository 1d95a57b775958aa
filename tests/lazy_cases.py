"""Records of gnark-whir_amd/csrc/lazy_ops.cuh for the tests of the NTT's lazy 8 x 32-bit arithmetic (host: tests/emu emu_lazy_op with the
overflow traps on, device: mi_debug_lazy_op_dev), their big-integer reference, and the structured whole-transform inputs (ntt_cases,
compute_h_cases) on which a representative is exactly 0, p, 2p, and two butterfly operands are equal -- what uniform random data never gives.

The reference is Python integers only; nothing in it calls the code under test.  With R = 2^256 and p = r (Fr):
    add_nored  x + y                      sub_plus2p  x - y + 2p                  condsub_2p  x - 2p if x >= 2p else x
    canon      x mod p                    mul_lazy    (x y + m p) / R, m = -x y / p mod R   (exact: every bit of the unreduced product)
and the butterflies, mul_lazy2 and store_sub composed from these as ntt_tile.cuh composes them.  reference() asserts every documented range
on the way (DIF results below 2p, DIT results below 4p, mul_lazy below 2p, canon below p), so the generator itself is checked.

Operands.  EDGE is the list of edge values: 0, 1, p - 1, p, p + 1, 2p - 1, 2p, 2p + 1, 3p - 1, 3p, 4p - 1; per band [kp, (k + 1)p) the values
whose low 1, 2, 4 or 7 limbs are all zero and their predecessors (low limbs all 0xFFFFFFFF): carry and borrow chains of every length up to
all eight limbs once two of them meet; and 2^k, 2^k +- 1 for k = 32, 64, 128, 224, 253, 254, 255 (each lies in one band).  Every op gets the
FULL cross product of EDGE with itself (times every twiddle where it takes one), filtered by the op's documented contract and by nothing
else; _check_coverage() asserts that against bounds written down a second time as plain numbers, so a mistake in the filter cannot empty a
class silently.  On top of that, RANDOM_PER_BAND seeded random values per band, each paired with itself, with every other representative
of its residue that the contract admits (both orders), with a random partner and with an edge value (both orders): the cross product of
all ~900 values with one another would be 10^6 records per op for no further edge.  Every value, edge or random, also meets itself and
every representative of its own residue for sub_plus2p, the butterflies and store_sub.

Run as a script it is the child process of run_emu: python lazy_cases.py <libemu.so> <op> <in.npy> <out.npy> <progress.npy>"""
import os
import subprocess
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

IN_W, OUT_W = 24, 16
ADD_NORED, SUB_PLUS2P, CONDSUB_2P, CANON, MUL_LAZY, MUL_LAZY2, BFLY_DIF, BFLY_DIF_1, BFLY_DIT, BFLY_DIT_1, STORE_SUB = range(11)
OP_END = 11
OP_NAMES = ["add_nored", "sub_plus2p", "condsub_2p", "canon", "mul_lazy", "mul_lazy2", "bfly_dif", "bfly_dif_1", "bfly_dit", "bfly_dit_1", "store_sub"]
P_ = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001   # r, the modulus of Fr
R_ = 1 << 256
PINV = pow(P_, -1, R_)
RANDOM_PER_BAND = 200
# a found bug's operands go here by name: (name, op, x, y, w); records() appends them to the op's cases
NAMED_CASES = []


def build_emu(so):
    src = os.path.join(HERE, "emu", "emu.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DMI_CHECK_NOWRAP", "-shared", "-fPIC", "-o", so, src])
    return so


# ---------------------------------------------------------------------------------------------------- the reference
def ref_add_nored(x, y):
    assert x + y < R_
    return x + y


def ref_sub_plus2p(x, y):
    z = x - y + 2 * P_
    assert 0 <= z < R_
    return z


def ref_condsub_2p(x):
    return x - 2 * P_ if x >= 2 * P_ else x


def ref_canon(x):
    assert x < 4 * P_
    z = x % P_
    assert z < P_
    return z


def ref_mul_lazy(x, y):
    m = (-x * y * PINV) % R_
    t = x * y + m * P_
    assert t % R_ == 0
    z = t // R_
    assert z < 2 * P_ and (z * R_ - x * y) % P_ == 0
    return z


def ref_bfly_dif(x, y, w):
    assert x < 2 * P_ and y < 2 * P_
    u = ref_condsub_2p(ref_add_nored(x, y))
    t = ref_sub_plus2p(x, y)
    assert 0 < t < 4 * P_
    v = ref_mul_lazy(t, w) if w is not None else ref_condsub_2p(t)
    assert u < 2 * P_ and v < 2 * P_
    return u, v


def ref_bfly_dit(x, y, w):
    assert x < 4 * P_ and y < 4 * P_
    a = ref_condsub_2p(x)
    t = ref_mul_lazy(y, w) if w is not None else ref_condsub_2p(y)
    assert a < 2 * P_ and t < 2 * P_
    u, v = ref_add_nored(a, t), ref_sub_plus2p(a, t)
    assert u < 4 * P_ and v < 4 * P_
    return u, v


def reference(op, x, y, w):
    """-> (out0, out1) as integers; out1 is 0 for an op with one result"""
    if op == ADD_NORED:
        return ref_add_nored(x, y), 0
    if op == SUB_PLUS2P:
        z = ref_sub_plus2p(x, y)
        assert 0 < z < 4 * P_
        return z, 0
    if op == CONDSUB_2P:
        z = ref_condsub_2p(x)
        assert z < 2 * P_
        return z, 0
    if op == CANON:
        return ref_canon(x), 0
    if op == MUL_LAZY:
        return ref_mul_lazy(x, y), 0
    if op == MUL_LAZY2:
        return ref_mul_lazy(ref_condsub_2p(x), ref_condsub_2p(y)), 0
    if op == BFLY_DIF:
        return ref_bfly_dif(x, y, w)
    if op == BFLY_DIF_1:
        return ref_bfly_dif(x, y, None)
    if op == BFLY_DIT:
        return ref_bfly_dit(x, y, w)
    if op == BFLY_DIT_1:
        return ref_bfly_dit(x, y, None)
    if op == STORE_SUB:
        return ref_canon(ref_sub_plus2p(ref_condsub_2p(x), ref_condsub_2p(y))), 0
    raise ValueError(op)


# ---------------------------------------------------------------------------------------------------- operands
def _edge_values():
    p = P_
    vals = [0, 1, p - 1, p, p + 1, 2 * p - 1, 2 * p, 2 * p + 1, 3 * p - 1, 3 * p, 4 * p - 1]
    for k in range(4):
        lo, hi = k * p, (k + 1) * p
        for j in (1, 2, 4, 7):
            z = ((hi - 1) >> (32 * j)) << (32 * j)     # the band's largest value whose low j limbs are all zero ...
            for v in (z, z - 1):                       # ... and its predecessor: low j limbs all 0xFFFFFFFF
                if lo <= v < hi:
                    vals.append(v)
    for k in (32, 64, 128, 224, 253, 254, 255):
        vals += [v for v in ((1 << k) - 1, 1 << k, (1 << k) + 1) if v < 4 * p]
    out = []
    for v in vals:
        if v not in out:
            out.append(v)
    return out


def _random_values():
    rng = np.random.default_rng(20260117)
    out = []
    for k in range(4):
        for _ in range(RANDOM_PER_BAND):
            out.append(k * P_ + int.from_bytes(rng.bytes(40), "little") % P_)
    return out


def twiddles():
    """Montgomery 1, Montgomery -1, p - 1, 0 and real entries of the in-tile table small[j] = w_4096^j (Montgomery form), all below p"""
    w4096 = pow(0x2a3c09f0a58a7e8500e0a7eb8ef62abc402d111e41112ed49bd61b6e725b19f0, 1 << 16, P_)   # the 2^28-th root, squared down
    assert pow(w4096, 2048, P_) == P_ - 1
    mont = lambda v: v * R_ % P_
    return [mont(1), mont(P_ - 1), P_ - 1, 0] + [mont(pow(w4096, j, P_)) for j in (1, 1024, 2047)]


EDGE = _edge_values()
RANDOM = _random_values()
TWIDDLES = twiddles()

# the contracts, as the filter applies them: (x, y) -> admissible
_FOUR, _TWO = 4 * P_, 2 * P_
CONTRACT = {
    ADD_NORED: lambda x, y: x < _FOUR and y < _FOUR and x + y < R_,
    SUB_PLUS2P: lambda x, y: x < _TWO and y < _TWO,
    CONDSUB_2P: lambda x, y: x < _FOUR,
    CANON: lambda x, y: x < _FOUR,
    MUL_LAZY: lambda x, y: (x < _FOUR and y < P_) or (x < _TWO and y < _TWO),
    MUL_LAZY2: lambda x, y: x < _FOUR and y < _FOUR,
    BFLY_DIF: lambda x, y: x < _TWO and y < _TWO,
    BFLY_DIF_1: lambda x, y: x < _TWO and y < _TWO,
    BFLY_DIT: lambda x, y: x < _FOUR and y < _FOUR,
    BFLY_DIT_1: lambda x, y: x < _FOUR and y < _FOUR,
    STORE_SUB: lambda x, y: x < _FOUR and y < _FOUR,
}
UNARY = (CONDSUB_2P, CANON)
WITH_TWIDDLE = (BFLY_DIF, BFLY_DIT)
SAME_RESIDUE_OPS = (SUB_PLUS2P, BFLY_DIF, BFLY_DIF_1, BFLY_DIT, BFLY_DIT_1, STORE_SUB)


def _pairs(op):
    """(x, y) of the op, in a fixed order, without repeats"""
    ok = CONTRACT[op]
    if op in UNARY:
        return [(x, 0) for x in EDGE + RANDOM if ok(x, 0)]
    seen, out = set(), []
    def add(x, y):
        if ok(x, y) and (x, y) not in seen:
            seen.add((x, y)); out.append((x, y))
    for x in EDGE:
        for y in EDGE:
            add(x, y)
    for v in EDGE + RANDOM:                                  # itself, and every representative of its residue, both orders
        for k in range(4):
            u = v % P_ + k * P_
            add(v, u); add(u, v)
    rng = np.random.default_rng(7 + op)
    partner = rng.permutation(len(RANDOM))
    for i, v in enumerate(RANDOM):
        u, e = RANDOM[int(partner[i])], EDGE[i % len(EDGE)]
        add(v, u); add(v, e); add(e, v)
        if op == MUL_LAZY:                                   # the second form of the contract: a canonical second factor for the bands above 2p
            add(v, u % P_); add(v, e % P_)
    return out


def cases(op):
    """[(x, y, w)] of the op; w is 0 where the op takes no twiddle"""
    pr = _pairs(op)
    if op in WITH_TWIDDLE:
        ne = sum(1 for x, y in pr if x in _EDGE_SET and y in _EDGE_SET)
        out = []
        for i, (x, y) in enumerate(pr):
            if x in _EDGE_SET and y in _EDGE_SET:
                out += [(x, y, w) for w in TWIDDLES]         # edge pairs: every twiddle
            else:
                out.append((x, y, TWIDDLES[i % len(TWIDDLES)]))
        assert ne
    else:
        out = [(x, y, 0) for x, y in pr]
    out += [(x, y, w) for (_, o, x, y, w) in NAMED_CASES if o == op]
    return out


_EDGE_SET = set(EDGE)
# the same contracts once more as plain per-operand bounds (in units of p), for the coverage check only
_BOUNDS = {ADD_NORED: (4, 4), SUB_PLUS2P: (2, 2), CONDSUB_2P: (4, None), CANON: (4, None), MUL_LAZY2: (4, 4), BFLY_DIF: (2, 2), BFLY_DIF_1: (2, 2),
           BFLY_DIT: (4, 4), BFLY_DIT_1: (4, 4), STORE_SUB: (4, 4)}


def _check_coverage(op, cs):
    have = {}
    for x, y, w in cs:
        have.setdefault((x, y), set()).add(w)
    tw = set(TWIDDLES) if op in WITH_TWIDDLE else {0}
    n = 0
    if op == MUL_LAZY:
        want = [(x, y) for x in EDGE for y in EDGE if (x < 4 * P_ and y < P_) or (x < 2 * P_ and y < 2 * P_)]
    else:
        bx, by = _BOUNDS[op]
        ys = [0] if by is None else [y for y in EDGE if y < by * P_]
        want = [(x, y) for x in EDGE if x < bx * P_ for y in ys if op != ADD_NORED or x + y < R_]
    for xy in want:
        assert have.get(xy, set()) >= tw, (OP_NAMES[op], xy)
        n += 1
    assert n >= (20 if op in UNARY else 400), (OP_NAMES[op], n)
    if op in SAME_RESIDUE_OPS:
        bx = _BOUNDS[op][0]
        for v in EDGE + RANDOM:
            if v < bx * P_:
                for k in range(bx):
                    assert (v, v % P_ + k * P_) in have and (v % P_ + k * P_, v) in have, (OP_NAMES[op], v, k)
    if op == MUL_LAZY:   # both forms of the contract are populated beyond the edge values
        assert sum(1 for x, y in have if x >= 2 * P_ and y < P_) > 400 and sum(1 for x, y in have if x < 2 * P_ and P_ <= y < 2 * P_) > 400


def words_of(v):
    assert 0 <= v < R_
    return [(v >> (32 * k)) & 0xFFFFFFFF for k in range(8)]


def words_val(w):
    return sum(int(x) << (32 * k) for k, x in enumerate(w))


_CACHE = {}


def records(op):
    """-> (cases, in records (n, 24) uint32, expected out records (n, 16) uint32), built once per op"""
    if op not in _CACHE:
        cs = cases(op)
        _check_coverage(op, cs)
        rin = np.zeros((len(cs), IN_W), np.uint32)
        want = np.zeros((len(cs), OUT_W), np.uint32)
        for i, (x, y, w) in enumerate(cs):
            rin[i] = words_of(x) + words_of(y) + words_of(w)
            o0, o1 = reference(op, x, y, w)
            want[i] = words_of(o0) + words_of(o1)
        rin.setflags(write=False); want.setflags(write=False)
        _CACHE[op] = (cs, rin, want)
    return _CACHE[op]


def describe(op, cs, idx):
    return [f"{OP_NAMES[op]}(x={cs[i][0]:#x}, y={cs[i][1]:#x}, w={cs[i][2]:#x})" for i in idx]


# ---------------------------------------------------------------------------------------------------- the host build, in a child process
def run_emu(so, op, recs):
    """(outputs, None) or (outputs so far, index of the record that trapped / failed and how)"""
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
    return out, (done, f"record {done} (op {OP_NAMES[op]}, exit status {res.returncode}: {res.stderr.strip()[-300:]})")


def _child(so, op, fi, fo, fp):
    import ctypes as C
    lib = C.CDLL(so)
    recs = np.load(fi)
    out = np.load(fo, mmap_mode="r+"); prog = np.load(fp, mmap_mode="r+")
    row = np.zeros(OUT_W, np.uint32)
    for i in range(len(recs)):
        r = np.ascontiguousarray(recs[i])
        if lib.emu_lazy_op(C.c_int(op), row.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), C.c_size_t(1)) != 0:
            sys.exit(3)
        out[i] = row
        prog[0] = i + 1
    out.flush(); prog.flush()


# ---------------------------------------------------------------------------------------------------- structured whole-transform inputs
INVERSE, COSET, DIT = 1, 2, 4
NTT_LOG_NS = (1, 2, 3, 6, 7, 8, 10, 12, 13, 14, 16)


def _cf():
    import closed_forms
    return closed_forms


def bitrev_index(log_n):
    return _cf().bitrev_bits(np.arange(1 << log_n), log_n)


class NttCase:
    """one logical vector a_0 .. a_(N-1); physical(flags) is the array a transform with these flags is given (a_i at slot i for DIF, at slot
    bitrev(i) for DIT, as the oracle's conventions have it).  support: frequencies at which a transform without the coset shift may be
    non-zero (None: no statement) -- forward, X_k = sum_i a_i w^(ik); the inverse transform's frequency k is the forward one's N - k.
    spikes: {forward frequency: value} where the closed form gives the values too."""

    def __init__(self, name, logical, support=None, spikes=None, physical=None, check=None):
        self.name, self.logical, self.support, self.spikes, self._physical, self.check = name, logical, support, spikes, physical, check

    def physical(self, flags, rev):
        if self._physical is not None:
            return self._physical[bool(flags & DIT)]
        return np.ascontiguousarray(self.logical[rev]) if flags & DIT else self.logical


def ntt_cases(log_n, seed=0):
    """the structured inputs of a transform of 2^log_n (canonical Montgomery rows, as the ABI requires)"""
    import cref
    cf = _cf()
    N = 1 << log_n
    rng = np.random.default_rng(1000 * seed + log_n)
    rnd = lambda: int.from_bytes(rng.bytes(40), "little") % P_
    import pyref
    w = pyref.Domain(N).gen
    zero = np.zeros((N, 4), np.uint64)
    out = [NttCase("zero", zero, support=[], spikes={})]
    for nm, c in (("const_1", 1), ("const_r_minus_1", P_ - 1), ("const_random", rnd())):
        out.append(NttCase(nm, cf.bcast(c, N), support=[0], spikes={0: N * c % P_}))
    ks = [(f"{k}", k) for k in sorted({0, 1 % N, N // 2, N - 1})] + [("random", int(rng.integers(0, N)))]
    for nm, k in ks:   # a_i = w^(k i): the forward transform is N at frequency -k, exact zeros elsewhere (cancellation at every stage)
        out.append(NttCase(f"root_power_k_{nm}", cf.powers_int(pow(w, k, P_), N).copy(), support=[(N - k) % N], spikes={(N - k) % N: N % P_}))
    for q in sorted({0, 1 % N, N // 2, N - 1}):
        a = zero.copy(); a[q] = cf.mont(rnd())
        out.append(NttCase(f"delta_at_{q}", a))
    v = rnd()
    a = np.empty((N, 4), np.uint64); a[0::2] = cf.mont(v); a[1::2] = cf.mont(P_ - v)
    out.append(NttCase("alternating_v_minus_v", a, support=[N // 2], spikes={N // 2: N * v % P_}))
    for s in range(log_n + 1):   # period 2^s: equal operands in every butterfly of log_n - s stages; non-zero only at multiples of N / 2^s
        per = cref.gen_scalars(1 << s, 50 + 100 * seed + s, 0)
        a = np.ascontiguousarray(np.tile(per, (N >> s, 1)))
        out.append(NttCase(f"periodic_2p{s}", a, support=list(range(0, N, N >> s))))
        if log_n:
            h = a.copy(); h[N // 2:] = 0
            out.append(NttCase(f"periodic_2p{s}_second_half_zero", h))
    # closed_forms: a_i = y^i + planted deltas, y a domain root (the geometric sum collapses) and y random; checked by ntt_check as well
    plants = cf.ntt_plants(log_n, seed)
    for nm, y in (("geometric_domain_root", pow(w, (N - max(1, N // 3)) % N, P_)), ("geometric_random", rnd())):
        phys = {False: cf.ntt_input(log_n, 0, y, plants), True: cf.ntt_input(log_n, DIT, y, plants)}
        out.append(NttCase(nm, phys[False], physical=phys, check=(y, plants)))
    for c in out:
        c.logical.setflags(write=False)
    return out


def ntt_closed_form_errors(case, got, log_n, flags, rev):
    """the closed-form statements of a case about one output (a second, oracle-free check); -> list of complaints"""
    cf = _cf()
    N = 1 << log_n
    bad = []
    if case.check is not None:
        y, plants = case.check
        slots = cf.ntt_check(got, log_n, flags, y, plants)
        if slots:
            bad.append(f"closed form (geometric) broken at slots {slots[:8]}")
    if case.support is None or flags & COSET:
        return bad
    inv, dit = bool(flags & INVERSE), bool(flags & DIT)
    # frequency k of this transform sits at slot k (DIT: natural out) or bitrev(k) (DIF)
    freq = lambda k: (N - k) % N if inv else k
    slot = lambda k: k if dit else int(rev[k])
    allowed = np.zeros(N, bool)
    for k in case.support:
        allowed[slot(freq(k))] = True
    nz = got.any(axis=1)
    if (nz & ~allowed).any():
        bad.append(f"non-zero rows outside the support: slots {np.nonzero(nz & ~allowed)[0][:8].tolist()}")
    for k, val in (case.spikes or {}).items():
        want = val * pow(N, -1, P_) % P_ if inv else val
        if not np.array_equal(got[slot(freq(k))], cf.mont(want)):
            bad.append(f"spike at frequency {k} is not {want:#x}")
    return bad


class HCase:
    def __init__(self, name, a, b, c, derive, zero_h=False, poly=None):
        self.name, self.a, self.b, self.c, self.derive, self.zero_h, self.poly = name, a, b, c, derive, zero_h, poly


def compute_h_cases(log_n, seed=0):
    """structured computeH inputs on the domain of 2^log_n; derive = True where c = a o b, so that c = None (formed on the device) is a case too"""
    import cref
    cf = _cf()
    N = 1 << log_n
    rng = np.random.default_rng(2000 * seed + log_n)
    rnd = lambda: int.from_bytes(rng.bytes(40), "little") % P_
    mul = lambda x, y: cref.field_op(0, 2, x, y)
    ra, rb, rc = (cref.gen_scalars(N, 70 + 10 * seed + k, 0) for k in range(3))
    zero = np.zeros((N, 4), np.uint64)
    out = [HCase("a_zero", zero, rb, zero, True, zero_h=True), HCase("b_zero", ra, zero, zero, True, zero_h=True),
           HCase("both_zero", zero, zero, zero, True, zero_h=True)]
    ca, cb = cf.bcast(rnd(), N), cf.bcast(P_ - 1, N)
    out.append(HCase("constants", ca, cb, mul(ca, cb), True, zero_h=N > 1))
    out.append(HCase("a_equals_b", ra, ra.copy(), mul(ra, ra), True))
    if log_n >= 1:   # deg a + deg b < N: a b - c is the zero polynomial, h is N exact zeros out of non-zero data
        rev = bitrev_index(log_n)
        da = N // 2 - 1; db = N - 1 - da
        def evals(deg, sd):
            co = zero.copy(); co[: deg + 1] = cref.gen_scalars(deg + 1, sd, 0)
            return np.ascontiguousarray(cref.ntt(co, log_n, 0)[rev])      # DIF: natural in, bit-reversed out
        pa, pb = evals(da, 90 + seed), evals(db, 91 + seed)
        out.append(HCase("low_degree_product", pa, pb, mul(pa, pb), True, zero_h=True))
    if log_n >= 2:
        ta, tb = cf.compute_h_poly(log_n, seed)
        pa, pb = cf.poly_eval(log_n, ta), cf.poly_eval(log_n, tb)
        out.append(HCase("sparse_polynomials", pa, pb, mul(pa, pb), True, poly=(ta, tb)))
    out.append(HCase("a_zero_c_unrelated", zero, rb, rc, False))
    for nc in sorted({1, min(2, N), max(N // 2, 1), min(N // 2 + 1, N), max(N - 1, 1), N}):
        out.append(HCase(f"zero_padded_nc{nc}", ra[:nc], rb[:nc], mul(ra[:nc], rb[:nc]), True))
        out.append(HCase(f"zero_padded_nc{nc}_c_unrelated", ra[:nc], rb[:nc], rc[:nc], False))
    for c in out:
        for v in (c.a, c.b, c.c):
            v.setflags(write=False)
    return out


if __name__ == "__main__":
    _child(sys.argv[1], int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5])

"""Closed-form references for the NTT, computeH and the MSMs at sizes where the oracle is too slow (2^27 and 2^28).

Every input is built so that its exact result has a closed form; host work is O(1) Python integers or chunked O(N) vector Fr arithmetic
through cref.field_op, CHUNK rows at a time, so host memory stays bounded whatever N is.

  NTT       a_i = y^i, plus planted deltas.  At frequency k the transform is s_k ((1 - (rho y)^N) / (1 - rho y z_k) + sum_j d_j (rho z_k)^p_j)
            with z_k = w^k (forward) or w^-k (inverse), rho = g for the forward coset transform (else 1), s_k = 1 forward, 1/N inverse,
            g^-k / N inverse coset.  DIF takes natural input and writes frequency k at slot bitrev(k); DIT takes a_i at slot bitrev(i)
            and writes natural output (oracle/pyref.py fft, fft_inverse).  Checked division-free: (V_k / s_k - D_k) (1 - rho y z_k) = C.
  computeH  a, b evaluations of sparse polynomials sum_t alpha_t X^m_t and sum_u beta_u X^p_u on the domain, c = a o b.  Then h is
            sum over m_t + p_u >= N of alpha_t beta_u X^(m_t + p_u - N), in bit-reversed order; every other coefficient is 0.
  MSM       points [x^i]G, scalars y^i (sum: geometric in xy) or a periodic mix v[i mod T] (sum: geometric per residue class), with
            planted rows (equal points, opposite points, infinity, scalars 0 / 1 / r - 1 / signed-digit edges) corrected one by one.
"""
import numpy as np
import pyref as P
import cref
from helpers import fr_arr, fr_vals, g1_arr, g2_arr

ADD, SUB, MUL = 0, 1, 2
R = P.R_MOD
CHUNK_BITS = 22
INVERSE, COSET, DIT = 1, 2, 4
G1 = g1_arr([P.G1_GEN])[0]
G2 = g2_arr([P.G2_GEN])[0]


def _op(op, x, y):
    return cref.field_op(0, op, x, y)


def mont(v):
    return fr_arr([v % R])[0]


def bcast(v, n):
    return np.ascontiguousarray(np.broadcast_to(mont(v).reshape(1, 4), (n, 4)))


_POW_CACHE = {}


def powers_int(g, n):
    """g^0 .. g^(n-1) as Montgomery rows (doubling blocks); the last few tables are kept (callers do not write into them)"""
    key = (g % R, n)
    if key in _POW_CACHE:
        return _POW_CACHE[key]
    if len(_POW_CACHE) > 8:
        _POW_CACHE.clear()
    _POW_CACHE[key] = out = _powers(g, n)
    return out


def _powers(g, n):
    out = np.empty((n, 4), np.uint64)
    out[0] = mont(1)
    k = 1
    while k < n:
        m = min(k, n - k)
        out[k:k + m] = _op(MUL, out[:m], bcast(pow(g, k, R), m))
        k *= 2
    return out


def bitrev_bits(v, bits):
    v = np.asarray(v, np.int64)
    r = np.zeros_like(v)
    for _ in range(bits):
        r = (r << 1) | (v & 1)
        v = v >> 1
    return r


def chunking(log_n, chunk_bits=CHUNK_BITS):
    """(cb, m, chunks, lo_rev): chunk h covers indices h*m .. h*m + m - 1; index h*m + lo is bitrev'd to lo_rev[lo] << (log_n - cb) | bitrev(h)"""
    cb = min(log_n, chunk_bits)
    return cb, 1 << cb, 1 << (log_n - cb), bitrev_bits(np.arange(1 << cb), cb)


def canonical(rows):
    """True where a Montgomery row is < r (the library keeps every element reduced)"""
    rl = [(R >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
    rows = np.asarray(rows, np.uint64)
    lt = np.zeros(rows.shape[0], bool)
    eq = np.ones(rows.shape[0], bool)
    for i in (3, 2, 1, 0):
        lt |= eq & (rows[:, i] < np.uint64(rl[i]))
        eq &= rows[:, i] == np.uint64(rl[i])
    return lt


# ---------------------------------------------------------------------------------------------------- NTT
def ntt_plants(log_n, seed=0):
    """planted deltas (logical position, value): the first and last positions, 2^10-element tile and 2^20 pass boundaries, the middle"""
    N = 1 << log_n
    pos = sorted({0, N - 1, N >> 1} | {p for p in (1 << 10, 3 << 10, 1 << 20, (1 << 20) + (1 << 10)) if p < N})
    rng = np.random.default_rng(seed)
    return [(p, int.from_bytes(rng.bytes(32), "little") % R) for p in pos]


def ntt_input_chunks(log_n, flags, y, plants, chunk_bits=CHUNK_BITS):
    """yields (slot offset, rows) of the input: a_i = y^i + planted deltas, a_i at slot i (DIF) or slot bitrev(i) (DIT)"""
    cb, m, chunks, lo_rev = chunking(log_n, chunk_bits)
    dit = bool(flags & DIT)
    hi_bits = log_n - cb
    # DIF: slot h*m + lo holds a_(h*m + lo) = y^(h m) * (y^lo);  DIT: it holds a_i, i = lo_rev << hi_bits | bitrev(h)
    tab = powers_int(pow(y, 1 << hi_bits, R), m)[lo_rev] if dit else powers_int(y, m)
    pl = dict(plants)
    for h in range(chunks):
        base = int(bitrev_bits(h, hi_bits)) if dit else h * m
        rows = _op(MUL, tab, bcast(pow(y, base, R), m))
        slots = np.arange(h * m, (h + 1) * m)
        idx = ((lo_rev << hi_bits) | base) if dit else slots
        for p, d in pl.items():
            hit = np.nonzero(idx == p)[0]
            if len(hit):
                rows[hit[0]] = mont(pow(y, p, R) + d)
        yield h * m, rows


def ntt_input(log_n, flags, y, plants, chunk_bits=CHUNK_BITS):
    out = np.empty((1 << log_n, 4), np.uint64)
    for off, rows in ntt_input_chunks(log_n, flags, y, plants, chunk_bits):
        out[off:off + rows.shape[0]] = rows
    return out


def ntt_check(out, log_n, flags, y, plants, chunk_bits=CHUNK_BITS):
    """-> indices of the output slots that break the closed form (empty: every output is right).  Division-free, chunk by chunk."""
    N = 1 << log_n
    dom = P.Domain(N)
    cb, m, chunks, lo_rev = chunking(log_n, chunk_bits)
    inv, coset, dit = bool(flags & INVERSE), bool(flags & COSET), bool(flags & DIT)
    om = dom.gen_inv if inv else dom.gen
    rho = P.FR_COSET_GEN if coset and not inv else 1
    # V_k / s_k: s_k = 1/N, or g^-k / N.  sinv_k = N (g^k): a table over lo and a constant per chunk
    sinv_tab = powers_int(P.FR_COSET_GEN, m) if inv and coset else None
    C = (1 - pow(rho * y, N, R)) % R
    # plant terms d_j rho^p_j (om^p_j)^k: chunk-invariant when (om^p_j)^m = 1, else a table times a constant per chunk
    fixed = np.zeros((m, 4), np.uint64)
    moving = []
    for p, d in plants:
        c0 = d * pow(rho, p, R) % R
        zp = pow(om, p, R)
        tab = _op(MUL, powers_int(zp, m), bcast(c0, m))
        if pow(zp, m, R) == 1:
            fixed = _op(ADD, fixed, tab)
        else:
            moving.append((zp, tab))
    u_tab = powers_int(om, m)
    one = bcast(1, m)
    bad = []
    for h in range(chunks):
        k0 = h * m
        slots = ((lo_rev << (log_n - cb)) | int(bitrev_bits(h, log_n - cb))) if not dit else np.arange(k0, k0 + m)
        V = np.ascontiguousarray(out[slots])
        ok = canonical(V)
        if inv:
            sinv = _op(MUL, sinv_tab, bcast(N * pow(P.FR_COSET_GEN, k0, R), m)) if coset else bcast(N, m)
            V = _op(MUL, V, sinv)
        D = fixed
        for zp, tab in moving:
            D = _op(ADD, D, _op(MUL, tab, bcast(pow(zp, k0, R), m)))
        one_minus_u = _op(SUB, one, _op(MUL, u_tab, bcast(rho * y * pow(om, k0, R), m)))
        lhs = _op(MUL, _op(SUB, V, D), one_minus_u)
        ok &= (lhs == mont(C)).all(axis=1)
        if not ok.all():
            bad.extend(slots[~ok][:8].tolist())
    return bad


# ---------------------------------------------------------------------------------------------------- computeH
def compute_h_poly(log_n, seed=0):
    """a = alpha_1 X^(N-1) + alpha_2 X^(N-64) + alpha_3 X^3, b = beta_1 X^(N-2) + beta_2 X^(N/2) + beta_3: degrees near N (products wrap)
    and one term each that stays below N; small sizes keep the same pattern"""
    N = 1 << log_n
    rng = np.random.default_rng(seed)
    rnd = lambda: int.from_bytes(rng.bytes(32), "little") % R
    ma = [N - 1, max(N - 64, 1), 3 % N]
    mb = [N - 2, N >> 1, 0]
    return [(d, rnd()) for d in ma], [(d, rnd()) for d in mb]


def poly_eval_chunks(log_n, terms, chunk_bits=CHUNK_BITS):
    """yields (offset, rows): sum_t coef_t (w^i)^deg_t for the domain points w^i, natural order"""
    cb, m, chunks, _ = chunking(log_n, chunk_bits)
    w = P.Domain(1 << log_n).gen
    tabs = [(pow(w, d, R), _op(MUL, powers_int(pow(w, d, R), m), bcast(cf, m))) for d, cf in terms]
    for h in range(chunks):
        acc = None
        for wd, tab in tabs:
            z = pow(wd, h * m, R)
            t = tab if z == 1 else _op(MUL, tab, bcast(z, m))
            acc = t if acc is None else _op(ADD, acc, t)
        yield h * m, acc


def poly_eval(log_n, terms, chunk_bits=CHUNK_BITS):
    out = np.empty((1 << log_n, 4), np.uint64)
    for off, rows in poly_eval_chunks(log_n, terms, chunk_bits):
        out[off:off + rows.shape[0]] = rows
    return out


def compute_h_expected(log_n, ta, tb):
    """{slot: Montgomery row} of the non-zero coefficients of h, at their bit-reversed slots"""
    N = 1 << log_n
    coef = {}
    for da, ca in ta:
        for db, cb_ in tb:
            if da + db >= N:
                e = da + db - N
                coef[e] = (coef.get(e, 0) + ca * cb_) % R
    return {int(bitrev_bits(e, log_n)): mont(v) for e, v in coef.items() if v}


def compute_h_check(h, log_n, ta, tb):
    """-> slots of h that differ from the closed form (whole vector, numpy only)"""
    want = compute_h_expected(log_n, ta, tb)
    nz = np.nonzero(h.any(axis=1))[0]
    bad = sorted(set(int(i) for i in nz[:64]) - set(want))
    bad += [s for s, v in want.items() if not np.array_equal(h[s], v)]
    if len(nz) != len(want):
        bad.append(-1)
    return bad


# ---------------------------------------------------------------------------------------------------- MSM
def edge_values():
    import dlog_keys
    return dlog_keys.edge_values()


def mix_values(T, bit_pm, byte_pm, u64_pm, seed=0):
    """one period of the periodic scalar mix: the census shares of {0, 1}, bytes and 64-bit values, the rest full-width"""
    rng = np.random.default_rng(seed)
    nb, ny, nu = (T * s // 1000 for s in (bit_pm, byte_pm, u64_pm))
    vals = [int(v) for v in rng.integers(0, 2, nb)] + [int(v) for v in rng.integers(0, 256, ny)]
    vals += [int(rng.integers(0, 1 << 63)) * 2 + 1 for _ in range(nu)]
    vals += [int.from_bytes(rng.bytes(32), "little") % R for _ in range(T - len(vals))]
    rng.shuffle(vals)
    return vals


def msm_plants(n, boundaries=(), seed=0):
    """planted rows {row: (kind, arg)} at the first and last rows and both sides of the given slice boundaries.
    kinds: 'eq' (point and scalar of row arg), 'neg' (minus the point of row arg, its scalar), 'inf' (point at infinity),
    'sc' (scalar arg), 'eqp' (point of row arg, own scalar)"""
    rows = sorted({r for b in (0, n - 1) + tuple(boundaries) for r in (b - 2, b - 1, b, b + 1, b + 2) if 0 <= r < n})
    ev = edge_values()
    kinds = []
    extra = [("sc", 0), ("sc", 1), ("sc", R - 1)] + [("sc", v) for v in ev]
    out = {}
    rng = np.random.default_rng(seed)
    for i, r in enumerate(rows):
        j = i % 6
        if j == 0 and r > 0:
            out[r] = ("eq", r - 1)
        elif j == 1 and r > 0:
            out[r] = ("neg", r - 1)
        elif j == 2:
            out[r] = ("inf", None)
        elif j == 3 and r > 0:
            out[r] = ("eqp", int(rng.integers(0, r)))
        else:
            out[r] = extra[i % len(extra)]
        kinds.append(out[r][0])
    # the rest of the edge values on rows spread over the middle
    free = [r for r in range(1, n - 1, max(1, (n - 2) // (len(extra) + 1)))][:len(extra)]
    for k, r in enumerate(free):
        if r not in out and all(v[1] != r for v in out.values()):
            out[r] = extra[k]
    return out


class MsmCase:
    """points [x^i]G and scalars (y^i, or mix[i mod T]) with plants; sum() is the discrete log of the MSM"""

    def __init__(self, n, x, y=None, mix=None, plants=None):
        self.n, self.x, self.y, self.mix = n, x, y, mix
        self.plants = plants or {}
        self.final = {}
        for r in sorted(self.plants):
            kind, arg = self.plants[r]
            e, s = self._e(r), self._s(r)
            if kind in ("eq", "neg", "eqp"):
                es, ss = self.final.get(arg, (self._e(arg), self._s(arg)))
                e = es if kind != "neg" else (R - es) % R
                s = ss if kind != "eqp" else s
            elif kind == "inf":
                e = 0
            else:
                s = arg % R
            self.final[r] = (e, s)

    def _e(self, i):
        return pow(self.x, i, R)

    def _s(self, i):
        return pow(self.y, i, R) if self.mix is None else self.mix[i % len(self.mix)] % R

    def sum(self):
        n, x = self.n, self.x
        if self.mix is None:
            q = x * self.y % R
            S = n % R if q == 1 else (1 - pow(q, n, R)) * P.fr_inv((1 - q) % R) % R
        else:
            T = len(self.mix)
            xt = pow(x, T, R)
            S = 0
            for r_, v in enumerate(self.mix):
                cnt = (n - r_ + T - 1) // T if r_ < n else 0
                geo = cnt % R if xt == 1 else (1 - pow(xt, cnt, R)) * P.fr_inv((1 - xt) % R) % R
                S += v * pow(x, r_, R) * geo
        for r, (e, s) in self.final.items():
            S += e * s - self._e(r) * self._s(r)
        return S % R

    def _rows(self, lo, hi, which):
        """Montgomery rows lo..hi-1 of the exponents ('e') or the scalars ('s'), plants applied"""
        m = hi - lo
        if which == "e" or self.mix is None:
            g = self.x if which == "e" else self.y
            rows = _op(MUL, powers_int(g, m), bcast(pow(g, lo, R), m)) if m else np.zeros((0, 4), np.uint64)
        else:
            T = len(self.mix)
            per = fr_arr(self.mix)
            rows = per[(np.arange(lo, hi) % T)]
        for r, (e, s) in self.final.items():
            if lo <= r < hi:
                rows[r - lo] = mont(e if which == "e" else s)
        return rows

    def chunks(self, which, chunk=1 << CHUNK_BITS):
        for lo in range(0, self.n, chunk):
            yield lo, self._rows(lo, min(self.n, lo + chunk), which)

    def spot_rows(self, k=64, seed=0):
        rng = np.random.default_rng(seed)
        pick = {0, self.n - 1} | set(list(self.final)[:k // 2])
        while len(pick) < min(k, self.n):
            pick.add(int(rng.integers(0, self.n)))
        return sorted(pick)


def fr_row_int(row):
    return fr_vals(np.asarray(row).reshape(1, 4))[0]

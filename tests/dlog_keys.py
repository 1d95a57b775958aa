"""Proving keys whose every point is a known multiple of the generator, and the proof they imply computed in the exponent.

With every key point g^e for a known e, the three proof points have discrete logs that follow from O(N) Fr arithmetic alone -- no MSM,
no NTT, no curve arithmetic at scale -- so a whole proof is checked against the Groth16 formulas themselves rather than against a second
implementation of the same conventions:

    ar  = alpha + sum_{j not infA} W_j A_j + r delta
    bs  = beta  + sum_{j not infB} W_j B_j + s delta                  (Bs in G2, Bs1 in G1: the same B exponents)
    krs = sum_{j in K} W_j K_j + (A(tau) B(tau) - C(tau)) / delta + s ar + r bs - r s delta
    A(tau) = sum_i a_i L_i(tau),  L_i(tau) = (tau^N - 1) / N * w^i / (tau - w^i)

The Z term holds because pk.G1.Z[i] has exponent tau^i (tau^N - 1) / delta (stored bit-reversed, as gnark keeps it) and h = (AB - C) /
(X^N - 1) when c = a o b on the domain.  All vector arithmetic runs through cref.field_op (Montgomery Fr, OpenMP); only the final scalars
become Python integers.

The keys are shaped like a real gnark key rather than like tests/helpers.py:synthetic_pk, through planted wires (make_exps):
  copies     equal A, B, K exponents and W value (runs of identical wires: buckets that start with P + P; some with W = 1)
  negations  A, B, K negated, the same W (alternating runs P, -P, P, ...: buckets that cancel to the point at infinity)
  unused     a private wire in no constraint: A and B at infinity, K = 0 (the point at infinity inside pk.G1.K), W non-zero
  committed  copies where one wire is committed (left out of K) and the other is not
  edges      W values at the signed-digit edges of the window widths c = 16..22, plus 0, 1 and r - 1
"""
import numpy as np
import pyref as P
import cref
from helpers import fr_arr, fr_vals, g1_arr, g2_arr, g1_pts, g2_pts

ADD, SUB, MUL, INV = 0, 1, 2, 3
ONE = fr_arr([1])[0]
ZERO = np.zeros(4, np.uint64)
EDGE_WIDTHS = (16, 17, 18, 19, 20, 22)
CHUNK_BITS = 22
G1 = g1_arr([P.G1_GEN])[0]
G2 = g2_arr([P.G2_GEN])[0]


# ---------------------------------------------------------------------------------------------------- vector Fr arithmetic (Montgomery rows)
def _op(op, x, y=None):
    return cref.field_op(0, op, x, y)


def _bc(v, n):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.uint64).reshape(1, 4), (n, 4)))


def neg(x):
    return _op(SUB, np.zeros_like(x), x)


def fr_sum(x):
    """sum of the rows (pairwise tree)"""
    x = np.ascontiguousarray(x, np.uint64)
    if x.shape[0] == 0:
        return ZERO.copy()
    while x.shape[0] > 1:
        if x.shape[0] & 1:
            x = np.concatenate([x, ZERO.reshape(1, 4)])
        x = _op(ADD, x[0::2], x[1::2])
    return x[0]


def fr_dot(x, y):
    return fr_sum(_op(MUL, x, y)) if len(x) else ZERO.copy()


def powers(g, n):
    """g^0 .. g^(n-1) by doubling blocks"""
    out = np.empty((n, 4), np.uint64)
    out[0] = ONE
    k, gk = 1, np.asarray(g, np.uint64).reshape(1, 4)
    while k < n:
        m = min(k, n - k)
        out[k:k + m] = _op(MUL, out[:m], _bc(gk, m))
        gk = _op(MUL, gk, gk)
        k *= 2
    return out


def batch_inv(x):
    """1/x for every row (none zero) by a product tree: log2(n) vector multiplications up, one inversion, log2(n) down"""
    levels = [np.ascontiguousarray(x, np.uint64)]
    while levels[-1].shape[0] > 1:
        cur = levels[-1]
        if cur.shape[0] & 1:
            cur = levels[-1] = np.concatenate([cur, ONE.reshape(1, 4)])
        levels.append(_op(MUL, cur[0::2], cur[1::2]))
    inv = _op(INV, levels[-1])
    for lvl in reversed(levels[:-1]):
        inv = inv[:lvl.shape[0] // 2]          # the parent level may carry a padding row of its own
        out = np.empty_like(lvl)
        out[0::2] = _op(MUL, inv, lvl[1::2])
        out[1::2] = _op(MUL, inv, lvl[0::2])
        inv = out
    return inv[:x.shape[0]]


def bitrev_index(log_n):
    i = np.arange(1 << log_n, dtype=np.uint64)
    r = np.zeros_like(i)
    for _ in range(log_n):
        r = (r << np.uint64(1)) | (i & np.uint64(1))
        i >>= np.uint64(1)
    return r.astype(np.int64)


def _int(row):
    return fr_vals(np.asarray(row).reshape(1, 4))[0]


# ---------------------------------------------------------------------------------------------------- the key's exponents
def edge_values():
    """W values at the edges of the signed c-bit digits the MSMs recode into (csrc/msm_core.cuh msm_digits_body: a digit reaching
    2^(c-1) becomes -2^(c-1) with a carry), for the window widths of the production plans, plus 0, 1, r - 1"""
    vals = {0, 1, P.R_MOD - 1, P.R_MOD - 2, (P.R_MOD - 1) // 2, 1 << 253}
    for c in EDGE_WIDTHS:
        h = 1 << (c - 1)
        m = 253 // c                                       # whole windows below r
        for k in range(1, m + 1):
            vals.add((1 << (c * k)) - 1)                   # all-ones chunks: digits -1 with carries, the last carry alone in window k
            vals.add(1 << (c * k - 1))                     # a lone top digit -2^(c-1)
        vals.add(h + sum((h - 1) << (c * k) for k in range(1, m)))   # every digit -2^(c-1)
        vals.add(sum((h - 1) << (c * k) for k in range(m)))          # every digit +2^(c-1) - 1 (the largest that needs no carry)
        vals.add(sum(h << (c * k) for k in range(m)))                # every chunk 2^(c-1): -2^(c-1) first, then 2^(c-1) + 1 - 2^c ...
    return sorted(v % P.R_MOD for v in vals)


def _plant_count(nb_wires, nb_public):
    priv = nb_wires - nb_public
    return max(4, min(max(300, nb_wires >> 8), priv // 16))


def make_exps(log_n, nb_wires, nb_public, n_committed, mask_permille=(900, 500), plants=True, seed=1):
    """Random Fr exponents for alpha, beta, delta, tau and every wire's A / B / K, the infinity masks (mask_permille = per-mille of the
    wires NOT at infinity in A, in B), the committed set and the planted structure.  Rows are Montgomery (n, 4) uint64."""
    rng = np.random.default_rng(seed)
    alpha, beta, delta, tau = cref.gen_scalars(4, seed, 0)
    A, B, K = (cref.gen_scalars(nb_wires, seed + k, 0) for k in (1, 2, 3))
    inf_a = (rng.integers(0, 1000, nb_wires) >= mask_permille[0]).astype(np.uint8)
    inf_b = (rng.integers(0, 1000, nb_wires) >= mask_permille[1]).astype(np.uint8)
    pl = {"dst": np.zeros(0, np.int64), "src": np.zeros(0, np.int64), "neg": np.zeros(0, bool), "runs": [], "w_one": np.zeros(0, np.int64),
          "unused": np.zeros(0, np.int64), "edge": np.zeros(0, np.int64), "edge_vals": [], "committed_pairs": 0}
    committed = np.zeros(0, np.int64)
    if plants:
        cnt = _plant_count(nb_wires, nb_public)
        run = min(128, max(2, cnt // 2))
        start = nb_public + int(rng.integers(0, nb_wires - nb_public - 9 * cnt))
        nxt = [start]

        def take(n):
            z = np.arange(nxt[0], nxt[0] + n); nxt[0] += n; return z
        copy_runs, neg_runs = take(2 * cnt), take(2 * cnt)
        scat_copy, scat_neg, unused = take(cnt), take(cnt), take(cnt)
        com_twins, edge = take(cnt), take(cnt)
        zone = np.arange(start, nxt[0])
        free = np.setdiff1d(np.arange(nb_public, nb_wires), zone)        # private wires outside the planted zone
        n_com_pairs = min(cnt, n_committed // 2)
        half = n_com_pairs // 2
        com_src = rng.choice(free, half, replace=False)                  # (d) committed sources of non-committed copies
        rest = np.setdiff1d(free, com_src)
        extra = rng.choice(rest, n_committed - n_com_pairs, replace=False)   # the rest of the committed set
        non_com = np.setdiff1d(rest, extra)
        nc_src = rng.choice(non_com, n_com_pairs - half, replace=False)  # (d) non-committed sources of committed copies
        committed = np.sort(np.concatenate([com_src, com_twins[half:n_com_pairs], extra])).astype(np.int64)
        # forced masks: runs and edges sit in A, B and K, unused wires in K alone
        for z in (copy_runs, neg_runs, edge):
            inf_a[z] = 0; inf_b[z] = 0
        inf_a[unused] = 1; inf_b[unused] = 1
        K[unused] = 0
        dst, src, sgn = [], [], []
        for zr, negate in ((copy_runs, False), (neg_runs, True)):
            for s0 in range(0, len(zr), run):
                r_ = zr[s0:s0 + run]
                pl["runs"].append((int(r_[0]), len(r_), negate))
                dst.append(r_[1:]); src.append(np.full(len(r_) - 1, r_[0]))
                sgn.append((np.arange(1, len(r_)) & 1).astype(bool) if negate else np.zeros(len(r_) - 1, bool))
        dst += [scat_copy, scat_neg]; src += [rng.choice(non_com, cnt), rng.choice(non_com, cnt)]
        sgn += [np.zeros(cnt, bool), np.ones(cnt, bool)]
        # (d): committed source -> non-committed copy; non-committed source -> committed copy
        dst.append(com_twins[:n_com_pairs]); src.append(np.concatenate([com_src, nc_src]))
        sgn.append(np.zeros(n_com_pairs, bool))
        pl["dst"], pl["src"], pl["neg"] = np.concatenate(dst), np.concatenate(src).astype(np.int64), np.concatenate(sgn)
        d, s_, ng = pl["dst"], pl["src"], pl["neg"]
        for X in (A, B, K):
            X[d] = X[s_]
            if ng.any():
                X[d[ng]] = neg(X[d[ng]])
        inf_a[d] = inf_a[s_]; inf_b[d] = inf_b[s_]
        pl["w_one"] = np.array([r0 for i, (r0, _, _) in enumerate(pl["runs"]) if i % 2 == 0], np.int64)
        pl["unused"], pl["edge"] = unused, edge
        ev = edge_values()
        pl["edge_vals"] = [ev[i % len(ev)] for i in range(len(edge))]
        pl["committed_pairs"] = n_com_pairs
    elif n_committed:
        committed = np.sort(rng.choice(np.arange(nb_public, nb_wires), n_committed, replace=False)).astype(np.int64)
    assert len(committed) == n_committed and len(np.unique(committed)) == n_committed
    return {"log_n": log_n, "nb_wires": nb_wires, "nb_public": nb_public, "alpha": alpha, "beta": beta, "delta": delta, "tau": tau,
            "A": A, "B": B, "K": K, "infinity_a": inf_a, "infinity_b": inf_b, "committed": committed, "plants": pl, "seed": seed}


def k_rows(exps):
    """wire indices of pk.G1.K: private and not committed"""
    keep = np.ones(exps["nb_wires"], bool)
    keep[:exps["nb_public"]] = False
    keep[exps["committed"]] = False
    return np.nonzero(keep)[0]


def z_exps(exps):
    """pk.G1.Z exponents in natural order: tau^i (tau^N - 1) / delta"""
    N = 1 << exps["log_n"]
    tau = _int(exps["tau"])
    zt = (pow(tau, N, P.R_MOD) - 1) * P.fr_inv(_int(exps["delta"])) % P.R_MOD
    return _op(MUL, powers(exps["tau"], N), _bc(fr_arr([zt])[0], N))


def witness(exps, dist, seed):
    """W from the oracle's generator with the plants applied: W[0] = 1, copies share W, some runs W = 1, unused wires non-zero, edges"""
    nw = exps["nb_wires"]
    W = cref.gen_scalars(nw, seed, dist)
    pl = exps["plants"]
    W[0] = ONE
    if len(pl["unused"]):
        W[pl["unused"]] = cref.gen_scalars(len(pl["unused"]), seed + 1, 0)
        W[pl["w_one"]] = ONE
        W[pl["edge"]] = fr_arr(pl["edge_vals"])
        W[pl["dst"]] = W[pl["src"]]
    return W


def constraint_values(n_constraints, dist, seed):
    a = cref.gen_scalars(n_constraints, seed, dist)
    b = cref.gen_scalars(n_constraints, seed + 1, 0)
    return a, b, _op(MUL, a, b)


# ---------------------------------------------------------------------------------------------------- the proof in the exponent
def z_exps_bitrev(exps, chunk_bits=CHUNK_BITS):
    """z_exps in the bit-reversed order pk.G1.Z is stored in, built chunk by chunk (no N-row index array, no second N-row copy): slot
    h m + lo holds the exponent of i = bitrev_cb(lo) 2^(log_n - cb) + bitrev(h), i.e. (tau^(2^(log_n - cb)))^bitrev_cb(lo) tau^bitrev(h)"""
    L = exps["log_n"]
    cb = min(L, chunk_bits)
    m, hi = 1 << cb, L - cb
    tau = _int(exps["tau"])
    zt = (pow(tau, 1 << L, P.R_MOD) - 1) * P.fr_inv(_int(exps["delta"])) % P.R_MOD
    tab = powers(fr_arr([pow(tau, 1 << hi, P.R_MOD)])[0], m)[bitrev_index(cb)]
    out = np.empty((1 << L, 4), np.uint64)
    for h in range(1 << hi):
        out[h * m:(h + 1) * m] = _op(MUL, tab, _bc(fr_arr([zt * pow(tau, P.bitrev(h, hi), P.R_MOD)])[0], m))
    return out


def _masked_dot(W, X, keep, chunk):
    acc = ZERO.copy()
    for lo in range(0, len(keep), chunk):
        k = keep[lo:lo + chunk]
        acc = _op(ADD, acc.reshape(1, 4), fr_dot(W[lo:lo + chunk][k], X[lo:lo + chunk][k]).reshape(1, 4))[0]
    return acc


def expected_proof_exps(exps, W, a, b, r, s, chunk=1 << CHUNK_BITS):
    """-> (ar, bs, krs) as canonical integers, by the formulas of the module docstring (c = a o b).  Vector work runs `chunk` rows at a
    time, so host memory beyond the inputs stays O(chunk) whatever N is."""
    N = 1 << exps["log_n"]
    nw = exps["nb_wires"]
    ia, ib = exps["infinity_a"][:nw] == 0, exps["infinity_b"][:nw] == 0
    keep_k = np.zeros(nw, bool)
    keep_k[k_rows(exps)] = True
    sa = _masked_dot(W, exps["A"], ia, chunk)
    sb = _masked_dot(W, exps["B"], ib, chunk)
    sk = _masked_dot(W, exps["K"], keep_k, chunk)
    dom = P.Domain(N)
    nc = a.shape[0]
    at = bt = ct = 0
    wtab = powers(fr_arr([dom.gen])[0], min(chunk, nc)) if nc else None
    for lo in range(0, nc, chunk):
        m = min(chunk, nc - lo)
        wp = _op(MUL, wtab[:m], _bc(fr_arr([pow(dom.gen, lo, P.R_MOD)])[0], m))
        lw = _op(MUL, wp, batch_inv(_op(SUB, _bc(exps["tau"], m), wp)))          # w^i / (tau - w^i)
        ac, bc_ = a[lo:lo + m], b[lo:lo + m]
        at += _int(fr_dot(ac, lw)); bt += _int(fr_dot(bc_, lw)); ct += _int(fr_dot(_op(MUL, ac, bc_), lw))
    tau, alpha, beta, delta = (_int(exps[k]) for k in ("tau", "alpha", "beta", "delta"))
    R = P.R_MOD
    lam = (pow(tau, N, R) - 1) * dom.card_inv % R                            # L_i(tau) = lam * w^i / (tau - w^i)
    hz = (lam * lam * at * bt - lam * ct) * P.fr_inv(delta) % R
    rc, sc = _int(r), _int(s)
    ar = (alpha + _int(sa) + rc * delta) % R
    bs = (beta + _int(sb) + sc * delta) % R
    krs = (_int(sk) + hz + sc * ar + rc * bs - rc * sc * delta) % R
    return ar, bs, krs


def check_proof(proof, want):
    """Ar, Bs, Krs of a proof (mi_proof_out / cref layout) against g^ar, g2^bs, g^krs (pyref's double-and-add)"""
    ar, bs, krs = want
    assert g1_pts(proof["ar"])[0] == P.g1_mul(P.G1_GEN, ar), "Ar is not g^ar"
    assert g2_pts(proof["bs"])[0] == P.g2_mul(P.G2_GEN, bs), "Bs is not g2^bs"
    assert g1_pts(proof["krs"])[0] == P.g1_mul(P.G1_GEN, krs), "Krs is not g^krs"


# ---------------------------------------------------------------------------------------------------- the key's points
def _key_scalars(exps):
    ia, ib = exps["infinity_a"] == 0, exps["infinity_b"] == 0
    N = 1 << exps["log_n"]
    z = z_exps_bitrev(exps)
    return {"g1_a": exps["A"][ia], "g1_b": exps["B"][ib], "g1_k": exps["K"][k_rows(exps)], "g1_z": z, "g2_b": exps["B"][ib]}, N


def _small_points(exps):
    d = {k + "1": cref.batch_scalar_mul(G1, exps[k].reshape(1, 4))[0] for k in ("alpha", "beta", "delta")}
    d.update({k + "2": cref.batch_scalar_mul(G2, exps[k].reshape(1, 4), g2=True)[0] for k in ("beta", "delta")})
    return d


def _pk_dict(exps, arrays):
    pk = {"log_n": exps["log_n"], "nb_public": exps["nb_public"], "nb_wires": exps["nb_wires"],
          "infinity_a": exps["infinity_a"], "infinity_b": exps["infinity_b"],
          "committed_wires": exps["committed"].astype(np.uint32) if len(exps["committed"]) else None}
    pk.update(_small_points(exps))
    pk.update(arrays)
    return pk


def spot_rows(n, exps_rows, seed=0):
    """64 rows to spot-check: the first, the last, and rows of the given exponents that are zero (points at infinity), the rest random"""
    rng = np.random.default_rng(seed)
    zero = np.nonzero(~exps_rows.any(axis=1))[0][:8]
    pick = np.concatenate([np.arange(min(n, 8)), np.arange(max(0, n - 8), n), zero, rng.integers(0, max(n, 1), 64)])
    return np.unique(pick)[:64] if n else pick[:0]


def _spot_check(name, rows, got, scal):
    want = [P.g2_mul(P.G2_GEN, e) if name == "g2_b" else P.g1_mul(P.G1_GEN, e) for e in fr_vals(scal[rows])]
    have = g2_pts(got) if name == "g2_b" else g1_pts(got)
    assert have == want, f"key array {name}: a row is not g^e"


def points_from_exps(exps, ctx=None, device=False):
    """The proving key of these exponents.  ctx None: host arrays by cref.batch_scalar_mul.  ctx given: host arrays by the device's
    mi_batch_scalar_mul_g1/g2; device = True: device-resident arrays (pk_load(device_points=True) form, (ptr, count)), returned with the
    DevArrays to free.  Device-built arrays are spot-checked: 64 rows of each against pyref's scalar multiplication."""
    scal, _ = _key_scalars(exps)
    arrays, bufs = {}, []
    for name, sc in scal.items():
        g2 = name == "g2_b"
        base = G2 if g2 else G1
        if ctx is None:
            arrays[name] = cref.batch_scalar_mul(base, sc, g2=g2)
            continue
        rows = spot_rows(sc.shape[0], sc, exps["seed"])
        width = 16 if g2 else 8
        if device:
            ds = ctx.to_dev(sc)
            out = ctx.alloc(max(8 * width * sc.shape[0], 32))
            ctx.batch_scalar_mul_dev(base, ds.ptr, sc.shape[0], out.ptr, g2=g2)
            ds.free()
            got = np.stack([_download_row(ctx, out.ptr, int(i), width) for i in rows]) if len(rows) else np.zeros((0, width), np.uint64)
            arrays[name] = (out.ptr, sc.shape[0]); bufs.append(out)
        else:
            arrays[name] = ctx.batch_scalar_mul(base, sc, g2=g2)
            got = arrays[name][rows]
        _spot_check(name, rows, got, sc)
    pk = _pk_dict(exps, arrays)
    return (pk, bufs) if device else pk


def _download_row(ctx, ptr, i, width):
    import ctypes as C
    out = np.zeros(width, np.uint64)
    ctx._ck(ctx.lib.mi_dev_download(ctx.h, out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr + 8 * width * i), C.c_size_t(out.nbytes)))
    return out

"""GPU: what the device entry points write and read, one row per entry point.  Every device argument is a tests/banded.py Banded:
exactly as many bytes as the call is told about, on a 32-byte boundary that is no 64-byte boundary (the header's contract and no
better; the byte strings documented as "any alignment" at an odd address), with 256 KiB of a seeded non-field pattern on either
side inside the same allocation.  Outputs start as pattern.  After the call the result equals the reference bit for bit, every
guard is unchanged and every const argument is unchanged; an in-place argument is checked on its guards.  References: the C oracle
(cref), pyref, Python integers, and for the verifier's bulk kernels the host build of the same text (tests/emu).

What this cannot see: a read past the end that never influences a result.  tests/test_banded_cpu.py proves that a read which IS
used cannot reproduce the oracle's zero padding, and that the sizes below are ragged where they are meant to be.

Before the first run the kernels behind these rows were read for how they load their caller pointers: the widest access is a 16-byte
vector (uint4) at a multiple of 32 bytes from the pointer, and the codecs read bytes; nothing asks for more than the 32 bytes of
include/mi355x_groth16.h."""
import ctypes as C
import time
import numpy as np
import pytest
import pyref as P
import cref
import banded as BD
import fixed_base_cases as FB
import generic_msm_cases as G
import keyfile_cases as K
import verify_cases as V
import verify_combined_cases as VC
import verify_locate_cases as LC
from banded import Banded
from helpers import fr_arr, g1_arr, g2_arr, g1_pts, g2_pts
from gpu_common import load_binding
from test_gpu_setup import _toy_setup_exps_only, _toy_key_from_exps

pytestmark = pytest.mark.gpu
RPRIME = 2   # MI_MSM_TABLE_RPRIME
M128 = (1 << 128) - 1


@pytest.fixture(scope="module")
def ctx():
    t0 = time.perf_counter()
    c = load_binding().Context(0)
    yield c
    c.close()
    print(f"\ntests/test_gpu_buffer_bounds.py: {time.perf_counter() - t0:.1f} s wall from its first test to its last")


class Bands:
    """the buffers of one test: freed together, and only after every check has run"""
    def __init__(self, ctx):
        self.ctx, self.all, self.const = ctx, [], []

    def inp(self, arr, name, odd=False):
        arr = np.ascontiguousarray(arr)
        b = Banded.of(self.ctx, arr, odd=odd, name=name)
        self.all.append(b); self.const.append((b, arr))
        return b

    def out(self, nbytes, name, odd=False):
        b = Banded(self.ctx, nbytes, odd=odd, name=name)
        self.all.append(b)
        return b

    def inout(self, arr, name):
        b = Banded.of(self.ctx, arr, name=name)
        self.all.append(b)
        return b

    def settle(self, what=""):
        """after a call: every guard and every const argument"""
        self.ctx.sync()
        msgs = [m for b in self.all for m in b.report()]
        assert not msgs, f"{what}: " + "; ".join(msgs)
        for b, arr in self.const:
            b.assert_unchanged(arr)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self.all:
            b.free()


def _jac_eq(got, want):
    """both normalised: equal limbs, or both the header's infinity"""
    if G.is_normalised_infinity(want):
        return G.is_normalised_infinity(got)
    return np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------------- the checker itself
@pytest.mark.parametrize("side", ["after", "before"])
def test_a_planted_byte_is_reported_with_side_and_offset(ctx, side):
    """one byte written through mi_dev_upload just past a payload, or just before it: check() names that side and offset 0"""
    b = Banded(ctx, 64 * 65, name="planted")
    try:
        b.check()
        addr = b.ptr + b.nbytes if side == "after" else b.ptr - 1
        b._put(addr, b._get(addr, 1) ^ np.uint8(0x5A))
        with pytest.raises(AssertionError) as e:
            b.check()
        msg = str(e.value)
        assert f"guard {side} the payload touched: 1 bytes changed, nearest at offset 0, farthest at offset 0" in msg
        assert ("guard before" if side == "after" else "guard after") not in msg
        assert np.array_equal(b.download(b.nbytes, np.uint8), b.initial())       # the payload itself was not touched
    finally:
        b.free()


# ---------------------------------------------------------------------------------------------------- mi_field_op_dev
def _field_want(field, op, x, y):
    if op <= 5:
        return cref.field_op(field, op, x, y)
    mod = P.Q_MOD if field else P.R_MOD
    ri = pow(1 << 256, -1, mod)
    xs, ys = ([cref.limbs_to_int(v) for v in a] for a in (x, y))
    f = {6: lambda a, b: 2 * a * b, 7: lambda a, b: a * b - b * b, 8: lambda a, b: a * a}[op]
    return np.array([cref.int_to_limbs(f(a, b) * ri % mod) for a, b in zip(xs, ys)], np.uint64).reshape(-1, 4)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("n", BD.FIELD_NS)
@pytest.mark.parametrize("field", [0, 1])
def test_field_op_dev(ctx, field, n, in_place):
    """ops 0..8 over Fr and Fp; out of place, and z == x in place"""
    x, y = BD.nonzero_scalars(n, 8100 + n), BD.nonzero_scalars(n, 8200 + n)      # below r, so reduced in both fields
    with Bands(ctx) as bs:
        dy = bs.inp(y, "y")
        dx = bs.inout(x, "x (also z)") if in_place else bs.inp(x, "x")
        dz = dx if in_place else bs.out(32 * n, "z")
        for op in range(9):
            if in_place:
                dx.upload(x)
            else:
                dz.refill()
            ctx.field_op_dev(field, op, dz.ptr, dx.ptr, dy.ptr, n)
            bs.settle(f"field {field} op {op}")
            assert np.array_equal(dz.download((n, 4)), _field_want(field, op, x, y)), (field, op, n, in_place)


# ---------------------------------------------------------------------------------------------------- the generators
@pytest.mark.parametrize("n", BD.GEN_NS)
def test_generators_dev(ctx, n):
    with Bands(ctx) as bs:
        for dist in (0, 1):
            d = bs.out(32 * n, f"scalars dist {dist}")
            ctx._ck(ctx.lib.mi_gen_scalars_dev(ctx.h, C.c_void_p(d.ptr), C.c_size_t(n), C.c_uint64(8300 + n), C.c_int(dist)))
            bs.settle("mi_gen_scalars_dev")
            assert np.array_equal(d.download((n, 4)), cref.gen_scalars(n, 8300 + n, dist))
        d1 = bs.out(64 * n, "G1 points")
        ctx._ck(ctx.lib.mi_gen_g1_dev(ctx.h, C.c_void_p(d1.ptr), C.c_size_t(n), C.c_uint64(8310 + n)))
        bs.settle("mi_gen_g1_dev")
        assert np.array_equal(d1.download((n, 8)), cref.gen_g1(n, 8310 + n))
        d2 = bs.out(128 * n, "G2 points")
        ctx._ck(ctx.lib.mi_gen_g2_dev(ctx.h, C.c_void_p(d2.ptr), C.c_size_t(n), C.c_uint64(8320 + n)))
        bs.settle("mi_gen_g2_dev")
        assert np.array_equal(d2.download((n, 16)), cref.gen_g2(n, 8320 + n))


# ---------------------------------------------------------------------------------------------------- mi_ntt_dev
@pytest.mark.parametrize("log_n,plan,wave", BD.NTT_ROWS)
def test_ntt_dev(ctx, log_n, plan, wave):
    """all 8 flag values, in place: the default plan from one element to two tiles, three and four passes under small plans, the
    wavefront stages on and off"""
    n = 1 << log_n
    a = BD.nonzero_scalars(n, 8400 + log_n)
    lib = ctx.lib
    with Bands(ctx) as bs:
        d = bs.inout(a, "inout")
        try:
            if plan:
                assert lib.mi_debug_set_ntt_plan(ctx.h, *plan) == 0
            if wave:
                assert lib.mi_debug_set_ntt_wave_stages(ctx.h, *wave) == 0
            for flags in range(8):
                d.upload(a)
                ctx.ntt_dev(d.ptr, log_n, flags)
                bs.settle(f"mi_ntt_dev flags {flags}")
                assert np.array_equal(d.download((n, 4)), cref.ntt(a, log_n, flags)), (log_n, plan, wave, flags)
        finally:
            assert lib.mi_debug_set_ntt_plan(ctx.h, *BD.DEFAULT_PLAN) == 0 and lib.mi_debug_set_ntt_wave_stages(ctx.h, *BD.DEFAULT_WAVE) == 0


# ---------------------------------------------------------------------------------------------------- mi_compute_h_dev
@pytest.mark.parametrize("log_n,plan", BD.H_ROWS)
def test_compute_h_dev(ctx, log_n, plan):
    """a, b, c hold exactly n_constraints elements: the guard begins where the zero padding begins.  c given and c == NULL, every
    launch fused and none; under plan (8, 7, 7) at log_n = 14 the pair, the triple and the last fused launch all run"""
    N = 1 << log_n
    lib = ctx.lib
    try:
        if plan:
            assert lib.mi_debug_set_ntt_plan(ctx.h, *plan) == 0
        for nc in BD.h_constraint_counts(log_n):
            a, b, c = (BD.nonzero_scalars(nc, 8500 + 10 * log_n + k) for k in range(3))
            want = {True: cref.compute_h(log_n, a, b, c), False: cref.compute_h(log_n, a, b, cref.field_op(0, 2, a, b))}
            with Bands(ctx) as bs:
                da, db, dc = bs.inp(a, "a"), bs.inp(b, "b"), bs.inp(c, "c")
                dh = bs.out(32 * N, "h")
                for fuse in (7, 0):
                    assert lib.mi_debug_set_ntt_fuse_pair(ctx.h, fuse) == 0
                    for given in (True, False):
                        dh.refill()
                        ctx.compute_h_dev(log_n, da.ptr, db.ptr, dc.ptr if given else None, nc, dh.ptr)
                        bs.settle(f"mi_compute_h_dev log_n {log_n}, {nc} constraints, fuse {fuse}, c {'given' if given else 'NULL'}")
                        assert np.array_equal(dh.download((N, 4)), want[given]), (log_n, nc, fuse, given)
    finally:
        assert lib.mi_debug_set_ntt_fuse_pair(ctx.h, 7) == 0 and lib.mi_debug_set_ntt_plan(ctx.h, *BD.DEFAULT_PLAN) == 0


# ---------------------------------------------------------------------------------------------------- the generic MSMs
def _msm_case(n, g2):
    if n >= 300:
        return G.case(n, [4], g2, 8600 + g2)
    pts = (cref.gen_g2 if g2 else cref.gen_g1)(n, 8610 + n)
    sc = cref.gen_scalars(n, 8620 + n, 1)
    sc[n - 1] = fr_arr([P.R_MOD - 1])[0]
    if n > 3:
        pts[2] = 0; sc[1] = 0
    return pts, sc


@pytest.mark.parametrize("g2", [False, True])
@pytest.mark.parametrize("n", BD.MSM_NS + (G.small_n(4),))
def test_msm_dev(ctx, n, g2):
    pts, sc = _msm_case(n, g2)
    want = (cref.msm_g2 if g2 else cref.msm_g1)(pts, sc)
    with Bands(ctx) as bs:
        dp, ds = bs.inp(pts, "points"), bs.inp(sc, "scalars")
        got = (ctx.msm_g2_dev if g2 else ctx.msm_g1_dev)(dp.ptr, ds.ptr, n)
        bs.settle("mi_msm_g2_dev" if g2 else "mi_msm_g1_dev")
        assert _jac_eq(got, want), (n, g2)


# ---------------------------------------------------------------------------------------------------- fixed-base tables and their MSMs
_TABLES = {}


def _table_case(g2):
    """65 bases (one at infinity) and their window table at c = 17 by pyref doublings: row [w][i] = 2^(17 w) P_i.  Made once; the
    smaller sizes take the first n bases"""
    if g2 not in _TABLES:
        n, c = max(BD.FIXED_NS), BD.FIXED_C
        pts = (cref.gen_g2 if g2 else cref.gen_g1)(n, 8700 + g2)
        pts[3] = 0
        add, to_pts, to_arr = (P.g2_add, g2_pts, g2_arr) if g2 else (P.g1_add, g1_pts, g1_arr)
        rows = [to_pts(pts)]
        for _ in range(1, FB.nwin(c)):
            cur = rows[-1]
            for _ in range(c):
                cur = [add(q, q) for q in cur]
            rows.append(cur)
        table = np.stack([to_arr(row) for row in rows])                 # (nwin, n, 8 or 16)
        table.setflags(write=False); pts.setflags(write=False)
        _TABLES[g2] = (pts, table)
    return _TABLES[g2]


@pytest.mark.parametrize("g2", [False, True])
@pytest.mark.parametrize("n", BD.FIXED_NS)
def test_fixed_base_tables_dev(ctx, n, g2):
    """precompute into a table of exactly ceil(256 / c) n points, the MSM on it, the conversion to R' in place, the MSM on that"""
    c, k = BD.FIXED_C, (4 if g2 else 2)
    all_pts, table = _table_case(g2)
    pts = np.ascontiguousarray(all_pts[:n])
    want_table = np.ascontiguousarray(table[:, :n]).reshape(FB.nwin(c) * n, 4 * k)
    sc = cref.gen_scalars(n, 8710 + n, 0)
    edge = G.width_scalars(c)
    sc[:min(n, len(edge))] = fr_arr(edge[:n])
    want = (cref.msm_g2 if g2 else cref.msm_g1)(pts, sc)
    rows = FB.nwin(c) * n
    lib = ctx.lib
    with Bands(ctx) as bs:
        dp, ds = bs.inp(pts, "bases"), bs.inp(sc, "scalars")
        pre = bs.out(16 * k * rows * 2, "table")
        f = lib.mi_msm_precompute_g2_dev if g2 else lib.mi_msm_precompute_g1_dev
        ctx._ck(f(ctx.h, C.c_void_p(dp.ptr), C.c_size_t(n), C.c_uint32(c), C.c_void_p(pre.ptr)))
        bs.settle("mi_msm_precompute")
        assert np.array_equal(pre.download((rows, 4 * k)), want_table), "table rows against pyref doublings"
        bs.const.append((pre, want_table))                              # const for the MSM that follows
        assert _jac_eq(ctx.msm_fixed_dev(pre.ptr, ds.ptr, n, c, flags=0, g2=g2), want), "standard table"
        bs.settle("mi_msm_fixed_dev, standard table")
        bs.const.pop()
        ctx.msm_table_to_rprime(pre.ptr, rows, g2=g2)
        bs.settle("mi_msm_table_to_rprime")
        after = pre.download((rows, 4 * k))
        assert FB.limbs_to_words(after, k) == FB.times32(FB.limbs_to_words(want_table, k)), "R' rows"
        bs.const.append((pre, after))
        assert _jac_eq(ctx.msm_fixed_dev(pre.ptr, ds.ptr, n, c, flags=RPRIME, g2=g2), want), "R' table"
        bs.settle("mi_msm_fixed_dev, R' table")


# ---------------------------------------------------------------------------------------------------- batch scalar multiplication
@pytest.mark.parametrize("g2", [False, True])
@pytest.mark.parametrize("n", BD.BSM_NS)
def test_batch_scalar_mul_dev(ctx, n, g2):
    """the conversion to affine walks groups of 16: 0, 1, r - 1 in front, an infinity output at the ragged end"""
    base = (cref.gen_g2 if g2 else cref.gen_g1)(1, 8800 + g2)[0]
    sc = BD.bsm_scalars(n, 8810 + n)
    want = cref.batch_scalar_mul(base, sc, g2=g2)
    assert not want[n - 1].any()
    with Bands(ctx) as bs:
        ds = bs.inp(sc, "scalars")
        do = bs.out((128 if g2 else 64) * n, "out")
        ctx.batch_scalar_mul_dev(base, ds.ptr, n, do.ptr, g2=g2)
        bs.settle("mi_batch_scalar_mul_dev")
        assert np.array_equal(do.download(want.shape), want), (n, g2)


# ---------------------------------------------------------------------------------------------------- the bulk codecs
@pytest.mark.parametrize("g2", [False, True])
@pytest.mark.parametrize("n", BD.CODEC_NS)
def test_codecs_dev(ctx, n, g2):
    """the byte strings at an odd address, as in a stream; decode from the compressed form, encode to both"""
    B = load_binding()
    pts = K.codec_points(n, 8900 + n, g2)
    arr = g2_arr(pts) if g2 else g1_arr(pts)
    enc = K.g2_enc if g2 else K.g1_enc
    blobs = {e: b"".join(enc(q, e) for q in pts) for e in (K.COMPRESSED, K.RAW)}
    with Bands(ctx) as bs:
        src = bs.inp(np.frombuffer(blobs[K.COMPRESSED], np.uint8), "compressed strings", odd=True)
        dst = bs.out(arr.nbytes, "points")
        rc, first = ctx.decompress_dev(src.ptr, n, dst.ptr, g2, B.KEYFILE_NO_SUBGROUP_CHECK if g2 else 0)
        bs.settle("decompress")
        assert (rc, first) == (0, B.NO_BAD_INDEX) and np.array_equal(dst.download(arr.shape), arr)
        dp = bs.inp(arr, "points to encode")
        for e in (K.COMPRESSED, K.RAW):
            out = bs.out(len(blobs[e]), f"encoding {e}", odd=True)
            ctx.compress_dev(dp.ptr, n, out.ptr, g2, e)
            bs.settle(f"compress, encoding {e}")
            assert bytes(out.download(len(blobs[e]), np.uint8)) == blobs[e], (n, g2, e)


# ---------------------------------------------------------------------------------------------------- the verifier's bulk kernels
@pytest.fixture(scope="module")
def emu_combined(tmp_path_factory):
    return C.CDLL(VC.build_emu(str(tmp_path_factory.mktemp("emu") / "libemu_verify_combined.so")))


@pytest.fixture(scope="module")
def emu_locate(tmp_path_factory):
    return C.CDLL(LC.build_emu(str(tmp_path_factory.mktemp("emu") / "libemu_verify_locate.so")))


@pytest.mark.parametrize("n", BD.VERIFY_NS)
def test_fp12_product_dev(ctx, emu_combined, n):
    rng = np.random.default_rng(9000 + n)
    X = V.gt_arr([[int.from_bytes(rng.bytes(31), "little") for _ in range(12)] for _ in range(n)])
    with Bands(ctx) as bs:
        dx = bs.inp(X, "x")
        do = bs.out(384, "out")
        ctx._ck(ctx.lib.mi_debug_fp12_product_dev(ctx.h, C.c_void_p(dx.ptr), C.c_size_t(n), C.c_void_p(do.ptr)))
        bs.settle("mi_debug_fp12_product_dev")
        assert np.array_equal(do.download((48,)), VC.emu_product(emu_combined, X))


def _verifier_points(n, seed):
    pts = V.seeded_pairs(n, seed, inf_first_last=False)[0]
    if n > 1:
        pts[5] = None; pts[n - 1] = None
    return pts


@pytest.mark.parametrize("n", BD.VERIFY_NS)
def test_g1_scale128_dev(ctx, emu_combined, n):
    rng = np.random.default_rng(9100 + n)
    pa = g1_arr(_verifier_points(n, 9110 + n))
    ks = ([M128, 0, 1, 2, 1 << 127, 1 << 64] + [int.from_bytes(rng.bytes(16), "little") for _ in range(n)])[:n]
    kk = np.array([[k & (1 << 64) - 1, k >> 64] for k in ks], np.uint64)
    with Bands(ctx) as bs:
        dp, dk = bs.inp(pa, "p"), bs.inp(kk, "k")
        do = bs.out(64 * n, "out")
        ctx._ck(ctx.lib.mi_debug_g1_scale128_dev(ctx.h, C.c_void_p(dp.ptr), C.c_void_p(dk.ptr), C.c_size_t(n), C.c_void_p(do.ptr)))
        bs.settle("mi_debug_g1_scale128_dev")
        assert np.array_equal(do.download((n, 8)), VC.emu_scale128(emu_combined, pa, ks))


@pytest.mark.parametrize("n", BD.VERIFY_NS)
def test_g1_sum_tree_dev(ctx, emu_locate, n):
    pa = g1_arr(_verifier_points(n, 9200 + n))
    want = LC.emu_sum_tree(emu_locate, pa)
    with Bands(ctx) as bs:
        dp = bs.inp(pa, "p")
        do = bs.out(64 * len(want), "levels")
        ctx._ck(ctx.lib.mi_debug_g1_sum_tree_dev(ctx.h, C.c_void_p(dp.ptr), C.c_size_t(n), C.c_void_p(do.ptr)))
        bs.settle("mi_debug_g1_sum_tree_dev")
        assert np.array_equal(do.download(want.shape), want)


# ---------------------------------------------------------------------------------------------------- the proof
_PROVE = {}


def _prove_case(log_n):
    """a satisfied toy circuit of N - 11 constraints: the key by the definition, the solver's vectors and the oracle's proof"""
    if log_n not in _PROVE:
        nc = (1 << log_n) - 11
        cs = P.ToyR1CS(nc, 5, 9300 + log_n, 0.5); td = P.ToyTrapdoor(9300 + log_n)
        pk, exps, _ = _toy_setup_exps_only(cs, td)
        assert pk["log_n"] == log_n
        key = _toy_key_from_exps(cs, td, pk, exps)
        w, a, b, c = cs.solve()
        rng = P.SplitMix64(9310 + log_n)
        W, a, b, c = fr_arr(w), fr_arr(a), fr_arr(b), fr_arr(c)
        rs = fr_arr([rng.fr()])[0], fr_arr([rng.fr()])[0]
        assert len(a) == nc and np.array_equal(cref.field_op(0, 2, a, b), c)
        for v in (W, a, b, c):
            v.setflags(write=False)
        _PROVE[log_n] = dict(key=key, W=W, a=a, b=b, c=c, r=rs[0], s=rs[1], want=cref.prove(key, W, a, b, c, *rs)["raw"])
    return _PROVE[log_n]


@pytest.mark.parametrize("log_n", BD.PROVE_LOG_NS)
def test_prove_dev_on_a_banded_key(ctx, log_n):
    """mi_pk_load_dev adopts five banded point arrays; W, a, b, c banded; c given and NULL.  The key's arrays and their guards are
    unchanged after the proofs and after mi_pk_free"""
    B = load_binding()
    g = _prove_case(log_n)
    key = g["key"]
    names =("g1_a", "g1_b", "g1_k", "g1_z", "g2_b")
    with Bands(ctx) as bs:
        arrays = {nm: bs.inp(key[nm], nm) for nm in names}
        dW, da, db, dc = (bs.inp(g[nm], nm) for nm in "Wabc")
        desc = dict(key)
        desc.update({nm: (arrays[nm].ptr, key[nm].shape[0]) for nm in names})
        pkh = ctx.pk_load(desc, device_points=True)
        try:
            bs.settle("mi_pk_load_dev")
            for given in (True, False):
                proof, _ = ctx.prove(pkh, dW.ptr, da.ptr, db.ptr, dc.ptr if given else None, g["r"], g["s"], device=True,
                                     n_wires=len(g["W"]), n_constraints=len(g["a"]))
                bs.settle(f"mi_groth16_prove_dev, c {'given' if given else 'NULL'}")
                assert B.proof_write(proof["raw"]) == cref.proof_write(g["want"]), (log_n, given)
        finally:
            ctx.pk_free(pkh)
        bs.settle("mi_pk_free")

"""GPU: a call's result does not depend on what its context did before.  Every scratch buffer of a context only grows and is never
cleared (mi_ctx::ws[], the MsmSlot::buf[] arrays, the NTT tables, the pool's input sets), so a kernel that relies on a workspace being
zero, walks a count left by a larger call, or reads a bucket, histogram, sorted entry or staged vector beyond the current size is right
on a fresh context and wrong later.  Each scenario runs a probe P on a FRESH context against the reference, then a dirtying call D with
other data on the same context, then P again for the same bits, through its sequence, and ends with mi_ctx_trim and P once more.
tests/test_banded_cpu.py asserts that the dirtying inputs fill what the probes must not look at.

1  computeH shrinking at one log_n: 1024, 1013, 513, 1 constraints, then log_n = 12, then 1 again; host staging and device pointers
2  generic MSMs at a pinned window width: every window full, then five sparse probes
3  fixed-base MSMs: a table of 600 under full-width scalars, then a table of 65 under edge scalars, zeros and a lone scalar
4  batch scalar multiplication: 1000, then 65 with zeros where the first group of 16 was
5  proofs: a log_n = 12 key, then a log_n = 10 key with an ordinary and an all-zero witness, host and device inputs
6  the pool's input set: a log_n = 12 job, then a shorter job in the same staged vectors"""
import time
import numpy as np
import pytest
import cref
import banded as BD
import fixed_base_cases as FB
import generic_msm_cases as G
from helpers import fr_arr
from gpu_common import load_binding
from test_gpu_buffer_bounds import _prove_case, _jac_eq

pytestmark = pytest.mark.gpu
RPRIME = 2   # MI_MSM_TABLE_RPRIME


@pytest.fixture(scope="module", autouse=True)
def _wall():
    t0 = time.perf_counter()
    yield
    print(f"\ntests/test_gpu_call_history.py: {time.perf_counter() - t0:.1f} s wall from its first test to its last")


@pytest.fixture()
def ctx():
    """a fresh context for every test: the first probe of a scenario meets workspaces nobody has used"""
    c = load_binding().Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------------- 1: computeH shrinking
_H = {}


def _h_inputs():
    if not _H:
        a, b, c = BD.shrinking_vectors(7000)
        _H["abc"] = (a, b, c, cref.field_op(0, 2, a, b))
        N = 1 << BD.H_BIG_LOG_N
        big = tuple(BD.nonzero_scalars(N, 7010 + k) for k in range(3))
        _H["big"] = big + (cref.field_op(0, 2, big[0], big[1]),)
        _H["want"] = {}
    return _H


def _h_want(key, log_n, a, b, c):
    w = _h_inputs()["want"]
    if key not in w:
        w[key] = cref.compute_h(log_n, a, b, c)
        w[key].setflags(write=False)
    return w[key]


def _h_step(ctx, which, log_n, nc, given, what):
    """one computeH through the host entry point and one through the device entry point, both against the oracle"""
    a, b, c, ab = _h_inputs()[which]
    a, b, cc = a[:nc], b[:nc], (c if given else ab)[:nc]
    want = _h_want((which, nc, given), log_n, a, b, cc)
    assert np.array_equal(ctx.compute_h(log_n, a, b, cc if given else None), want), f"{what}: mi_compute_h"
    bufs = [ctx.to_dev(x) for x in ((a, b, cc) if given else (a, b))] + [ctx.alloc(32 << log_n)]
    try:
        ctx.compute_h_dev(log_n, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr if given else None, nc, bufs[-1].ptr)
        assert np.array_equal(bufs[-1].download((1 << log_n, 4)), want), f"{what}: mi_compute_h_dev"
    finally:
        for d in bufs:
            d.free()


@pytest.mark.parametrize("fuse", [7, 0])
@pytest.mark.parametrize("given", [True, False])
def test_compute_h_shrinking(ctx, given, fuse):
    """every element of the longer vectors is non-zero: what a shorter call must pad with zeros is there, in the staging workspace
    and in the two working vectors, from the call before"""
    lib = ctx.lib
    try:
        assert lib.mi_debug_set_ntt_fuse_pair(ctx.h, fuse) == 0
        for nc in BD.H_SHRINK:
            _h_step(ctx, "abc", BD.H_LOG_N, nc, given, f"{nc} constraints")
        _h_step(ctx, "big", BD.H_BIG_LOG_N, 1 << BD.H_BIG_LOG_N, given, "log_n = 12, full")
        _h_step(ctx, "abc", BD.H_LOG_N, 1, given, "1 constraint after log_n = 12")
        _h_step(ctx, "abc", BD.H_LOG_N, 1013, given, "1013 constraints after 1")
        ctx.trim()
        _h_step(ctx, "abc", BD.H_LOG_N, 1, given, "1 constraint after the trim")
        _h_step(ctx, "abc", BD.H_LOG_N, 513, given, "513 constraints after the trim")
    finally:
        assert lib.mi_debug_set_ntt_fuse_pair(ctx.h, 7) == 0


# ---------------------------------------------------------------------------------------------------- 2: generic MSMs
_MSM = {}


def _msm_inputs(g2):
    if g2 not in _MSM:
        msm = cref.msm_g2 if g2 else cref.msm_g1
        n = G.small_n(BD.MSM_C)
        deg = G.degenerate_sets(300, 7110 + g2, g2)
        probes = [("case", ) + G.case(n, [BD.MSM_C], g2, 7100 + g2)]
        probes += [(name,) + deg[name] for name in ("zero", "lone_first", "lone_last", "all_infinity")]
        probes = [(name, pts, sc, msm(pts, sc)) for name, pts, sc in probes]
        assert G.is_normalised_infinity(probes[1][3]) and G.is_normalised_infinity(probes[4][3])
        dpts = (cref.gen_g2 if g2 else cref.gen_g1)(BD.MSM_DIRTY_N, 7120 + g2)
        vals = BD.msm_dirty_scalars()
        dirty = [(name, dpts, np.ascontiguousarray(np.tile(fr_arr([v]), (BD.MSM_DIRTY_N, 1)))) for name, v in vals.items()]
        dirty = [(name, pts, sc, msm(pts, sc)) for name, pts, sc in dirty]
        _MSM[g2] = (probes, dirty)
    return _MSM[g2]


@pytest.mark.parametrize("g2", [False, True])
def test_generic_msm_after_a_fuller_one(ctx, g2):
    """the window width pinned to 8, so that D and P share their bucket and sort arrays: D leaves n = 5000 entries in one key of every
    window; P has a few hundred entries, none at all (infinity), one in the first window, one in the last, or only infinity bases"""
    probes, dirty = _msm_inputs(g2)
    host = ctx.msm_g2 if g2 else ctx.msm_g1
    dev = ctx.msm_g2_dev if g2 else ctx.msm_g1_dev

    def run(case, what):
        name, pts, sc, want = case
        assert _jac_eq(host(pts, sc), want), f"{name} {what}: host entry point"
        dp, ds = ctx.to_dev(pts), ctx.to_dev(sc)
        try:
            assert _jac_eq(dev(dp.ptr, ds.ptr, len(pts)), want), f"{name} {what}: device entry point"
        finally:
            dp.free(); ds.free()

    try:
        assert ctx.lib.mi_debug_set_msm_plan(ctx.h, BD.MSM_C, 0, 0, 0, 0) == 0
        run(probes[0], "on a fresh context")
        for p in probes:
            for d in dirty:
                run(d, "(dirtying)")
                run(p, f"after {d[0]}")
        ctx.trim()
        for p in probes:
            run(p, "after the trim")
    finally:
        assert ctx.lib.mi_debug_set_msm_plan(ctx.h, 0, 0, 0, 0, 0) == 0


# ---------------------------------------------------------------------------------------------------- 3: fixed-base MSMs
_FIXED = {}


def _fixed_inputs(g2):
    if g2 not in _FIXED:
        gen, msm = (cref.gen_g2, cref.msm_g2) if g2 else (cref.gen_g1, cref.msm_g1)
        big, small = gen(BD.FIXED_DIRTY_N, 7200 + g2), gen(BD.FIXED_PROBE_N, 7210 + g2)
        small[7] = 0
        bsc = BD.nonzero_scalars(BD.FIXED_DIRTY_N, 7200)
        probes = [(name, sc, msm(small, sc)) for name, sc in BD.fixed_probe_scalars().items()]
        assert G.is_normalised_infinity(probes[1][2])
        _FIXED[g2] = (big, bsc, msm(big, bsc), small, probes)
    return _FIXED[g2]


@pytest.mark.parametrize("rprime", [False, True])
@pytest.mark.parametrize("g2", [False, True])
def test_fixed_base_msm_after_a_larger_table(ctx, g2, rprime):
    c = BD.FIXED_C
    big, bsc, bwant, small, probes = _fixed_inputs(g2)
    flags = RPRIME if rprime else 0
    bufs = [ctx.to_dev(big), ctx.to_dev(small), ctx.to_dev(bsc)]
    try:
        tabs = [ctx.msm_precompute(bufs[0].ptr, len(big), c, g2=g2), ctx.msm_precompute(bufs[1].ptr, len(small), c, g2=g2)]
        bufs += tabs
        if rprime:
            for t, pts in zip(tabs, (big, small)):
                ctx.msm_table_to_rprime(t.ptr, FB.nwin(c) * len(pts), g2=g2)

        def probe(p, what):
            name, sc, want = p
            ds = ctx.to_dev(sc)
            try:
                assert _jac_eq(ctx.msm_fixed_dev(tabs[1].ptr, ds.ptr, len(small), c, flags=flags, g2=g2), want), f"{name} {what}"
            finally:
                ds.free()

        probe(probes[0], "on a fresh context")
        for p in probes:
            assert _jac_eq(ctx.msm_fixed_dev(tabs[0].ptr, bufs[2].ptr, len(big), c, flags=flags, g2=g2), bwant), "the table of 600"
            probe(p, "after the table of 600")
        ctx.trim()
        for p in probes:
            probe(p, "after the trim")
    finally:
        for d in bufs:
            d.free()


# ---------------------------------------------------------------------------------------------------- 4: batch scalar multiplication
@pytest.mark.parametrize("g2", [False, True])
def test_batch_scalar_mul_after_a_larger_batch(ctx, g2):
    """D's first group of 16 and its entry 64 are non-zero scalars; P has zeros exactly there: infinity outputs where D left points"""
    base = (cref.gen_g2 if g2 else cref.gen_g1)(2, 7400 + g2)
    big, small = BD.nonzero_scalars(BD.BSM_DIRTY_N, 7401), BD.bsm_probe_scalars(7400)
    want_big, want = cref.batch_scalar_mul(base[0], big, g2=g2), cref.batch_scalar_mul(base[1], small, g2=g2)
    assert not want[:16].any() and not want[64].any() and want[16:64].any(axis=1).all()

    def run(b, sc, w, what):
        assert np.array_equal(ctx.batch_scalar_mul(b, sc, g2=g2), w), f"{what}: host entry point"
        ds = ctx.to_dev(sc); do = ctx.alloc(w.nbytes)
        try:
            ctx.batch_scalar_mul_dev(b, ds.ptr, len(sc), do.ptr, g2=g2)
            assert np.array_equal(do.download(w.shape), w), f"{what}: device entry point"
        finally:
            ds.free(); do.free()

    run(base[1], small, want, "65 on a fresh context")
    run(base[0], big, want_big, "1000")
    run(base[1], small, want, "65 after 1000")
    ctx.trim()
    run(base[1], small, want, "65 after the trim")


# ---------------------------------------------------------------------------------------------------- 5: proofs
def _zero_witness(g):
    """wire 0 = 1, every other wire 0, a = b = c = 0: every scalar of four of the five MSMs is zero but one, and h is zero"""
    key = g["key"]
    W = np.zeros_like(g["W"]); W[0] = fr_arr([1])[0]
    z = np.zeros_like(g["a"])
    if "want_zero" not in g:
        g["want_zero"] = cref.proof_write(cref.prove(key, W, z, z, z, g["r"], g["s"])["raw"])
    return W, z, g["want_zero"]


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("device", [False, True])
def test_proofs_large_then_small(ctx, device, fused):
    """one context, a log_n = 12 key and a log_n = 10 key: large, small, small with the all-zero witness, small again, large again, and
    after a trim small once more.  17-bit tables are forced for the Z MSM so that its digit count can ride in computeH's last launch
    (knob z_count_fused); the counter shows that it did, or with the knob off that it did not"""
    B = load_binding()
    big, small = _prove_case(12), _prove_case(10)
    Wz, z, want_zero = _zero_witness(small)
    held = []

    def prove(pkh, W, a, b, c, g):
        if not device:
            return ctx.prove(pkh, W, a, b, c, g["r"], g["s"])[0]
        bufs = [ctx.to_dev(x) for x in (W, a, b, c)]
        held.extend(bufs)
        return ctx.prove(pkh, *(d.ptr for d in bufs), g["r"], g["s"], device=True, n_wires=len(W), n_constraints=len(a))[0]

    keys = []
    try:
        assert ctx.lib.mi_debug_set_prove_fixed_base(ctx.h, 17, 17, 17) == 0
        ctx.set_knob("z_count_fused", fused)
        keys = [ctx.pk_load(big["key"]), ctx.pk_load(small["key"])]
        assert ctx.pk_table_plan(keys[0])[2] == 17 and ctx.pk_table_plan(keys[1])[2] == 17
        steps = [("large", 0, big, None), ("small", 1, small, None), ("small, all-zero witness", 1, small, (Wz, z, want_zero)),
                 ("small again", 1, small, None), ("large again", 0, big, None), ("trim", None, None, None), ("small after the trim", 1, small, None)]
        for what, k, g, other in steps:
            if k is None:
                ctx.trim()
                continue
            before = ctx.counter("z_count_fused_launches")
            if other:
                got = prove(keys[k], other[0], other[1], other[1], other[1], g)
                want = other[2]
            else:
                got = prove(keys[k], g["W"], g["a"], g["b"], g["c"], g)
                want = cref.proof_write(g["want"])
            assert B.proof_write(got["raw"]) == want, what
            # both domains qualify under the default NTT plan: the last pass has radix 2^9 and its tile of 512 elements is one slice
            # of the Z sort, whose slices cover the domain exactly (csrc/ntt.hip mi_compute_h_part, csrc/msm.hip mi_msm_z_count_arm)
            assert ctx.counter("z_count_fused_launches") == before + fused, f"{what}: the fused count ran with the knob on, and only then"
    finally:
        ctx.set_knob("z_count_fused", 1)
        assert ctx.lib.mi_debug_set_prove_fixed_base(ctx.h, 0, 0, 0) == 0
        for k in keys:
            ctx.pk_free(k)
        for d in held:
            d.free()


# ---------------------------------------------------------------------------------------------------- 6: the pool's input set
def test_pool_short_job_after_a_long_one():
    """in_flight = 1, host inputs: the log_n = 12 job sizes the input set, the log_n = 10 job of N - 11 constraints is staged into the
    front of the same vectors, which are longer than the job and hold the first job's values behind it"""
    B = load_binding()
    big, small = _prove_case(12), _prove_case(10)
    assert len(small["a"]) == (1 << 10) - 11 and len(big["a"]) > 4 * len(small["a"])
    pool = B.Prover(0, 1)
    single = B.Context(0)
    keys = []
    try:
        c0 = pool.ctx(0)
        keys = [c0.pk_load(big["key"]), c0.pk_load(small["key"])]
        direct = {}
        for k, g, name in ((1, small, "small"), (0, big, "big")):
            for given in (True, False):
                direct[(name, given)] = B.proof_write(single.prove(keys[k], g["W"], g["a"], g["b"], g["c"] if given else None, g["r"], g["s"])[0]["raw"])
                assert direct[(name, given)] == cref.proof_write(g["want"])
        for given in (True, False):
            for k, g, name in ((0, big, "big"), (1, small, "small"), (1, small, "small")):
                t = pool.submit(keys[k], g["W"], g["a"], g["b"], g["c"] if given else None, g["r"], g["s"])
                assert B.proof_write(pool.wait(t)[0]["raw"]) == direct[(name, given)], (name, given)
        pool.trim()
        t = pool.submit(keys[1], small["W"], small["a"], small["b"], small["c"], small["r"], small["s"])
        assert B.proof_write(pool.wait(t)[0]["raw"]) == direct[("small", True)], "after the trim"
    finally:
        for k in keys:
            pool.ctx(0).pk_free(k)
        single.close()
        pool.close()

"""GPU: the device-resident R1CS and the proofs from W alone (include/mi355x_groth16_r1cs.h, csrc/r1cs.hip).  Every comparison is exact.

1  against the definition: pyref.ToyR1CS circuits, A W / B W / C W against the solver's a, b, c; the constraint check
2  skew, size, coefficient classes: seeded R1CS at 2^16 and 2^20 rows (tests/r1cs_cases.py) against the host reference
3  proofs: prove_w and the pool's submit_w* return the bytes of the existing entry points given a = A W, b = B W
4  refusals: what Setup refuses of a descriptor, null arguments, keys and wire vectors that do not fit
5  lifetime: bytes held, the ledger, trim
"""
import ctypes as C
import time
import numpy as np
import pytest
import pyref as P
import cref
import dlog_keys as D
import setup_cases as S
import r1cs_cases as RC
from helpers import fr_arr, toy_pk_arrays
from gpu_common import load_binding
from test_gpu_setup import _toy_setup_exps_only, _toy_key_from_exps, _refusals, _small

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    B = load_binding()
    t0 = time.perf_counter()
    c = B.Context(0)
    yield c
    c.close()
    print(f"\ntests/test_gpu_r1cs.py: {time.perf_counter() - t0:.1f} s wall from its first test to its last")


def _same(p, q):
    return np.array_equal(p["raw"], q["raw"])


# ---------------------------------------------------------------------------------------------------- 1: against the definition
@pytest.mark.parametrize("small_frac", [0.0, 0.9])
@pytest.mark.parametrize("nc", [100, 1000, 4096])
def test_r1cs_eval_against_the_definition(ctx, nc, small_frac):
    cs = P.ToyR1CS(nc, 5, nc + int(small_frac * 10), small_frac)
    w, a, b, c = cs.solve()
    r1cs, W = S.toy_r1cs(cs), fr_arr(w)
    rh = ctx.r1cs_load(r1cs)
    try:
        for have, want, name in zip(ctx.r1cs_eval(rh, W, nc), (a, b, c), "abc"):
            assert np.array_equal(have, fr_arr(want)), name
        assert ctx.r1cs_check(rh, W) == (0, RC.U64_MAX)
        j = max(next(iter(row[0])) for row in cs.rows)          # a private wire that occurs in some constraint
        W2 = W.copy(); W2[j] = fr_arr([w[j] + 1])[0]
        want = RC.check_rows(*RC.eval_all(r1cs, W2))
        assert want[0] > 0 and ctx.r1cs_check(rh, W2) == want
    finally:
        ctx.r1cs_free(rh)


# ---------------------------------------------------------------------------------------------------- 2: skew, size, classes
@pytest.mark.parametrize("log_n", [16, 20])
def test_r1cs_eval_skew_and_size(ctx, log_n):
    B = load_binding()
    n = (1 << log_n) - 1234                               # not a power of two
    r1cs = RC.skewed_r1cs(n, nb_wires=(1 << log_n) + 777, nb_public=33, seed=log_n)
    W = RC.witness(r1cs["nb_wires"], log_n + 1)
    t0 = time.perf_counter()
    ref = RC.eval_all(r1cs, W)
    print(f"host reference 2^{log_n}: {time.perf_counter() - t0:.1f} s on {cref.num_threads()} threads")
    rh = ctx.r1cs_load(r1cs)
    dW = ctx.to_dev(W)
    try:
        got = ctx.r1cs_eval(rh, W, n)
        st = ctx.r1cs_stats()
        print(f"r1cs_eval 2^{log_n}: {st}")
        for have, want, name in zip(got, ref, "ABC"):
            assert np.array_equal(have, want), f"{name} W (host entry point)"
        n_long, n_pieces = RC.split_counts(r1cs)
        assert n_long > 0 and n_pieces > n_long
        assert (st["matrices"], st["entries"], st["long_rows"], st["pieces"]) == (3, sum(len(r1cs[m][1]) for m in "ABC"), n_long, n_pieces)
        for have, want, name in zip(ctx.r1cs_eval(rh, dW.ptr, n, device=True), ref, "ABC"):
            assert np.array_equal(have, want), f"{name} W (device entry point)"
        a_only, b_only, none = ctx.r1cs_eval(rh, dW.ptr, n, which=B.R1CS_A | B.R1CS_B, device=True)
        assert none is None and np.array_equal(a_only, ref[0]) and np.array_equal(b_only, ref[1])
        st = ctx.r1cs_stats()
        assert (st["matrices"], st["long_rows"], st["pieces"]) == (2,) + RC.split_counts(r1cs, "AB")
        want = RC.check_rows(*ref)
        assert want[0] > n // 2                             # a random W satisfies next to nothing
        assert ctx.r1cs_check(rh, dW.ptr, device=True) == want
    finally:
        dW.free()
        ctx.r1cs_free(rh)


# ---------------------------------------------------------------------------------------------------- 3: proofs
@pytest.mark.parametrize("nc", [100, 1000])
def test_prove_w_toy(ctx, nc):
    B = load_binding()
    seed = nc + 3
    cs = P.ToyR1CS(nc, 5, seed, 0.5); td = P.ToyTrapdoor(seed)
    if nc <= 100:
        pk, exps, _ = P.toy_setup(cs, td)
        pk_arrays = toy_pk_arrays(pk)
    else:
        pk, exps, _ = _toy_setup_exps_only(cs, td)
        pk_arrays = _toy_key_from_exps(cs, td, pk, exps)
    w, a, b, c = cs.solve()
    r1cs, W = S.toy_r1cs(cs), fr_arr(w)
    rng = P.SplitMix64(seed + 1)
    r, s = fr_arr([rng.fr()])[0], fr_arr([rng.fr()])[0]
    a_ref, b_ref, c_ref = RC.eval_all(r1cs, W)
    pkh, _, _ = ctx.setup(r1cs, S.toy_trapdoor(td))
    rh = ctx.r1cs_load(r1cs)
    dW = ctx.to_dev(W)
    try:
        old, _ = ctx.prove(pkh, W, a_ref, b_ref, None, r, s)
        want = cref.prove(pk_arrays, W, fr_arr(a), fr_arr(b), fr_arr(c), r, s)
        assert B.proof_write(old["raw"]) == cref.proof_write(want["raw"])
        for kw in (dict(), dict(flags=B.PROVE_W_EVAL_C)):
            assert _same(ctx.prove_w(pkh, rh, W, r, s, **kw)[0], old), f"host {kw}"
            assert _same(ctx.prove_w(pkh, rh, dW.ptr, r, s, device=True, n_wires=len(W), **kw)[0], old), f"device {kw}"
        st = ctx.r1cs_stats()
        assert st["matrices"] == 3 and st["entries"] == sum(len(r1cs[m][1]) for m in "ABC")
        # a wire vector that does NOT satisfy the constraints: c = C W and c = a o b now differ, and each path follows its own
        j = max(next(iter(row[0])) for row in cs.rows)
        W2 = W.copy(); W2[j] = fr_arr([w[j] + 1])[0]
        a2, b2, c2 = RC.eval_all(r1cs, W2)
        assert RC.check_rows(a2, b2, c2)[0] > 0
        with_c, _ = ctx.prove(pkh, W2, a2, b2, c2, r, s)
        derived, _ = ctx.prove(pkh, W2, a2, b2, None, r, s)
        assert not _same(with_c, derived)
        assert _same(ctx.prove_w(pkh, rh, W2, r, s, flags=B.PROVE_W_EVAL_C)[0], with_c)
        assert _same(ctx.prove_w(pkh, rh, W2, r, s)[0], derived)
    finally:
        dW.free()
        ctx.r1cs_free(rh)
        ctx.pk_free(pkh)


BIG_LOG_N = 20


@pytest.fixture(scope="module")
def big(ctx):
    """a solvable skewed circuit of 2^20 - 1234 constraints with one commitment, its key from Setup, the resident R1CS, the proof of the
    existing entry point"""
    n = (1 << BIG_LOG_N) - 1234
    r1cs, W, a, b, c = RC.solved_r1cs(n, nb_wires_ab=(1 << 19) + 55, nb_public=33, seed=2020, commitments=1, n_committed=1 << 12)
    td = S.synth_trapdoor(21, n_sigma=1)
    r, s = cref.gen_scalars(2, 22, 0)
    pkh, peds, _ = ctx.setup(r1cs, td)
    rh = ctx.r1cs_load(r1cs)
    old, _ = ctx.prove(pkh, W, a, b, None, r, s)
    yield dict(r1cs=r1cs, td=td, W=W, a=a, b=b, c=c, r=r, s=s, pkh=pkh, ped=peds[0], rh=rh, old=old, n=n)
    ctx.r1cs_free(rh); ctx.pedersen_pk_free(peds[0]); ctx.pk_free(pkh)


def test_prove_w_at_2p20(ctx, big):
    B = load_binding()
    g = big
    assert ctx.r1cs_check(g["rh"], g["W"]) == (0, RC.U64_MAX)
    for have, want, name in zip(ctx.r1cs_eval(g["rh"], g["W"], g["n"]), (g["a"], g["b"], g["c"]), "abc"):
        assert np.array_equal(have, want), name
    dW = ctx.to_dev(g["W"])
    try:
        for kw in (dict(), dict(flags=B.PROVE_W_EVAL_C)):
            p, st = ctx.prove_w(g["pkh"], g["rh"], g["W"], g["r"], g["s"], **kw)
            assert _same(p, g["old"]), f"host {kw}"
            assert _same(ctx.prove_w(g["pkh"], g["rh"], dW.ptr, g["r"], g["s"], device=True, n_wires=len(g["W"]), **kw)[0], g["old"]), f"device {kw}"
        print(f"prove_w 2^{BIG_LOG_N}: {ctx.r1cs_stats()}; h2d_ms {st['h2d_ms']:.2f}")
    finally:
        dW.free()
    # the proof itself, in the exponent
    exps = ctx.setup_exponents(g["r1cs"], g["td"], want=("a", "b", "k", "infinity_a", "infinity_b"))
    e = S.dlog_exps(g["r1cs"], g["td"], exps, BIG_LOG_N)
    D.check_proof(g["old"], D.expected_proof_exps(e, g["W"], g["a"], g["b"], g["r"], g["s"]))


def test_pool_submit_w_matches_submit(ctx, big):
    B = load_binding()
    g = big
    committed = g["r1cs"]["commitments"][0][0]
    vals = np.ascontiguousarray(g["W"][committed])
    ch = cref.gen_scalars(1, 23, 0)[0]
    nw = len(g["W"])
    pool = B.Prover(0, 2)
    dW = ctx.to_dev(g["W"]); da = ctx.to_dev(g["a"]); db = ctx.to_dev(g["b"])
    try:
        # host and device jobs of both kinds mixed on one pool
        t = [pool.submit(g["pkh"], g["W"], g["a"], g["b"], None, g["r"], g["s"]),
             pool.submit_w(g["pkh"], g["rh"], g["W"], g["r"], g["s"]),
             pool.submit_w(g["pkh"], g["rh"], dW.ptr, g["r"], g["s"], device=True, n_wires=nw),
             pool.submit(g["pkh"], dW.ptr, da.ptr, db.ptr, None, g["r"], g["s"], device=True, n_wires=nw, n_constraints=g["n"]),
             pool.submit_w(g["pkh"], g["rh"], g["W"], g["r"], g["s"], flags=B.PROVE_W_EVAL_C),
             pool.submit_bsb22(g["pkh"], g["W"], g["a"], g["b"], None, g["r"], g["s"], [(g["ped"], vals)], ch),
             pool.submit_w_bsb22(g["pkh"], g["rh"], g["W"], g["r"], g["s"], [(g["ped"], vals)], ch),
             pool.submit_w(g["pkh"], g["rh"], dW.ptr, g["r"], g["s"], device=True, n_wires=nw)]
        res = [pool.wait(x) for x in t]
        for i, (p, _) in enumerate(res):
            assert _same(p, g["old"]), f"job {i}"
        assert np.array_equal(res[5][0]["pok"], res[6][0]["pok"]) and res[5][0]["pok"].any()
        assert 0 < res[1][1]["h2d_ms"] and res[2][1]["h2d_ms"] == 0
        # an idle pool trims, and the next job still matches
        pool.trim()
        p, _ = pool.wait(pool.submit_w(g["pkh"], g["rh"], g["W"], g["r"], g["s"]))
        assert _same(p, g["old"])
        with pytest.raises(B.MiError):
            pool.submit_w(g["pkh"], g["rh"], g["W"][:-1], g["r"], g["s"])
    finally:
        pool.close()
        for d in (dW, da, db):
            d.free()


def test_pool_submit_w_bsb22_at_the_benchmark_shape(ctx):
    """log_n 23, the R1CS of test_setup_whole_key_at_the_benchmark_shape: one Setup, one host product, two proofs"""
    B = load_binding()
    N = 1 << 23
    ctx.trim()
    r1cs = S.synth_r1cs(N - 100, nb_wires=N - 1000, nb_public=4097, seed=2222, per_row=3, n_coeffs=1 << 12, n_heavy=64, commitments=1, n_committed=N >> 5)
    td = S.synth_trapdoor(77, n_sigma=1)
    W = cref.gen_scalars(r1cs["nb_wires"], 31, 1); W[0] = D.ONE
    t0 = time.perf_counter()
    a, b = RC.eval_rows(r1cs, "A", W), RC.eval_rows(r1cs, "B", W)
    print(f"host reference of A W, B W at 2^23: {time.perf_counter() - t0:.1f} s")
    r, s = cref.gen_scalars(2, 51, 0)
    ch = cref.gen_scalars(1, 52, 0)[0]
    committed = r1cs["commitments"][0][0]
    vals = np.ascontiguousarray(W[committed])
    pool = B.Prover(0, 2)
    try:
        c0 = pool.ctx(0)
        pkh, peds, _ = c0.setup(r1cs, td)
        rh = c0.r1cs_load(r1cs)
        try:
            print(f"resident R1CS at 2^23: {c0.r1cs_bytes(rh) / 1e9:.3f} GB")
            old, st_old = pool.wait(pool.submit_bsb22(pkh, W, a, b, None, r, s, [(peds[0], vals)], ch))
            new, st_new = pool.wait(pool.submit_w_bsb22(pkh, rh, W, r, s, [(peds[0], vals)], ch))
            print(f"h2d_ms: submit_bsb22 {st_old['h2d_ms']:.1f}, submit_w_bsb22 {st_new['h2d_ms']:.1f}")
        finally:
            c0.r1cs_free(rh); c0.pedersen_pk_free(peds[0]); c0.pk_free(pkh)
    finally:
        pool.close()
    assert _same(new, old) and np.array_equal(new["pok"], old["pok"]) and new["raw"].any()


# ---------------------------------------------------------------------------------------------------- 4: refusals
_R1CS_REFUSALS = sorted(k for k, v in _refusals()[2].items() if not v[1])      # the cases that do not concern the trapdoor


@pytest.mark.parametrize("case", _R1CS_REFUSALS)
def test_r1cs_load_refusals(ctx, case):
    B = load_binding()
    r1cs, _, cases = _refusals()
    dr, _, word = cases[case]
    before = ctx.mem_ledger()
    with pytest.raises(B.MiError) as ei:
        ctx.r1cs_load({**r1cs, **dr})
    assert "rc=-1:" in str(ei.value) and word in str(ei.value), str(ei.value)
    assert ctx.mem_ledger() == before


def test_r1cs_refuses_null_arguments(ctx):
    B = load_binding()
    r1cs, _ = _small()
    d, keep = B._r1cs_desc(r1cs)
    lib, h, v = ctx.lib, C.c_void_p(), C.c_uint64()
    assert len(_R1CS_REFUSALS) == 14
    assert lib.mi_r1cs_load(ctx.h, None, C.byref(h)) == -1 and b"r1cs is null" in lib.mi_last_error(ctx.h)
    assert lib.mi_r1cs_load(ctx.h, C.byref(d), None) == -1
    assert lib.mi_r1cs_load(None, C.byref(d), C.byref(h)) == -1 and not h.value
    rh = ctx.r1cs_load(r1cs)
    try:
        n, nw = r1cs["n_constraints"], r1cs["nb_wires"]
        W = RC.witness(nw, 1)
        out = np.zeros((n, 4), np.uint64)
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        assert lib.mi_r1cs_eval(ctx.h, None, p(W), 1, p(out), None, None) == -1
        assert lib.mi_r1cs_eval(ctx.h, rh, None, 1, p(out), None, None) == -1
        assert lib.mi_r1cs_eval(ctx.h, rh, p(W), 3, p(out), None, None) == -1      # B asked for, no room given
        assert lib.mi_r1cs_eval(ctx.h, rh, p(W), 0, p(out), None, None) == -1 and lib.mi_r1cs_eval(ctx.h, rh, p(W), 8, p(out), None, None) == -1
        assert lib.mi_r1cs_eval_dev(ctx.h, rh, None, 1, None, None, None) == -1
        assert lib.mi_r1cs_check_dev(ctx.h, rh, None, C.byref(v), C.byref(v)) == -1
        assert lib.mi_r1cs_bytes(None, C.byref(v)) == -1 and lib.mi_r1cs_bytes(rh, None) == -1
        assert lib.mi_r1cs_get_stats(ctx.h, None) == -1 and lib.mi_r1cs_free(ctx.h, None) == -1
        assert not out.any()
        got = ctx.r1cs_eval(rh, W, n, which=B.R1CS_C)
        assert got[0] is None and got[1] is None and np.array_equal(got[2], RC.eval_rows(r1cs, "C", W))
    finally:
        ctx.r1cs_free(rh)


def test_prove_w_refuses_what_does_not_fit(ctx):
    B = load_binding()
    cs = P.ToyR1CS(300, 5, 9, 0.5); td = S.toy_trapdoor(P.ToyTrapdoor(9))
    r1cs, W = S.toy_r1cs(cs), fr_arr(cs.wires)
    other = S.toy_r1cs(P.ToyR1CS(600, 5, 9, 0.5))           # another log_n, and other wire counts
    r, s = cref.gen_scalars(2, 5, 0)
    a, b, _ = RC.eval_all(r1cs, W)
    pkh, _, _ = ctx.setup(r1cs, td)
    pk_other, _, _ = ctx.setup(other, td)
    rh, rh_other = ctx.r1cs_load(r1cs), ctx.r1cs_load(other)
    wider = dict(r1cs); wider["nb_wires"] = r1cs["nb_wires"] + 1      # the same rows over one wire more
    rh_wider = ctx.r1cs_load(wider)
    try:
        old, _ = ctx.prove(pkh, W, a, b, None, r, s)
        for key, handle, wires, word in ((pkh, rh, W[:-1], "n_wires"), (pkh, rh_other, W, "r1cs"), (pk_other, rh, W, "proving key"),
                                         (pkh, rh_wider, W, "r1cs")):
            with pytest.raises(B.MiError) as ei:
                ctx.prove_w(key, handle, wires, r, s)
            assert "rc=-1:" in str(ei.value) and word in str(ei.value), str(ei.value)
        # a key over the same wires whose domain is another: the same rows followed by 300 empty ones
        padded = dict(r1cs); padded["n_constraints"] = 600
        for m in "ABC":
            rp, col, cf = r1cs[m]
            padded[m] = (np.concatenate([rp, np.full(300, rp[-1], np.uint64)]), col, cf)
        pk_padded, _, _ = ctx.setup(padded, td)
        try:
            with pytest.raises(B.MiError) as ei:
                ctx.prove_w(pk_padded, rh, W, r, s)
            assert "log_n" in str(ei.value)
        finally:
            ctx.pk_free(pk_padded)
        with pytest.raises(B.MiError):
            ctx.prove_w(pkh, rh, W, r, s, flags=2)
        # nothing is left queued: the same context still proves, both ways
        assert _same(ctx.prove_w(pkh, rh, W, r, s)[0], old) and _same(ctx.prove(pkh, W, a, b, None, r, s)[0], old)
    finally:
        for x in (rh, rh_other, rh_wider):
            ctx.r1cs_free(x)
        ctx.pk_free(pkh); ctx.pk_free(pk_other)


# ---------------------------------------------------------------------------------------------------- 5: lifetime
def test_r1cs_bytes_ledger_and_trim(ctx):
    n = (1 << 14) - 5
    r1cs = RC.skewed_r1cs(n, nb_wires=(1 << 14) + 9, nb_public=5, seed=14)
    W = RC.witness(r1cs["nb_wires"], 15)
    ctx_part = lambda m: {k: v for k, v in m.items() if k.startswith("ctx_")}
    ctx.trim()
    base = ctx.mem_ledger()
    want = RC.eval_all(r1cs, W)
    for _ in range(2):
        rh = ctx.r1cs_load(r1cs)
        held = ctx.r1cs_bytes(rh)
        formula = RC.r1cs_bytes(r1cs)
        assert formula <= held <= formula + 13 * 64, (held, formula)     # an empty array still holds one 64-byte allocation
        assert {k: v for k, v in ctx.mem_ledger().items() if k.startswith("key_")} == {k: v for k, v in base.items() if k.startswith("key_")}
        for have, ref in zip(ctx.r1cs_eval(rh, W, n), want):
            assert np.array_equal(have, ref)
        ctx.r1cs_check(rh, W)
        assert ctx_part(ctx.mem_ledger())["ctx_other"] > ctx_part(base)["ctx_other"]      # the evaluation's workspaces are the context's
        ctx.r1cs_free(rh)
    ctx.trim()
    assert ctx_part(ctx.mem_ledger()) == ctx_part(base)

"""GPU: whole proofs checked in the exponent, on proving keys whose every point is a known multiple of the generator (tests/dlog_keys.py).

Every other full-proof test compares the HIP prover with the oracle (oracle/groth16_ref.c), and both follow the same conventions.  Here
Ar, Bs and Krs must equal g^ar, g2^bs, g^krs with (ar, bs, krs) computed from the Groth16 formulas in Fr alone, on keys shaped like a real
gnark key: runs of equal and of opposite points (the doubling and cancellation branches of the 29-bit level-1 additions, reached through
mi_pk_load's window tables), unused private wires whose K is the point at infinity, committed twins, witness values at the signed-digit
edges of the production window widths, and the census's infinity masks (tools/wire_census.py census_masks_permille) and witness mix.
"""
import os
import sys
import time
import pytest
import cref
import dlog_keys as D
from gpu_common import load_binding

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import wire_census  # noqa: E402

pytestmark = pytest.mark.gpu
CENSUS_MASKS = wire_census.census_masks_permille()


@pytest.fixture(scope="module")
def ctx():
    B = load_binding()
    c = B.Context(0)
    yield c
    c.close()


def _census_dist():
    return load_binding().dist_mix(*wire_census.census_mix_permille())


def _inputs(log_n, nb_public, masks, dist, seed, nb_wires=None, n_constraints=None):
    N = 1 << log_n
    t0 = time.perf_counter()
    e = D.make_exps(log_n, nb_wires or N - 1000, nb_public, N >> 5, masks, True, seed)
    W = D.witness(e, dist, seed + 10)
    a, b, c = D.constraint_values(n_constraints or N - 100, dist, seed + 20)
    r, s = cref.gen_scalars(2, seed + 30, 0)
    want = D.expected_proof_exps(e, W, a, b, r, s)
    print(f"exponent reference at N=2^{log_n}: {time.perf_counter() - t0:.1f} s on {cref.num_threads()} threads")
    return dict(e=e, W=W, a=a, b=b, c=c, r=r, s=s, want=want)


@pytest.fixture(scope="module")
def case16(ctx):
    x = _inputs(16, 257, (900, 500), 1, 1616)
    x["pk"] = D.points_from_exps(x["e"], ctx)
    x["oracle"] = cref.proof_write(cref.prove(x["pk"], x["W"], x["a"], x["b"], x["c"], x["r"], x["s"])["raw"])
    return x


@pytest.mark.parametrize("knob", [(0, 0, 0), (17, 18, 17), (1, 1, 1)], ids=["auto", "tables-17-18-17", "generic"])
@pytest.mark.parametrize("limb29", [1, 2, 0])
def test_prove_2p16_dlog_keys(ctx, case16, limb29, knob):
    """N = 2^16, all plants: every 29-bit level-1 mode crossed with no tables, forced window tables and the generic sort; exponent check
    and the oracle's bytes"""
    B = load_binding()
    x = case16
    assert ctx.lib.mi_debug_set_msm_limb29(ctx.h, limb29) == 0
    assert ctx.lib.mi_debug_set_prove_fixed_base(ctx.h, *knob) == 0
    try:
        pkh = ctx.pk_load(x["pk"])
    finally:
        assert ctx.lib.mi_debug_set_prove_fixed_base(ctx.h, 0, 0, 0) == 0
    try:
        got, _ = ctx.prove(pkh, x["W"], x["a"], x["b"], x["c"], x["r"], x["s"])
    finally:
        ctx.pk_free(pkh)
        assert ctx.lib.mi_debug_set_msm_limb29(ctx.h, 1) == 0
    D.check_proof(got, x["want"])
    assert B.proof_write(got["raw"]) == x["oracle"]


@pytest.fixture(scope="module")
def case20(ctx):
    x = _inputs(20, 4097, CENSUS_MASKS, _census_dist(), 2020)
    pk, bufs = D.points_from_exps(x["e"], ctx, device=True)
    x["pk_dev"], x["bufs"] = pk, bufs
    yield x
    for d in bufs:
        d.free()


@pytest.mark.parametrize("knob", [(0, 0, 0), (1, 1, 1)], ids=["production", "generic"])
def test_prove_2p20_census_dlog_keys(ctx, case20, knob):
    """N = 2^20, census masks and witness mix, all plants, device-built key: the default plan (tables where they pay, the dense-sort rule)
    and the generic plan; exponent check, and the oracle's bytes on the production plan"""
    B = load_binding()
    x = case20
    assert ctx.lib.mi_debug_set_prove_fixed_base(ctx.h, *knob) == 0
    try:
        pkh = ctx.pk_load(x["pk_dev"], device_points=True)
    finally:
        assert ctx.lib.mi_debug_set_prove_fixed_base(ctx.h, 0, 0, 0) == 0
    print(f"N=2^20 census masks {CENSUS_MASKS}, knob {knob}: pk_table_plan (c_ak, c_b, c_z) = {ctx.pk_table_plan(pkh)}")
    try:
        got, _ = ctx.prove(pkh, x["W"], x["a"], x["b"], None, x["r"], x["s"])
    finally:
        ctx.pk_free(pkh)
    D.check_proof(got, x["want"])
    if knob == (0, 0, 0):
        host = {k: v for k, v in x["pk_dev"].items()}
        for name, d in zip(("g1_a", "g1_b", "g1_k", "g1_z", "g2_b"), x["bufs"]):
            host[name] = d.download((x["pk_dev"][name][1], 16 if name == "g2_b" else 8))
        want = cref.proof_write(cref.prove(host, x["W"], x["a"], x["b"], x["c"], x["r"], x["s"])["raw"])
        assert B.proof_write(got["raw"]) == want


def test_prove_2p20_census_dlog_keys_through_the_pool(ctx, case20):
    """the same key through the prover pool: host buffers, c formed on the device"""
    B = load_binding()
    x = case20
    pool = B.Prover(0, 2)
    try:
        c0 = pool.ctx(0)
        pkh = c0.pk_load(x["pk_dev"], device_points=True)
        try:
            got, _ = pool.wait(pool.submit(pkh, x["W"], x["a"], x["b"], None, x["r"], x["s"]))
        finally:
            c0.pk_free(pkh)
    finally:
        pool.close()
    D.check_proof(got, x["want"])


def test_prove_2p23_census_dlog_keys(ctx, case20):
    """BASELINE configs[1] shape (N = 2^23, nbPublic 4097, N / 32 committed wires), census masks and witness mix, all plants; production
    plan on a device-resident, device-built key; exponent check (no oracle prove at this size)"""
    for d in case20["bufs"]:
        d.free()
    case20["bufs"] = []
    ctx.trim()   # what the earlier tests grew goes back first (mi_ctx_trim), as the full-size tests do
    N = 1 << 23
    x = _inputs(23, 4097, CENSUS_MASKS, _census_dist(), 2323, nb_wires=N - 1000, n_constraints=N - 100)
    t0 = time.perf_counter()
    pk, bufs = D.points_from_exps(x["e"], ctx, device=True)
    try:
        pkh = ctx.pk_load(pk, device_points=True)
        print(f"N=2^23 key from exponents: {time.perf_counter() - t0:.1f} s; census masks {CENSUS_MASKS}: "
              f"|A| = {pk['g1_a'][1]}, |B| = {pk['g1_b'][1]}, |K| = {pk['g1_k'][1]}; pk_table_plan (c_ak, c_b, c_z) = {ctx.pk_table_plan(pkh)}")
        try:
            got, _ = ctx.prove(pkh, x["W"], x["a"], x["b"], None, x["r"], x["s"])
        finally:
            ctx.pk_free(pkh)
    finally:
        for d in bufs:
            d.free()
    D.check_proof(got, x["want"])

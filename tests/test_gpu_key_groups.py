"""GPU suite: what a loaded proving key holds, per group of MSMs that share a sort (A+K, B1+B2, Z), against closed forms.

The table plan and the three key_* byte counts of mi_get_mem_ledger are computed here from the masks, the fixed-base knobs, who owns
the point arrays and whether the 29-bit level-1 kernels are on -- never from what the library reports -- and compared as integers;
every key then proves to the oracle's bytes.  Arrays of the caller (mi_pk_load_dev) come back bit for bit after load, prove and free.
The load's failure exits are walked with mi_debug_inject_hip_failure (a checked HIP call returns an error code; nothing faults)."""
import ctypes as C
import numpy as np
import pytest
import cref
from helpers import *
from gpu_common import load_binding

pytestmark = pytest.mark.gpu

LOG_N = 12
N = 1 << LOG_N
KNOBS = ((0, 0, 0), (1, 1, 1), (17, 18, 17), (17, 1, 20))
ARRAYS = ("g1_a", "g1_b", "g1_k", "g1_z", "g2_b")
G1, G2 = 64, 128


@pytest.fixture(scope="module")
def case():
    """one key with infinity masks, public and committed wires, one witness and the oracle's proof bytes: shared, never written"""
    pk = synthetic_pk(LOG_N, N - 50, 300, 6161, n_committed=9)
    W = cref.gen_scalars(N - 50, 1, 1); a = cref.gen_scalars(N - 10, 2, 1); b = cref.gen_scalars(N - 10, 3, 0); c = cref.field_op(0, 2, a, b)
    r, s = cref.gen_scalars(2, 4, 0)
    want = cref.proof_write(cref.prove(pk, W, a, b, c, r, s)["raw"])
    return pk, (W, a, b, c, r, s), want


@pytest.fixture()
def ctx():
    B = load_binding()
    c = B.Context(0)
    yield c
    c.lib.mi_debug_inject_hip_failure(0)
    c.close()


def msm_nwin(c):
    return -(-256 // c)


def plan_of(knob, sizes):
    """the fixed-base rule at sizes below 2^20: nothing automatic; 1 = never; 17..22 = that width"""
    assert all(n < (1 << 20) for n in sizes)
    return tuple(k if 17 <= k <= 22 else 0 for k in knob)


def ledger_of(pk, plan, caller_owned, limb29):
    """key_bases, key_tables, key_indices of the loaded key in bytes"""
    nw = pk["nb_wires"]
    na, nb = int((pk["infinity_a"] == 0).sum()), int((pk["infinity_b"] == 0).sum())
    nk = pk["g1_k"].shape[0]
    n_z, n_z_msm = pk["g1_z"].shape[0], N - 1
    c_ak, c_b, c_z = plan
    tables = (2 * msm_nwin(c_ak) * nw * G1 if c_ak else 0) + (msm_nwin(c_b) * nb * (G1 + G2) if c_b else 0) + (msm_nwin(c_z) * n_z_msm * G1 if c_z else 0)
    bases = 0 if c_ak else 2 * nw * G1                         # A and K, one slot per wire: the key's own in both cases
    if not caller_owned:                                       # the library's uploads: dropped where tables replace them
        bases += (0 if c_b else nb * (G1 + G2)) + (0 if c_z else n_z * G1)
    elif limb29:                                               # converted copies of the caller's B1 / B2 / Z where there are no tables
        bases += (0 if c_b else nb * (G1 + G2)) + (0 if c_z else n_z_msm * G1)
    return bases, tables, (na + nb + nk) * 4


def read_ledger(ctx, pkh):
    B = load_binding()
    m = B.MemLedger()
    assert ctx.lib.mi_get_mem_ledger(ctx.h, pkh, C.byref(m)) == 0
    return int(m.key_bases), int(m.key_tables), int(m.key_indices)


def to_device(ctx, pk):
    bufs = {n: ctx.to_dev(pk[n]) for n in ARRAYS}
    d = dict(pk)
    for n in ARRAYS:
        d[n] = (bufs[n].ptr, pk[n].shape[0])
    return d, bufs


@pytest.mark.parametrize("limb29", [1, 0])
@pytest.mark.parametrize("caller_owned", [False, True])
def test_ledger_plan_and_proof_per_knob(ctx, case, caller_owned, limb29):
    """items 1 and 2: plan and ledger exact, the oracle's proof bytes, the caller's arrays untouched, nothing left after the free"""
    B = load_binding()
    pk, (W, a, b, c, r, s), want = case
    assert ctx.lib.mi_debug_set_msm_limb29(ctx.h, limb29) == 0
    start = read_ledger(ctx, None)
    for knob in KNOBS:
        assert ctx.lib.mi_debug_set_prove_fixed_base(ctx.h, *knob) == 0
        desc, bufs = to_device(ctx, pk) if caller_owned else (pk, {})
        pkh = ctx.pk_load(desc, device_points=caller_owned)
        plan = plan_of(knob, (pk["nb_wires"], pk["g1_b"].shape[0], N - 1))
        got_plan, got_ledger = ctx.pk_table_plan(pkh), read_ledger(ctx, pkh)
        print(f"caller_owned={caller_owned} limb29={limb29} knob={knob}: plan {got_plan} ledger {got_ledger}")
        assert got_plan == plan, knob
        assert got_ledger == ledger_of(pk, plan, caller_owned, limb29), knob
        got, _ = ctx.prove(pkh, W, a, b, c, r, s)
        assert B.proof_write(got["raw"]) == want, knob
        ctx.pk_free(pkh)
        assert read_ledger(ctx, None) == start
        for n, buf in bufs.items():
            assert np.array_equal(buf.download(pk[n].shape), pk[n]), (knob, n)
            buf.free()


@pytest.fixture(scope="module")
def setup_case():
    """a Setup at the same size: the R1CS and trapdoor, and the key mi_groth16_setup must make of them -- host points from the device's
    exponents (tests/test_gpu_setup.py checks those against the definition) by the oracle's scalar multiplication -- with the oracle's proof"""
    import dlog_keys as D
    import setup_cases as S
    B = load_binding()
    r1cs = S.synth_r1cs(N - 3, nb_wires=N - 50, nb_public=17, seed=14, per_row=4, n_coeffs=1000, n_heavy=8, heavy_len=200, commitments=1, n_committed=40)
    td = S.synth_trapdoor(15, n_sigma=1)
    c = B.Context(0)
    try:
        pk = D.points_from_exps(S.dlog_exps(r1cs, td, c.setup_exponents(r1cs, td), LOG_N))
    finally:
        c.close()
    W = cref.gen_scalars(r1cs["nb_wires"], 3, 1); a, b, cc = D.constraint_values(r1cs["n_constraints"], 1, 4); r, s = cref.gen_scalars(2, 5, 0)
    return r1cs, td, pk, (W, a, b, cc, r, s), cref.proof_write(cref.prove(pk, W, a, b, cc, r, s)["raw"])


@pytest.mark.parametrize("limb29", [1, 0])
def test_setup_made_key_ledger_plan_and_proof_per_knob(ctx, setup_case, limb29):
    """item 1, the third way in: mi_groth16_setup hands its device arrays to the key (they are the key's own, as uploaded ones are)"""
    B = load_binding()
    r1cs, td, pk, (W, a, b, c, r, s), want = setup_case
    assert ctx.lib.mi_debug_set_msm_limb29(ctx.h, limb29) == 0
    start = read_ledger(ctx, None)
    for knob in KNOBS:
        assert ctx.lib.mi_debug_set_prove_fixed_base(ctx.h, *knob) == 0
        pkh, peds, _ = ctx.setup(r1cs, td)
        try:
            plan = plan_of(knob, (pk["nb_wires"], pk["g1_b"].shape[0], N - 1))
            got_plan, got_ledger = ctx.pk_table_plan(pkh), read_ledger(ctx, pkh)
            print(f"setup limb29={limb29} knob={knob}: plan {got_plan} ledger {got_ledger}")
            assert got_plan == plan, knob
            assert got_ledger == ledger_of(pk, plan, False, limb29), knob
            got, _ = ctx.prove(pkh, W, a, b, c, r, s)
            assert B.proof_write(got["raw"]) == want, knob
        finally:
            ctx.pk_free(pkh)
            for ped in peds:
                ctx.pedersen_pk_free(ped)
        assert read_ledger(ctx, None) == start


@pytest.mark.parametrize("caller_owned", [False, True])
def test_load_unwinds_on_every_failing_call(ctx, case, caller_owned):
    """item 3: the n-th checked HIP call of the load fails, n = 1, 2, ... until a load gets through: each failure raises with a message,
    and the same context then loads and proves to the oracle's bytes.  The n of the first success is printed: it counts the load's
    checked calls"""
    B = load_binding()
    pk, (W, a, b, c, r, s), want = case
    assert ctx.lib.mi_debug_set_prove_fixed_base(ctx.h, 17, 18, 17) == 0
    desc, bufs = to_device(ctx, pk) if caller_owned else (pk, {})
    first_ok = None
    for nth in range(1, 200):
        assert ctx.lib.mi_debug_inject_hip_failure(nth) == 0
        try:
            pkh = ctx.pk_load(desc, device_points=caller_owned)
        except B.MiError as e:
            pkh = None
            assert ctx.lib.mi_last_error(ctx.h), (nth, str(e))
        finally:
            ctx.lib.mi_debug_inject_hip_failure(0)
        if pkh is None:
            pkh = ctx.pk_load(desc, device_points=caller_owned)
        else:
            first_ok = nth
        got, _ = ctx.prove(pkh, W, a, b, c, r, s)
        assert B.proof_write(got["raw"]) == want, nth
        ctx.pk_free(pkh)
        if first_ok:
            break
    print(f"caller_owned={caller_owned}: the load first succeeds at n = {first_ok}")
    # whoever owns the points, the load checks at least the three index uploads (an allocation and a copy each) and the two
    # expansions (allocation, clearing, launch): 12 calls
    assert first_ok and first_ok > 12, first_ok
    for n, buf in bufs.items():
        assert np.array_equal(buf.download(pk[n].shape), pk[n]), n
        buf.free()

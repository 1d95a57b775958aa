"""GPU suite: the failure exits of the four ways a proving key reaches the device -- mi_groth16_setup, mi_phase2_seal, mi_pk_load_stream
and mi_pk_load_raw -- walked with mi_debug_inject_hip_failure (a checked HIP call returns an error code; nothing faults).

One key serves all four: a seeded R1CS of 8 constraints, 48 wires, 5 public, one commitment over 3 wires and one heavy column, under a
trapdoor with gamma = delta = 1, so that the phase-2 state of the same (tau, alpha, beta, sigma) holds the same key.  Per entry point the
call runs once without injection and its result is kept; then the n-th checked call fails for n = 1, 2, ...: every failing call returns
non-zero, leaves a message, a null key handle and the Pedersen outputs named below; the first call that gets through gives the kept
result, and so does one more call after it."""
import ctypes as C
import numpy as np
import pytest
import cref
import dlog_keys as D
import setup_cases as S
from helpers import fr_arr
from gpu_common import load_binding
from test_gpu_phase2 import make_srs, secrets, trapdoor

pytestmark = pytest.mark.gpu
RAW, COMPRESSED = 0, 1
NC, NW, NPUB, LOG_N = 8, 48, 5, 3
# range(1, BOUND) of each sweep: twice the first n at which the call gets through on the commit before the shared handover
# (setup 169, seal 30, load_stream 44, load_raw 38), so that a few more checked calls do not end a sweep early
BOUND = {"setup": 338, "seal": 60, "load_stream": 88, "load_raw": 76}


@pytest.fixture(scope="module")
def ctx():
    B = load_binding()
    c = B.Context(0)
    yield c
    c.lib.mi_debug_inject_hip_failure(0)
    c.close()


@pytest.fixture(scope="module")
def case(ctx):
    """the R1CS, trapdoor and SRS, and what no injected call may change: Setup's two streams in both encodings and its vk, the oracle's proof
    from the key of Setup's exponents, the commitment and the proof of knowledge of Setup's Pedersen key.  Shared, never written"""
    tau, alpha, beta, sigma = secrets(77, 1)
    r1cs = S.synth_r1cs(NC, nb_wires=NW, nb_public=NPUB, seed=81, per_row=4, n_coeffs=64, n_heavy=1, heavy_len=NC, n_empty_cols=6, commitments=1,
                        n_committed=3)
    td = trapdoor(tau, alpha, beta, 1, sigma)
    streams = {}
    for enc in (RAW, COMPRESSED):
        pk_s, vk_s, _, _, vk = ctx.setup_to_streams(r1cs, td, enc, build=False)
        streams[enc] = (pk_s, vk_s)
    pk = D.points_from_exps(S.dlog_exps(r1cs, td, ctx.setup_exponents(r1cs, td), LOG_N))
    W = cref.gen_scalars(NW, 3, 1)
    a, b, c = D.constraint_values(NC, 1, 4)
    r, s = cref.gen_scalars(2, 5, 0)
    want = cref.proof_write(cref.prove(pk, W, a, b, c, r, s)["raw"])
    vals = cref.gen_scalars(3, 9, 1)
    pkh, peds, vk0 = ctx.setup(r1cs, td)
    try:
        assert all(np.array_equal(vk0[k], vk[k]) for k in vk)
        cm = (ctx.pedersen_commit(peds[0], vals), ctx.pedersen_commit(peds[0], vals, knowledge=True))
    finally:
        ctx.pedersen_pk_free(peds[0]); ctx.pk_free(pkh)
    removed = np.array(sorted(int(x) for ws, cw in r1cs["commitments"] for x in list(ws) + [cw]), np.uint32)
    return {"r1cs": r1cs, "td": td, "srs": make_srs(ctx, NC, tau, alpha, beta), "sigma": [fr_arr([x])[0] for x in sigma], "streams": streams, "vk": vk,
            "prove": (W, a, b, c, r, s), "want": want, "vals": vals, "cm": cm, "removed": removed}


class Outs:
    """the outputs of one call: the key handle starts as a value no call leaves (it must be WRITTEN null), the Pedersen handles null"""
    def __init__(self, B):
        self.h = C.c_void_p(1)
        self.ped = (C.c_void_p * B.MAX_COMMITMENTS)()
        self.nped = C.c_uint32(99)
        self.vk_k = np.zeros((NPUB + 1, 8), np.uint64)
        self.vk = B.VkOut(); self.vk.k = self.vk_k.ctypes.data; self.vk.k_cap = NPUB + 1

    def vk_dict(self):
        d = {n: np.array(getattr(self.vk, n), dtype=np.uint64) for n in ("alpha1", "beta2", "gamma2", "delta2")}
        d["k"] = self.vk_k[:int(self.vk.n_k)].copy()
        return d


def check_key(ctx, case, o, with_vk):
    """the key and the Pedersen key a call handed out: the oracle's proof bytes, the kept commitment and proof of knowledge, the kept vk"""
    B = load_binding()
    W, a, b, c, r, s = case["prove"]
    ped = C.c_void_p(o.ped[0])
    try:
        got, _ = ctx.prove(o.h, W, a, b, c, r, s)
        assert B.proof_write(got["raw"]) == case["want"]
        assert np.array_equal(ctx.pedersen_commit(ped, case["vals"]), case["cm"][0])
        assert np.array_equal(ctx.pedersen_commit(ped, case["vals"], knowledge=True), case["cm"][1])
        if with_vk:
            got_vk = o.vk_dict()
            assert sorted(got_vk) == sorted(case["vk"]) and all(np.array_equal(got_vk[k], case["vk"][k]) for k in got_vk)
    finally:
        ctx.pedersen_pk_free(ped); ctx.pk_free(o.h)


def sweep(ctx, name, call, failed, succeeded):
    """call() -> (rc, Outs).  failed(nth, outs) after every failing call, succeeded(outs) after the first that gets through and after one
    more call without injection; returns the n of the first success"""
    first_ok = None
    for nth in range(1, BOUND[name]):
        assert ctx.lib.mi_debug_inject_hip_failure(nth) == 0
        try:
            rc, o = call()
        finally:
            ctx.lib.mi_debug_inject_hip_failure(0)
        if rc == 0:
            first_ok = nth
            succeeded(o)
            break
        assert ctx.lib.mi_last_error(ctx.h), (name, nth)
        assert o.h.value is None, (name, nth)
        failed(nth, o)
    print(f"{name}: the call first gets through at n = {first_ok}")
    assert first_ok, f"{name}: no call got through below n = {BOUND[name]}"
    rc, o = call()
    assert rc == 0, ctx.lib.mi_last_error(ctx.h)
    succeeded(o)
    return first_ok


def no_pedersen_key(nth, o):
    assert o.ped[0] is None, nth


def test_setup_unwinds_on_every_failing_call(ctx, case):
    B = load_binding()
    r1cs, td = case["r1cs"], case["td"]

    def call():
        o = Outs(B)
        d, keep = B._r1cs_desc(r1cs); t = B._trapdoor(td)
        return ctx.lib.mi_groth16_setup(ctx.h, C.byref(d), C.byref(t), C.byref(o.h), o.ped, C.byref(o.vk)), o

    def succeeded(o):
        check_key(ctx, case, o, with_vk=True)
        for enc in (RAW, COMPRESSED):
            assert ctx.setup_to_streams(r1cs, td, enc, build=False)[:2] == case["streams"][enc], enc

    # the Fr half alone checks its 22 allocations, the three matrices' uploads and the per-matrix events: far more than 50 calls
    assert sweep(ctx, "setup", call, no_pedersen_key, succeeded) > 50


def test_seal_unwinds_on_every_failing_call(ctx, case):
    B = load_binding()
    st = ctx.phase2_init(case["r1cs"], case["srs"], case["sigma"])
    try:
        for enc in (RAW, COMPRESSED):
            assert ctx.phase2_to_streams(st, enc) == case["streams"][enc], enc

        def call():
            o = Outs(B)
            return ctx.lib.mi_phase2_seal(ctx.h, st, C.byref(o.h), o.ped, C.byref(o.vk)), o

        def succeeded(o):
            check_key(ctx, case, o, with_vk=True)
            for enc in (RAW, COMPRESSED):
                assert ctx.phase2_to_streams(st, enc) == case["streams"][enc], enc

        # seven device copies with an allocation each, and the load's own calls (test_gpu_key_groups.py: more than 12)
        assert sweep(ctx, "seal", call, no_pedersen_key, succeeded) > 26
    finally:
        ctx.phase2_free(st)


def loader_call(ctx, case, fn, blob, with_flags):
    B = load_binding()
    buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
    cw = case["removed"]

    def call():
        o = Outs(B)
        args = [ctx.h, buf, C.c_size_t(len(blob))] + ([C.c_uint32(0)] if with_flags else [])
        return fn(*args, C.c_uint32(NPUB), C.c_void_p(cw.ctypes.data), C.c_size_t(cw.shape[0]), C.byref(o.h), o.ped, C.byref(o.nped)), o
    return call


def test_load_stream_unwinds_on_every_failing_call(ctx, case):
    call = loader_call(ctx, case, ctx.lib.mi_pk_load_stream, case["streams"][COMPRESSED][0], True)

    def failed(nth, o):   # a Pedersen key made before the failure is freed and its slot cleared; the count stays 0
        assert o.ped[0] is None and o.nped.value == 0, nth

    def succeeded(o):
        assert o.nped.value == 1
        check_key(ctx, case, o, with_vk=False)

    # nine sections with an allocation and a launch check each, and the load's own calls
    assert sweep(ctx, "load_stream", call, failed, succeeded) > 30


def test_load_raw_unwinds_on_every_failing_call(ctx, case):
    call = loader_call(ctx, case, ctx.lib.mi_pk_load_raw, case["streams"][RAW][0], False)
    kept = []

    def failed(nth, o):
        # The older entry point frees the key but KEEPS the Pedersen keys it has adopted and reports their count: after a failure the
        # caller owns n_ped_out of them.  With one commitment that is the last wait for the stream, after the one adoption.
        assert o.nped.value in (0, 1), nth
        if o.nped.value == 0:
            assert o.ped[0] is None, nth
            return
        kept.append(nth)
        ped = C.c_void_p(o.ped[0])
        try:
            assert np.array_equal(ctx.pedersen_commit(ped, case["vals"]), case["cm"][0]), nth
        finally:
            ctx.pedersen_pk_free(ped)

    def succeeded(o):
        assert o.nped.value == 1
        check_key(ctx, case, o, with_vk=False)

    first_ok = sweep(ctx, "load_raw", call, failed, succeeded)
    print(f"load_raw: failing calls that left a Pedersen key to the caller: n = {kept}")
    assert first_ok > 30
    assert kept == [first_ok - 1], kept

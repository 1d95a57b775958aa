"""GPU: one proof schedule for every way the inputs arrive (csrc/prove.hip prove_common).  The arrivals -- host pointers, device pointers,
W alone from host or device memory against a resident R1CS, the pool's gated upload, the pool over device buffers -- run the same
sequence and differ only in how W, a, b, c become resident.  Every comparison of proofs is exact, against the oracle's bytes.

A  the same bytes from every arrival, c given or derived, the wire MSMs' accumulations held or not; the statistics each arrival owes
B  the Z MSM's digit count rides in computeH's last launch exactly once per proof on every arrival (the hook is armed right before part 3)
C  every checked HIP call of every arrival, made to fail in turn, unwinds: an error code or the right proof, and the next proof is right

Shapes.  A and C: a pyref.ToyR1CS of 1000 rows (1009 wires, log_n = 10: ragged against the domain and every tile), so that A W, B W, C W of
the W-only arrivals ARE the a, b, c of the others.  This is not test_gpu_errors.py's 1000 wires and 1020 constraints: one circuit has to serve
all six arrivals, and a ToyR1CS has one wire per row plus its inputs; the key the oracle proves with is built apart from the device's Setup.
The encodings compared are 164 bytes, not 196: these circuits carry no BSB22 commitment.  B: 4100 rows (4109 wires, log_n = 13) with 17-bit tables forced, the smallest domain at
which test_gpu_knobs.py::test_z_digit_count_from_compute_h_equals_the_count_pass shows the hook arming."""
import time
import pytest
import pyref as P
import cref
import setup_cases as S
from helpers import fr_arr
from gpu_common import load_binding
from test_gpu_setup import _toy_setup_exps_only, _toy_key_from_exps

pytestmark = pytest.mark.gpu

SINGLE = ("prove", "prove_dev", "prove_w", "prove_w_dev")     # the arrivals of one context
HOST = ("prove", "prove_w", "pool_host")                      # the ones whose inputs cross the bus inside the call


class Case:
    """One satisfied toy circuit: its key by the definition (for the oracle), its R1CS, witness, solver vectors and the oracle's proof"""
    def __init__(self, nc, seed):
        cs = P.ToyR1CS(nc, 5, seed, 0.5); td = P.ToyTrapdoor(seed)
        pk, exps, _ = _toy_setup_exps_only(cs, td)
        w, a, b, c = cs.solve()
        rng = P.SplitMix64(seed + 1)
        self.r1cs, self.td = S.toy_r1cs(cs), S.toy_trapdoor(td)
        self.W, self.a, self.b, self.c = fr_arr(w), fr_arr(a), fr_arr(b), fr_arr(c)      # c = a o b = C W: given or derived, one proof
        self.r, self.s = fr_arr([rng.fr()])[0], fr_arr([rng.fr()])[0]
        self.log_n = pk["log_n"]
        self.want = cref.proof_write(cref.prove(_toy_key_from_exps(cs, td, pk, exps), self.W, self.a, self.b, self.c, self.r, self.s)["raw"])

    def load(self, ctx):
        """the key by the device's Setup, the resident R1CS and device copies of the inputs, all on ctx's device"""
        self.pkh, _, _ = ctx.setup(self.r1cs, self.td)
        self.rh = ctx.r1cs_load(self.r1cs)
        self.dev = [ctx.to_dev(x) for x in (self.W, self.a, self.b, self.c)]

    def free(self, ctx):
        for d in self.dev:
            d.free()
        ctx.r1cs_free(self.rh); ctx.pk_free(self.pkh)

    def run(self, B, arrival, ctx, pool, derive_c):
        """one proof through `arrival` -> (the encoding of the proof: 164 bytes, these circuits have no commitment; stats)"""
        g = self
        dW, da, db, dc = (d.ptr for d in g.dev)
        nw, nc = len(g.W), len(g.a)
        flags = 0 if derive_c else B.PROVE_W_EVAL_C
        if arrival == "prove":
            p, st = ctx.prove(g.pkh, g.W, g.a, g.b, None if derive_c else g.c, g.r, g.s)
        elif arrival == "prove_dev":
            p, st = ctx.prove(g.pkh, dW, da, db, None if derive_c else dc, g.r, g.s, device=True, n_wires=nw, n_constraints=nc)
        elif arrival == "prove_w":
            p, st = ctx.prove_w(g.pkh, g.rh, g.W, g.r, g.s, flags=flags)
        elif arrival == "prove_w_dev":
            p, st = ctx.prove_w(g.pkh, g.rh, dW, g.r, g.s, flags=flags, device=True, n_wires=nw)
        elif arrival == "pool_host":     # an idle pool of one hands the job over while a, b, c are still arriving: the gated arrival
            p, st = pool.wait(pool.submit(g.pkh, g.W, g.a, g.b, None if derive_c else g.c, g.r, g.s))
        else:
            assert arrival == "pool_dev"
            p, st = pool.wait(pool.submit(g.pkh, dW, da, db, None if derive_c else dc, g.r, g.s, device=True, n_wires=nw, n_constraints=nc))
        return B.proof_write(p["raw"]), st


@pytest.fixture(scope="module")
def ctx():
    c = load_binding().Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small(ctx):
    g = Case(1000, 1003)
    assert g.log_n == 10 and len(g.W) == 1009
    g.load(ctx)
    yield g
    g.free(ctx)


# ---------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("hold", [0, 1])
@pytest.mark.parametrize("derive_c", [False, True])
def test_every_arrival_gives_the_oracles_bytes(ctx, small, derive_c, hold):
    B = load_binding()
    pool = B.Prover(0, 1)
    try:
        ctx.set_knob("hold_accum", hold); pool.set_knob("hold_accum", hold)
        for arrival in SINGLE + ("pool_host", "pool_dev"):
            got, st = small.run(B, arrival, ctx, pool, derive_c)
            print(f"{arrival} derive_c={derive_c} hold={hold}: compute_h_ms={st['compute_h_ms']:.3f} h2d_ms={st['h2d_ms']:.3f}")
            assert got == small.want, arrival
            assert st["compute_h_ms"] > 0, arrival
            assert (st["h2d_ms"] > 0) == (arrival in HOST), (arrival, st["h2d_ms"])
    finally:
        ctx.set_knob("hold_accum", 0)
        pool.close()


# ---------------------------------------------------------------------------------------------------- B
def test_z_count_hook_fires_once_per_proof_on_every_arrival(ctx):
    B = load_binding()
    assert ctx.lib.mi_debug_set_prove_fixed_base(ctx.h, 17, 17, 17) == 0      # read when a key is loaded
    g = None
    try:
        g = Case(4100, 4103)
        assert g.log_n == 13
        g.load(ctx)
        for fused in (1, 0, 1):
            ctx.set_knob("z_count_fused", fused)
            for arrival in SINGLE:
                for derive_c in (False, True):
                    before = ctx.counter("z_count_fused_launches")
                    got, _ = g.run(B, arrival, ctx, None, derive_c)
                    assert got == g.want, (arrival, derive_c, fused)
                    assert ctx.counter("z_count_fused_launches") == before + fused, (arrival, derive_c, fused)
    finally:
        ctx.set_knob("z_count_fused", 1)
        assert ctx.lib.mi_debug_set_prove_fixed_base(ctx.h, 0, 0, 0) == 0
        if g is not None and hasattr(g, "dev"):
            g.free(ctx)


# ---------------------------------------------------------------------------------------------------- C
@pytest.mark.parametrize("arrival", SINGLE)
def test_every_failure_point_of_every_arrival_unwinds(ctx, small, arrival):
    """mi_debug_inject_hip_failure(n) for n = 1, 2, 3, ...: the armed proof is refused or right, and the proof after it is right.  The sweep
    ends at the first n the proof does not reach (it succeeds and the countdown is still running): before n = 2000, after at least 20
    refusals.  hold_accum = 1 on the device arrival: the helpers wait for computeH's promise there, and every failure must release them."""
    B = load_binding()
    ctx.set_knob("hold_accum", 1 if arrival == "prove_dev" else 0)
    refused, n, t0 = 0, 0, time.perf_counter()
    try:
        assert small.run(B, arrival, ctx, None, False)[0] == small.want      # warm: every workspace has its size
        for n in range(1, 2000):
            assert ctx.lib.mi_debug_inject_hip_failure(n) == 0
            try:
                try:
                    got = small.run(B, arrival, ctx, None, False)[0]
                except B.MiError:
                    got = None
                left = ctx.counter("hip_failure_countdown")
            finally:
                ctx.lib.mi_debug_inject_hip_failure(0)
            ctx.sync()
            assert got is None or got == small.want, (arrival, n)
            assert small.run(B, arrival, ctx, None, False)[0] == small.want, (arrival, n)
            if got is None:
                refused += 1
            elif left > 0:
                break
        else:
            pytest.fail(f"{arrival}: a proof still reached its 1999th checked call")
    finally:
        ctx.lib.mi_debug_inject_hip_failure(0)
        ctx.set_knob("hold_accum", 0)
    print(f"{arrival}: {n - 1} checked calls in a proof, {refused} refused, {time.perf_counter() - t0:.1f} s")
    assert refused >= 20, (arrival, refused)

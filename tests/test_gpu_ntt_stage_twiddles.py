"""GPU: computeH with its stage twiddles taken by global index (knob "ntt_stage_twiddles" = 1, the default: NttPass::tw_stage, no
inter-pass product) and with today's tile-local twiddles plus the product at every strided pass's edge (= 0), on one context, against the
oracle's h.  The field is exact: every coefficient is compared for equality.  Sizes: 2^14 (one strided pass of radix 2^5, every stage
through LDS), 2^16 (radix 2^7, M = N), 2^17 under the plan (9, 9, 8) (radix 2^8: k_ntt_strided_triple8 and one LDS stage per pass;
the default plan has the strided radices 2^4 2^4 there) and 2^21 under the plan (9, 7, 7) (two strided passes of radix 2^7: the
benchmark's shape at a sixteenth of its size)."""
import ctypes as C
import numpy as np
import pytest
import cref
from gpu_common import load_binding

pytestmark = pytest.mark.gpu

KNOB = "ntt_stage_twiddles"
SIZES = [(14, None), (16, None), (17, (9, 9, 8)), (21, (9, 7, 7))]
DEFAULT_PLAN = (9, 9, 7)


@pytest.fixture(scope="module")
def ctx():
    c = load_binding().Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def inputs():
    """log_n -> a, b, c of N - 100 rows (c unrelated to a o b); one size kept"""
    kept = {}
    def get(log_n):
        if log_n not in kept:
            kept.clear()
            kept[log_n] = tuple(cref.gen_scalars((1 << log_n) - 100, 4100 + 3 * log_n + k, int(k == 0)) for k in range(3))
        return kept[log_n]
    return get


def _ntt_table_bytes(ctx):
    m = load_binding().MemLedger()
    assert ctx.lib.mi_get_mem_ledger(ctx.h, None, C.byref(m)) == 0
    return int(m.ctx_ntt_tables)


def _h(ctx, log_n, a, b, c):
    """mi_compute_h_dev on device copies of the rows given (c None: formed on the device)"""
    bufs = [ctx.to_dev(x) for x in ((a, b) if c is None else (a, b, c))] + [ctx.alloc(32 << log_n)]
    try:
        ctx.compute_h_dev(log_n, bufs[0].ptr, bufs[1].ptr, None if c is None else bufs[2].ptr, a.shape[0], bufs[-1].ptr)
        return bufs[-1].download((1 << log_n, 4))
    finally:
        for d in bufs:
            d.free()


@pytest.mark.parametrize("nc_of", [lambda n: n - 100, lambda n: 1], ids=["N-100", "1"])
@pytest.mark.parametrize("log_n,plan", SIZES)
def test_compute_h_with_stage_twiddles_and_without_matches_oracle(ctx, inputs, log_n, plan, nc_of):
    nc = nc_of(1 << log_n)
    a, b, c = (v[:nc] for v in inputs(log_n))
    want = {True: cref.compute_h(log_n, a, b, c), False: cref.compute_h(log_n, a, b, cref.field_op(0, 2, a, b))}
    try:
        if plan:
            assert ctx.lib.mi_debug_set_ntt_plan(ctx.h, *plan) == 0
        for knob in (1, 0):
            ctx.set_knob(KNOB, knob)
            for given in (True, False):
                got = _h(ctx, log_n, a, b, c if given else None)
                assert np.array_equal(got, want[given]), (log_n, nc, knob, given, int((got != want[given]).any(axis=1).sum()))
    finally:
        ctx.set_knob(KNOB, 1)
        if plan:
            assert ctx.lib.mi_debug_set_ntt_plan(ctx.h, *DEFAULT_PLAN) == 0


def test_tables_follow_the_knob(ctx):
    """1 -> 0 -> 1 on one context at 2^14 under the plan (5, 4, 5) (strided radices 2^5 2^5): the next computeH rebuilds its tables.  With
    the knob on, the M = N stage table takes the direct twiddle table's place byte for byte and the inner pass's table (2^9 entries per
    root) is the whole difference; h is the oracle's every time"""
    log_n, nc = 14, (1 << 14) - 9
    a, b, c = (cref.gen_scalars(nc, 5200 + k, int(k == 1)) for k in range(3))
    want = cref.compute_h(log_n, a, b, c)
    inner = 2 * 32 * (1 << 9)
    try:
        assert ctx.lib.mi_debug_set_ntt_plan(ctx.h, 5, 4, 5) == 0
        seen = []
        for knob in (1, 0, 1):
            ctx.set_knob(KNOB, knob)
            assert np.array_equal(_h(ctx, log_n, a, b, c), want), knob
            seen.append(_ntt_table_bytes(ctx))
        assert seen[0] == seen[2] == seen[1] + inner, seen
        with pytest.raises(Exception):
            ctx.set_knob(KNOB, 2)
    finally:
        ctx.set_knob(KNOB, 1)
        assert ctx.lib.mi_debug_set_ntt_plan(ctx.h, *DEFAULT_PLAN) == 0


def test_ntt_ledger_does_not_grow(ctx, inputs):
    """mem_ledger()'s NTT figure with the knob at 1 is not above its figure at 0 by more than 1 %: at 2^21 under (9, 7, 7) the inner
    pass's two 2^14-entry tables (1 MiB) on top of four N-entry tables either way; at 2^16 (one strided pass) nothing at all"""
    try:
        for log_n, plan in ((21, (9, 7, 7)), (16, None)):
            a, b, _ = inputs(log_n)
            if plan:
                assert ctx.lib.mi_debug_set_ntt_plan(ctx.h, *plan) == 0
            fig = {}
            for knob in (0, 1):
                ctx.set_knob(KNOB, knob)
                _h(ctx, log_n, a[:1000], b[:1000], None)
                fig[knob] = ctx.mem_ledger()["ctx_ntt_tables"]
            print(f"ctx_ntt_tables at 2^{log_n}: knob 0 {fig[0]:.6f} GB, knob 1 {fig[1]:.6f} GB")
            assert 0 < fig[1] <= 1.01 * fig[0], (log_n, fig)
            if plan:
                assert ctx.lib.mi_debug_set_ntt_plan(ctx.h, *DEFAULT_PLAN) == 0
    finally:
        ctx.set_knob(KNOB, 1)
        assert ctx.lib.mi_debug_set_ntt_plan(ctx.h, *DEFAULT_PLAN) == 0

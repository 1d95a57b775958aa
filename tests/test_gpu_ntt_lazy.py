"""GPU: the lazy 8 x 32-bit arithmetic under every NTT stage at its contract edges.  (1) The device bodies of fe_add_nored / fe_sub_plus2p /
fe_condsub_2p / fe_canon / fe_mul_lazy and the butterflies built on them (inline-asm carry chains and selects), one record per lane through
mi_debug_lazy_op_dev, against Python integers and against the host build of the same code, word for word, on every case of
lazy_cases.py.  (2) Whole transforms and computeH on structured inputs -- exact zeros, constants, root powers, deltas, periodic vectors,
a b - c the zero polynomial -- where a representative is exactly 0, p or 2p and butterfly operands are equal, through the default plan, the
turned-down plans, the register / LDS stage paths and every combination of computeH's fused launches, against the oracle (whose
arithmetic is fully reduced) and the closed forms.  Every comparison is exact: a true zero comes back as eight zero limbs."""
import ctypes as C
import numpy as np
import pytest
import cref
import closed_forms as cf
import lazy_cases as LZ
from gpu_common import load_binding

pytestmark = pytest.mark.gpu

SMALL_PLANS = {10: (6, 3, 3), 13: (7, 5, 4), 14: (8, 8, 2)}            # test_ntt_small_tiles_multi_pass
WAVE_SETTINGS = ((1, 7), (0, 29), (1, 29), (0, 7))                      # test_ntt_register_and_lds_stage_paths_agree_with_oracle
NTT_PATHS = [(n, "default") for n in LZ.NTT_LOG_NS] + [(n, "small_plan") for n in SMALL_PLANS] + [(n, f"wave_{on}_{dmin}") for n in LZ.NTT_LOG_NS for on, dmin in WAVE_SETTINGS]
NTT_PATHS.sort(key=lambda t: t[0])                                      # one size after the other: the fixture keeps one size's oracle outputs
# test_compute_h_with_and_without_the_fused_launches without its 2^19 .. 2^21 entries, plus a three-pass plan at 2^16 (radices 2^7 2^7 2^2)
H_PLANS = [(10, None), (14, (8, 7, 7)), (16, None), (16, (10, 8, 8)), (16, (10, 2, 7)), (17, (10, 10, 7)), (17, (9, 9, 8))]


@pytest.fixture(scope="module")
def ctx():
    B = load_binding()
    c = B.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def emu_so(tmp_path_factory):
    return LZ.build_emu(str(tmp_path_factory.mktemp("emu") / "libemu_lazy.so"))


@pytest.fixture(scope="module")
def ntt_oracle():
    """log_n -> (cases, bit-reversal index, {(case index, flags): oracle output}); built once per size, one size kept"""
    kept = {}
    def get(log_n):
        if log_n not in kept:
            kept.clear()
            cases, rev = LZ.ntt_cases(log_n), LZ.bitrev_index(log_n)
            want = {(i, f): cref.ntt(c.physical(f, rev), log_n, f) for i, c in enumerate(cases) for f in range(8)}
            for (i, f), w in want.items():   # the closed forms hold for the oracle: they are statements about the inputs, checked once here
                assert not LZ.ntt_closed_form_errors(cases[i], w, log_n, f, rev), (cases[i].name, f)
            kept[log_n] = (cases, rev, want)
        return kept[log_n]
    return get


@pytest.fixture(scope="module")
def h_oracle():
    kept = {}
    def get(log_n):
        if log_n not in kept:
            kept.clear()
            cases = LZ.compute_h_cases(log_n)
            want = [cref.compute_h(log_n, c.a, c.b, c.c) for c in cases]
            for c, w in zip(cases, want):
                if c.zero_h:
                    assert not w.any(), c.name
                if c.poly:
                    assert not cf.compute_h_check(w, log_n, *c.poly), c.name
            kept[log_n] = (cases, want)
        return kept[log_n]
    return get


# ---------------------------------------------------------------------------------------------------- primitives
def test_lazy_op_rejects_bad_arguments(ctx):
    lib, h = ctx.lib, ctx.h
    buf = ctx.alloc(256)
    try:
        for op in (-1, LZ.OP_END, 1000):
            assert lib.mi_debug_lazy_op_dev(h, C.c_int(op), C.c_void_p(buf.ptr), C.c_void_p(buf.ptr), C.c_size_t(1)) != 0, op
        assert lib.mi_debug_lazy_op_dev(h, C.c_int(0), None, C.c_void_p(buf.ptr), C.c_size_t(1)) != 0
        assert lib.mi_debug_lazy_op_dev(h, C.c_int(0), C.c_void_p(buf.ptr), None, C.c_size_t(1)) != 0
        assert lib.mi_debug_lazy_op_dev(h, C.c_int(0), C.c_void_p(buf.ptr), C.c_void_p(buf.ptr), C.c_size_t((1 << 30) + 1)) != 0
        assert lib.mi_debug_lazy_op_dev(h, C.c_int(0), None, None, C.c_size_t(0)) == 0
    finally:
        buf.free()


@pytest.mark.parametrize("op", range(LZ.OP_END), ids=LZ.OP_NAMES)
def test_device_lazy_ops_equal_the_integer_reference_and_the_host_build(ctx, emu_so, op):
    cs, rin, want = LZ.records(op)
    dev = ctx.lazy_op(op, rin)
    bad = np.nonzero((dev != want).any(axis=1))[0]
    assert not len(bad), ("device differs from the integer reference", len(bad), LZ.describe(op, cs, bad[:5]))
    assert np.array_equal(dev, want)
    host, err = LZ.run_emu(emu_so, op, rin)
    assert err is None, (err[1], LZ.describe(op, cs, [err[0]]))
    assert np.array_equal(dev, host), ("device differs from the host build", LZ.describe(op, cs, np.nonzero((dev != host).any(axis=1))[0][:5]))


# ---------------------------------------------------------------------------------------------------- whole transforms
@pytest.mark.parametrize("log_n,path", NTT_PATHS, ids=[f"2p{n}-{p}" for n, p in NTT_PATHS])
def test_ntt_structured_inputs(ctx, ntt_oracle, log_n, path):
    cases, rev, want = ntt_oracle(log_n)
    lib = ctx.lib
    try:
        if path == "small_plan":
            assert lib.mi_debug_set_ntt_plan(ctx.h, *SMALL_PLANS[log_n]) == 0
        elif path.startswith("wave_"):
            on, dmin = (int(v) for v in path.split("_")[1:])
            assert lib.mi_debug_set_ntt_wave_stages(ctx.h, on, dmin) == 0
        for i, case in enumerate(cases):
            for flags in range(8):
                got = ctx.ntt(case.physical(flags, rev), log_n, flags)
                assert np.array_equal(got, want[(i, flags)]), (case.name, flags, path)
    finally:
        if path.startswith("wave_"):
            assert lib.mi_debug_set_ntt_wave_stages(ctx.h, 1, 12) == 0
        if path == "small_plan":
            assert lib.mi_debug_set_ntt_plan(ctx.h, 9, 9, 7) == 0


def _check_h(ctx, log_n, cases, want, tag):
    for case, w in zip(cases, want):
        got = ctx.compute_h(log_n, case.a, case.b, case.c)
        assert np.array_equal(got, w), (case.name, tag)
        if case.derive:   # c = NULL: formed on the device as a o b
            assert np.array_equal(ctx.compute_h(log_n, case.a, case.b, None), w), (case.name, tag, "derived c")


@pytest.mark.parametrize("log_n,plan", H_PLANS, ids=[f"2p{n}-{'default' if p is None else 'x'.join(map(str, p))}" for n, p in H_PLANS])
def test_compute_h_structured_inputs_in_every_fused_combination(ctx, h_oracle, log_n, plan):
    cases, want = h_oracle(log_n)
    lib = ctx.lib
    try:
        if plan:
            assert lib.mi_debug_set_ntt_plan(ctx.h, *plan) == 0
        for mask in range(8):
            assert lib.mi_debug_set_ntt_fuse_pair(ctx.h, mask) == 0
            _check_h(ctx, log_n, cases, want, f"fuse mask {mask}")
    finally:
        assert lib.mi_debug_set_ntt_fuse_pair(ctx.h, 7) == 0
        if plan:
            assert lib.mi_debug_set_ntt_plan(ctx.h, 9, 9, 7) == 0


@pytest.mark.parametrize("log_n", [13, 16])
def test_compute_h_structured_inputs_on_register_and_lds_stage_paths(ctx, h_oracle, log_n):
    cases, want = h_oracle(log_n)
    try:
        for on, dmin in WAVE_SETTINGS:
            assert ctx.lib.mi_debug_set_ntt_wave_stages(ctx.h, on, dmin) == 0
            _check_h(ctx, log_n, cases, want, f"wave stages {on}, direct tables from 2^{dmin}")
    finally:
        assert ctx.lib.mi_debug_set_ntt_wave_stages(ctx.h, 1, 12) == 0

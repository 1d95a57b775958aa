"""GPU parity of the 29-bit-limb arithmetic (csrc/limb29_ops.cuh through mi_debug_limb29_op_dev): the device build, whose every multiply-
accumulate is an inline-asm v_mad_u64_u32, against the host build of the same code (overflow traps on) limb for limb, and against pyref --
the primitives at their documented edges, 2^16 random edge operands per product, and the group steps from adversarial accumulator states."""
import numpy as np
import pytest
import pyref as P
import limb29_cases as L29
from gpu_common import load_binding

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    B = load_binding()
    c = B.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def emu_so(tmp_path_factory):
    return L29.build_emu(str(tmp_path_factory.mktemp("emu") / "libemu_limb29.so"))


def _same(dev, host, names):
    bad = [names[i] for i in np.nonzero((dev != host).any(axis=1))[0][:10]]
    assert not bad, f"device limbs differ from the host build: {bad}"


def test_limb29_op_rejects_bad_arguments(ctx):
    lib, h = ctx.lib, ctx.h
    import ctypes as C
    buf = ctx.alloc(320)
    for op in (-1, 17, 19, 26, 1000):
        assert lib.mi_debug_limb29_op_dev(h, C.c_int(op), C.c_void_p(buf.ptr), C.c_void_p(buf.ptr), C.c_size_t(1)) != 0, op
    assert lib.mi_debug_limb29_op_dev(h, C.c_int(0), None, C.c_void_p(buf.ptr), C.c_size_t(1)) != 0
    assert lib.mi_debug_limb29_op_dev(h, C.c_int(0), C.c_void_p(buf.ptr), None, C.c_size_t(1)) != 0
    assert lib.mi_debug_limb29_op_dev(h, C.c_int(0), C.c_void_p(buf.ptr), C.c_void_p(buf.ptr), C.c_size_t((1 << 30) + 1)) != 0
    assert lib.mi_debug_limb29_op_dev(h, C.c_int(0), None, None, C.c_size_t(0)) == 0
    buf.free()


def test_limb29_device_primitives_at_their_edges_match_host(ctx, emu_so):
    for op, recs in L29.primitive_edge_records().items():
        host, err = L29.run_emu(emu_so, op, recs)
        assert err is None, err
        dev = ctx.limb29_op(op, recs)
        _same(dev, host, [f"op {op} record {i}" for i in range(len(recs))])
        if op in (L29.MUL, L29.SQR, L29.MUL2, L29.MUL4):
            for r, o in zip(recs, dev):
                assert L29.val([int(x) for x in o[:9]]) % P.Q_MOD == L29.product_value(op, [int(x) for x in r])[0], (op, r)


@pytest.mark.parametrize("op", [0, 8, 1, 9])   # f29_mul, f29_sqr, f29_mul2, f29_mul4
def test_limb29_device_products_on_random_edge_operands(ctx, emu_so, op):
    recs = L29.product_records(op, 1 << 16, 1000 + op)
    host, err = L29.run_emu(emu_so, op, recs)
    assert err is None, err
    dev = ctx.limb29_op(op, recs)
    _same(dev, host, [f"op {op} record {i}" for i in range(len(recs))])
    for r, o in zip(recs, dev):
        want, s_ = L29.product_value(op, [int(x) for x in r])
        v = L29.val([int(x) for x in o[:9]])
        assert v % P.Q_MOD == want and all(int(x) <= L29.M29 for x in o[:8]) and v < s_ // (1 << 261) + P.Q_MOD + 1, (op, r)


def test_limb29_device_group_steps_from_adversarial_states(ctx, emu_so):
    cases = L29.group_cases(seed=5, per_kind=4) + L29.group_cases(seed=6, per_kind=2)
    host = L29.run_group_cases(emu_so, cases)
    dev = np.zeros_like(host)
    for op in sorted({c[1] for c in cases}):
        idx = [i for i, c in enumerate(cases) if c[1] == op]
        dev[idx] = ctx.limb29_op(op, np.stack([cases[i][2] for i in idx]))
    _same(dev, host, [c[0] for c in cases])
    bad = L29.check_group_outputs(cases, dev)
    assert not bad, "\n".join(bad)

"""GPU: the field arithmetic on operands the compiler can see through.  Every other per-primitive test feeds the inline-asm bodies of
field.cuh / field29.cuh / mont_cols.inc values loaded from memory; a wrong asm constraint shows only where the register allocator knows
something about an operand -- a literal, a limb that is provably zero, one value in two positions, a result over its input (DESIGN.md 4d:
the "+v" accumulator of the generated Montgomery columns under fr_from_u128).  One kernel per shape of csrc/shape_ops.cuh through
mi_debug_field_shape_dev, against the integer reference of shape_cases.py and against the host build of the same bodies, word for word,
at n = 1, 65 and 130 records.  Everything is exact."""
import ctypes as C
import time
import numpy as np
import pytest
import shape_cases as SH
from gpu_common import load_binding

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    B = load_binding()
    t0 = time.perf_counter()
    c = B.Context(0)
    yield c
    c.close()
    print(f"\ntests/test_gpu_field_shapes.py: {time.perf_counter() - t0:.1f} s wall from its first test to its last")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """the host build, called in this process: tests/test_shape_cases_cpu.py has run the same records in a child process, where a trap
    names its record"""
    return C.CDLL(SH.build_emu(str(tmp_path_factory.mktemp("emu") / "libemu_shape.so")))


def test_field_shape_rejects_bad_arguments(ctx):
    lib, h = ctx.lib, ctx.h
    EINVAL = -1   # MI_EINVAL (include/mi355x_groth16.h)
    assert lib.mi_debug_field_shape_dev(h, C.c_int(-1), None, None, C.c_size_t(0)) == EINVAL
    buf = ctx.alloc(256)
    try:
        p = C.c_void_p(buf.ptr)
        for shape in (-1, SH.OP_END, 1000):
            assert lib.mi_debug_field_shape_dev(h, C.c_int(shape), p, p, C.c_size_t(1)) == EINVAL, shape
        assert lib.mi_debug_field_shape_dev(h, C.c_int(0), None, p, C.c_size_t(1)) == EINVAL
        assert lib.mi_debug_field_shape_dev(h, C.c_int(0), p, None, C.c_size_t(1)) == EINVAL
        assert lib.mi_debug_field_shape_dev(h, C.c_int(0), p, p, C.c_size_t((1 << 24) + 1)) == EINVAL
        assert lib.mi_debug_field_shape_dev(None, C.c_int(0), p, p, C.c_size_t(1)) == EINVAL
        assert lib.mi_debug_field_shape_dev(h, C.c_int(0), None, None, C.c_size_t(0)) == 0
        assert lib.mi_debug_field_shape_dev(h, C.c_int(SH.OP_END - 1), None, None, C.c_size_t(0)) == 0
    finally:
        buf.free()


@pytest.mark.parametrize("shape", range(SH.OP_END), ids=SH.NAMES)
def test_device_shapes_equal_the_integer_reference_and_the_host_build(ctx, emu, shape):
    rin, want = SH.records(shape)
    host = np.zeros_like(want)
    assert emu.emu_field_shape(C.c_int(shape), host.ctypes.data_as(C.c_void_p), rin.ctypes.data_as(C.c_void_p), C.c_size_t(len(rin))) == 0
    assert np.array_equal(host, want), "the host build differs from the integer reference"
    for n in (1, 65, SH.RECORDS):
        dev = ctx.field_shape(shape, rin[:n])
        bad = np.nonzero((dev != want[:n]).any(axis=1))[0]
        assert not len(bad), (f"device differs from the integer reference at n = {n}", len(bad), SH.describe(shape, rin, bad[:3]),
                              "got " + " ".join(f"{int(w):08x}" for w in dev[bad[0]]), "want " + " ".join(f"{int(w):08x}" for w in want[bad[0]]))
        assert np.array_equal(dev, want[:n]) and np.array_equal(dev, host[:n])

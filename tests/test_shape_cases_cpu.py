"""CPU suite: every operand shape of gnark-whir_amd/csrc/shape_ops.cuh (literal factors, limbs that are provably zero, one value in two
places, results over inputs, chains that start at a literal) in its host build, overflow traps on, against the integer reference of
shape_cases.py.  This proves the table and the references before a kernel runs, and the traps prove the inputs are within the contracts;
what the shapes are FOR -- the inline-asm bodies on operands the register allocator knows -- only the device run can show
(tests/test_gpu_field_shapes.py)."""
import ctypes as C
import numpy as np
import pytest
import pyref as P
import shape_cases as SH


@pytest.fixture(scope="module")
def emu_so(tmp_path_factory):
    return SH.build_emu(str(tmp_path_factory.mktemp("emu") / "libemu_shape.so"))


@pytest.fixture(scope="module")
def emu(emu_so):
    return C.CDLL(emu_so)


def test_the_table_and_the_enum_agree(emu):
    assert emu.emu_shape_generic_end() == SH.SHG_END and emu.emu_shape_op_end() == SH.OP_END == len(SH.NAMES)
    assert len(set(SH.NAMES)) == len(SH.NAMES)


def test_the_generator_checks_itself():
    """130 records per shape; the field operands hold the adversarial pairs, 0, 1, p - 1, p - 2, limbs of 0xFFFFFFFF in every kept word,
    and every value is below its modulus; a shape whose answer is fixed by definition has it in the reference"""
    for field, mod in ((0, P.R_MOD), (1, P.Q_MOD)):
        ops = SH.field_operands(mod, 77 + field)
        assert len(ops) == SH.RECORDS == 130
        xs = [o[0] for o in ops]
        assert {0, 1, mod - 1, mod - 2} <= set(xs) and all(0 <= t < mod for o in ops for t in o)
        ones = SH.all_ones_below(mod)
        assert ones in xs and all(w == 0xFFFFFFFF for w in SH.words_of(ones)[:7])
        assert sum(1 for x in xs if x & 0xFFFFFFFF == 0xFFFFFFFF) >= 30
        base = field * SH.SHG_END
        _, want = SH.records(base + SH.GENERIC.index("mul_sub_same"))
        assert not want[:, :8].any()                                                       # x y - x y
        _, want = SH.records(base + SH.GENERIC.index("sub_lit"))
        assert all(SH.words_val(r[24:32]) == mod and not r[8:24].any() for r in want)      # fe_neg_raw(0) = p; x - x = -0 = 0
        rin, want = SH.records(base + SH.GENERIC.index("mul2_lit"))
        assert np.array_equal(want[:, :8], want[:, 16:24])                                 # fe_mul2_add(x, y, 0, v) = x y
    for shape in range(SH.OP_END):
        rin, want = SH.records(shape)
        assert rin.shape == (130, 32) and want.shape == (130, 32) and want.any(), SH.NAMES[shape]


@pytest.mark.parametrize("shape", range(SH.OP_END), ids=SH.NAMES)
def test_host_shapes_equal_the_integer_reference(emu_so, shape):
    """emu_field_shape (the portable bodies, MI_CHECK_NOWRAP) word for word on every record, in a child process: a trap names its record"""
    rin, want = SH.records(shape)
    got, err = SH.run_emu(emu_so, shape, rin)
    assert err is None, (err[1], SH.describe(shape, rin, [err[0]]))
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert not len(bad), (len(bad), SH.describe(shape, rin, bad[:3]), [f"{int(w):08x}" for w in got[bad[0]]], [f"{int(w):08x}" for w in want[bad[0]]])
    assert np.array_equal(got, want)


def test_host_shape_refuses_an_unknown_shape(emu):
    buf = np.zeros(SH.IN_W, np.uint32); out = np.zeros(SH.OUT_W, np.uint32)
    for shape in (-1, SH.OP_END, 1000):
        assert emu.emu_field_shape(C.c_int(shape), out.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p), C.c_size_t(1)) != 0

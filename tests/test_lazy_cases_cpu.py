"""CPU suite: the NTT's lazy arithmetic (field.cuh fe_add_nored / fe_sub_plus2p / fe_condsub_2p / fe_canon / fe_mul_lazy, ntt_tile.cuh
butterflies) in its host build, overflow traps on, against Python integers on every record of lazy_cases.py, and the structured
whole-transform inputs (exact zeros, equal butterfly operands, spikes) through the trapping emulator against the oracle."""
import ctypes as C
import numpy as np
import pytest
import cref
import lazy_cases as LZ

PLANS = [(1, 11, 11, 8), (4, 11, 11, 8), (6, 3, 3, 2), (9, 5, 4, 3), (10, 6, 3, 3)]   # (log_n, log_e, max_contig, max_strided): 1- to 4-pass plans


@pytest.fixture(scope="module")
def emu_so(tmp_path_factory):
    return LZ.build_emu(str(tmp_path_factory.mktemp("emu") / "libemu_lazy.so"))


@pytest.fixture(scope="module")
def emu(emu_so):
    return C.CDLL(emu_so)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_reference_and_generator_check_themselves():
    """every op has its records, every record met its documented range (reference() asserts them), the coverage assertions of
    lazy_cases.records hold, and the edge list is what the contract edges are"""
    p = LZ.P_
    assert set([0, 1, p - 1, p, p + 1, 2 * p - 1, 2 * p, 2 * p + 1, 3 * p - 1, 3 * p, 4 * p - 1]) <= set(LZ.EDGE) and max(LZ.EDGE) == 4 * p - 1
    for k in range(4):
        band = [v for v in LZ.EDGE if k * p <= v < (k + 1) * p]
        assert any(v & 0xFFFFFFFF == 0xFFFFFFFF and (v >> 32) & 0xFFFFFFFF == 0xFFFFFFFF for v in band) and any(v & ((1 << 224) - 1) == 0 for v in band), k
        assert sum(1 for v in LZ.RANDOM if k * p <= v < (k + 1) * p) == LZ.RANDOM_PER_BAND
    assert all(w < p for w in LZ.TWIDDLES)
    for op in range(LZ.OP_END):
        cs, rin, want = LZ.records(op)
        assert 800 <= len(cs) == len(rin) == len(want), LZ.OP_NAMES[op]
    # the unreduced product really is unreduced: some records of mul_lazy land in [p, 2p), and x == 2p / x == p are met by condsub_2p and canon
    cs, _, want = LZ.records(LZ.MUL_LAZY)
    assert sum(1 for r in want if LZ.words_val(r[:8]) >= p) > 100
    assert (2 * p, 0, 0) in LZ.records(LZ.CONDSUB_2P)[0] and (p, 0, 0) in LZ.records(LZ.CANON)[0] and (3 * p, 0, 0) in LZ.records(LZ.CANON)[0]


@pytest.mark.parametrize("op", range(LZ.OP_END), ids=LZ.OP_NAMES)
def test_host_lazy_ops_equal_the_integer_reference(emu_so, op):
    """emu_lazy_op (the portable bodies, MI_CHECK_NOWRAP) word for word on every case, in a child process: a trap names its record"""
    cs, rin, want = LZ.records(op)
    got, err = LZ.run_emu(emu_so, op, rin)
    assert err is None, (err[1], LZ.describe(op, cs, [err[0]]))
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert not len(bad), LZ.describe(op, cs, bad[:5])
    assert np.array_equal(got, want)


def test_host_lazy_op_refuses_an_unknown_op(emu):
    buf = np.zeros(LZ.IN_W, np.uint32); out = np.zeros(LZ.OUT_W, np.uint32)
    for op in (-1, LZ.OP_END, 1000):
        assert emu.emu_lazy_op(C.c_int(op), _p(out), _p(buf), C.c_size_t(1)) != 0


@pytest.mark.parametrize("log_n,log_e,mc,ms", PLANS)
def test_structured_ntt_inputs_through_the_trapping_emulator(emu, log_n, log_e, mc, ms):
    """zeros, constants, root powers, deltas, periodic vectors: every flag combination equals the oracle bit for bit (a true zero is eight
    zero limbs) and the closed forms, and no bound of the lazy arithmetic trips"""
    n = 1 << log_n
    rev = LZ.bitrev_index(log_n)
    for case in LZ.ntt_cases(log_n):
        for flags in range(8):
            a = case.physical(flags, rev)
            got = a.copy()
            assert emu.emu_ntt(_p(got), log_n, flags, log_e, mc, ms, 64, n) >= 1
            assert np.array_equal(got, cref.ntt(a, log_n, flags)), (case.name, flags)
            assert not LZ.ntt_closed_form_errors(case, got, log_n, flags, rev), (case.name, flags)


def _emu_compute_h(emu, plan, a, b, c):
    """computeH out of the emulator's transforms, the way the device composes it: h = den (FFTInverse_coset(ca o cb) - FFTInverse(c)), the
    product and the subtraction fused into the edges of the last transform (NttPass::load_mul / store_sub)"""
    log_n, log_e, mc, ms = plan
    n = 1 << log_n
    def tr(v, flags, n_valid=n, load_mul=None, store_sub=None):
        d = np.zeros((n, 4), np.uint64); d[: len(v)] = v
        assert emu.emu_ntt_fused(_p(d), log_n, flags, log_e, mc, ms, 64, n_valid, _p(load_mul), _p(store_sub)) >= 1
        return d
    ia, ib, ic = (tr(v, LZ.INVERSE, n_valid=len(v)) for v in (a, b, c))
    ca, cb = tr(ia, LZ.COSET | LZ.DIT), tr(ib, LZ.COSET | LZ.DIT)
    t = tr(ca, LZ.INVERSE | LZ.COSET, load_mul=cb, store_sub=ic)
    import closed_forms as cf
    den = pow(pow(5, n, LZ.P_) - 1, -1, LZ.P_)
    return cref.field_op(0, 2, t, cf.bcast(den, n))


@pytest.mark.parametrize("plan", [p for p in PLANS if p[0] >= 4])
def test_structured_compute_h_inputs_through_the_trapping_emulator(emu, plan):
    """a = 0, constants, a = b, a b - c the zero polynomial (h is exact zeros out of non-zero data: store_sub meets two representatives of
    one residue), sparse polynomials, zero padding: equal to the oracle, to the closed forms, without a trap"""
    import closed_forms as cf
    log_n = plan[0]
    for case in LZ.compute_h_cases(log_n):
        want = cref.compute_h(log_n, case.a, case.b, case.c)
        if case.zero_h:
            assert not want.any(), case.name
        if case.poly:
            assert not cf.compute_h_check(want, log_n, *case.poly), case.name
        got = _emu_compute_h(emu, plan, case.a, case.b, case.c)
        assert np.array_equal(got, want), case.name

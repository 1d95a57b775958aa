"""CPU: tests/banded.py without a device -- what its fill guarantees, its offset arithmetic and its report (over a host stand-in for
mi_dev_alloc / mi_dev_upload / mi_dev_download), and that every input set of tests/test_gpu_buffer_bounds.py and
tests/test_gpu_call_history.py reaches what it is there for."""
import ctypes as C
import numpy as np
import pytest
import pyref as P
import cref
import banded as BD
import fixed_base_cases as FB
import generic_msm_cases as G
from helpers import fr_vals


class _HostArray:
    def __init__(self, nbytes):
        self.buf = np.zeros(nbytes + 256, np.uint8)
        self.ptr = (self.buf.ctypes.data + 255) & ~255          # hipMalloc's alignment

    def free(self):
        self.buf = None


class _HostLib:
    @staticmethod
    def mi_dev_upload(h, dst, src, n):
        C.memmove(dst.value, src.value, n.value); return 0

    @staticmethod
    def mi_dev_download(h, dst, src, n):
        C.memmove(dst.value, src.value, n.value); return 0


class HostCtx:
    """host memory behind the three calls a Banded makes"""
    lib, h = _HostLib, None

    def alloc(self, nbytes):
        return _HostArray(nbytes)

    def _ck(self, rc):
        assert rc == 0


def _int(word):
    return int.from_bytes(bytes(word), "little")


# ---------------------------------------------------------------------------------------------------- the fill
@pytest.mark.parametrize("seed", [0, 1, 0x6261])
def test_no_aligned_word_of_the_fill_is_a_reduced_field_element(seed):
    s = BD.pattern(BD.GUARD + 4096, seed)
    assert s.dtype == np.uint8 and (s[31::32] >= 0x80).all()
    words = [_int(s[i:i + 32]) for i in range(0, len(s), 32)]
    assert min(words) >= 1 << 255 > P.Q_MOD > P.R_MOD
    assert len(set(words)) == len(words)                               # a stream, not one repeated word
    assert np.array_equal(s, BD.pattern(len(s), seed)) and not np.array_equal(s, BD.pattern(len(s), seed + 1))
    # read as points the way the library stores them (Montgomery limbs), the first 64 and 128 bytes lie on neither curve, reduced or not
    for at in (0, BD.GUARD + 32):
        x, y = (P.fp_from_mont(_int(s[at + 32 * k:at + 32 * k + 32]) % P.Q_MOD) for k in range(2))
        assert not P.g1_is_on_curve((x, y))
        v = [P.fp_from_mont(_int(s[at + 32 * k:at + 32 * k + 32]) % P.Q_MOD) for k in range(4)]
        assert not P.g2_is_on_curve(((v[0], v[1]), (v[2], v[3])))
    # and as Fr values (what an NTT or an MSM would take them for) they are not what zero padding gives
    assert all(w % P.R_MOD for w in words[:64])


# ---------------------------------------------------------------------------------------------------- offsets
@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("payload", [0, 1, 32, 33, 64 * 257, 384])
def test_layout_and_alignment(payload, odd):
    off, total = BD.layout(payload, odd=odd)
    assert off == BD.GUARD + 32 + odd and total == off + payload + BD.GUARD
    assert BD.GUARD == 2 * 4096 * 32                                    # twice the largest NTT tile (log_e <= 12)
    b = BD.Banded(HostCtx(), payload, odd=odd)
    assert b.ptr - b.base == off and b.ptr % 32 == odd and b.ptr % 64 == 32 + odd
    assert b.total == total
    assert np.array_equal(b._get(b.base, total), BD.pattern(total, b.seed))          # guards and payload start as the stream
    b.check()
    data = np.arange(payload, dtype=np.uint8)
    b.upload(data)
    assert np.array_equal(b.download(payload, np.uint8), data)
    b.assert_unchanged(data)                                            # an upload touches the payload only
    assert np.array_equal(b.refill().download(payload, np.uint8), b.initial())


def test_two_buffers_do_not_share_a_stream():
    ctx = HostCtx()
    a, b = BD.Banded(ctx, 64), BD.Banded(ctx, 64)
    assert a.seed != b.seed and not np.array_equal(a.initial(), b.initial())


# ---------------------------------------------------------------------------------------------------- the report
@pytest.mark.parametrize("side,at,first,last,count", [("after", [0], 0, 0, 1), ("before", [0], 0, 0, 1), ("after", [5, 4095], 5, 4095, 2),
                                                      ("before", [31, 32, 200], 31, 200, 3), ("after", [BD.GUARD - 1], BD.GUARD - 1, BD.GUARD - 1, 1)])
def test_check_names_side_offsets_and_count(side, at, first, last, count):
    b = BD.Banded(HostCtx(), 96, name="probe")
    for k in at:
        addr = b.ptr + b.nbytes + k if side == "after" else b.ptr - 1 - k
        b._put(addr, b._get(addr, 1) ^ np.uint8(0xFF))
    with pytest.raises(AssertionError) as e:
        b.check()
    msg = str(e.value)
    assert f"probe (96 bytes): guard {side} the payload touched: {count} bytes changed, nearest at offset {first}, farthest at offset {last}" in msg
    assert ("before" if side == "after" else "after") not in msg
    with pytest.raises(AssertionError):
        b.assert_unchanged(b.initial())


def test_assert_unchanged_sees_a_written_input():
    b = BD.Banded.of(HostCtx(), np.arange(40, dtype=np.uint64))
    b.assert_unchanged(np.arange(40, dtype=np.uint64))
    b._put(b.ptr + 17, np.array([0xEE], np.uint8))
    with pytest.raises(AssertionError, match="const input was written: 1 bytes changed, the first at byte 17"):
        b.assert_unchanged(np.arange(40, dtype=np.uint64))
    b.check()                                                           # the guards are still whole


# ---------------------------------------------------------------------------------------------------- the input sets
def test_ragged_sizes_are_ragged():
    for n in BD.RAGGED + (G.small_n(4),):
        assert all(n % k for k in (16, 64, 256, 512)), n
    used = set(BD.FIELD_NS + BD.GEN_NS + BD.MSM_NS + BD.FIXED_NS + BD.BSM_NS + BD.CODEC_NS + BD.VERIFY_NS)
    assert used - {1} == set(BD.RAGGED)                                 # every size but 1 is a ragged one
    # a tail (63), a full wave and one more (65), a second workgroup (257); around the conversion's groups of 16
    assert {15, 17} <= set(BD.BSM_NS) and {63, 65, 257} <= set(BD.FIELD_NS)
    for log_n, _ in BD.H_ROWS:
        N = 1 << log_n
        counts = BD.h_constraint_counts(log_n)
        assert counts == ([1, 5, 8] if log_n == 3 else [1, N // 2 + 1, N - 11, N])
        assert all(k % 16 for k in counts[1:-1])
    assert all(((1 << k) - 11) % 16 for k in BD.PROVE_LOG_NS)


def test_shrinking_compute_h_inputs_are_non_zero_where_a_shorter_call_must_not_look():
    a, b, c = BD.shrinking_vectors(7000)
    assert BD.H_SHRINK == (1024, 1013, 513, 1) and BD.H_SHRINK[0] == 1 << BD.H_LOG_N
    for v in (a, b, c):
        assert v.shape == (1024, 4) and v.any(axis=1).all()
        assert 0 not in fr_vals(v[[0, 1, 512, 513, 1012, 1013, 1023]])
    assert not np.array_equal(a, b) and not np.array_equal(b, c)
    # and the product the library forms for c == NULL is non-zero there too
    assert cref.field_op(0, 2, a, b).any(axis=1).all()


def test_dirtying_generic_msm_fills_every_window():
    c, top = BD.MSM_C, G.top_window(BD.MSM_C)
    vals = BD.msm_dirty_scalars()
    # one_value: a non-zero digit in every window up to the top one: each holds one key with all n entries
    d = FB.digits(vals["one_value"], c)
    assert c in G.ONE_VALUE_WIDTHS and 0 not in d[:top + 1] and len(d) == FB.nwin(c)
    # r - 1 is a multiple of 2^28: windows 0..2 are empty, every window from 3 to the top one holds all n entries in one key, and in
    # another key than one_value's
    d1 = FB.digits(vals["r_minus_1"], c)
    assert sum(x << (c * w) for w, x in enumerate(d1)) == P.R_MOD - 1 and (P.R_MOD - 1) % (1 << 28) == 0
    assert d1[:3] == [0, 0, 0] and 0 not in d1[3:top + 1]
    assert all(x != y for x, y in zip(d[:top + 1], d1[:top + 1]))
    # what the probes leave empty: the zero scalars no window, lone_first one window, lone_last one
    assert [w for w, x in enumerate(FB.digits(G.LONE_FIRST, c)) if x] == [0]
    assert [w for w, x in enumerate(FB.digits(G.LONE_LAST, c)) if x] == [240 // c]
    assert BD.MSM_DIRTY_N > G.small_n(c) > 300


def test_dirtying_fixed_base_msm_and_its_probes():
    c = BD.FIXED_C
    full = [FB.digits(v, c) for v in fr_vals(BD.nonzero_scalars(BD.FIXED_DIRTY_N, 7200))]
    top = G.top_window(c)
    assert all(any(d[w] for d in full) for w in range(top + 1))         # entries in every window
    assert len({(w, abs(d[w])) for d in full for w in range(top + 1) if d[w]}) > 8000   # nearly every entry a bucket of its own
    pr = BD.fixed_probe_scalars()
    assert set(pr) == {"edges", "zeros", "lone_64"} and all(v.shape == (BD.FIXED_PROBE_N, 4) for v in pr.values())
    G.assert_reaches_the_digit_edges(c, fr_vals(pr["edges"]))
    assert not pr["zeros"].any()
    assert [i for i, v in enumerate(fr_vals(pr["lone_64"])) if v] == [64]


def test_batch_scalar_mul_inputs():
    for n in BD.BSM_NS:
        v = fr_vals(BD.bsm_scalars(n, 7300 + n))
        assert v[n - 1] == 0 and (n == 1 or v[:min(3, n - 1)] == [0, 1, P.R_MOD - 1][:min(3, n - 1)])
        assert all(v[3:n - 1])
    v = fr_vals(BD.bsm_probe_scalars(7400))
    assert [i for i, x in enumerate(v) if not x] == list(range(16)) + [64]
    assert all(fr_vals(BD.nonzero_scalars(BD.BSM_DIRTY_N, 7401)))

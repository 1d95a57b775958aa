"""Device buffers with a guard band on each side, for tests/test_gpu_buffer_bounds.py and tests/test_gpu_call_history.py, and the input
sets of those two files; tests/test_banded_cpu.py checks both without a device.  Nothing here calls a kernel: only mi_dev_alloc,
mi_dev_upload and mi_dev_download, pyref's integers and the C oracle's generators.

A Banded is ONE mi_dev_alloc of guard + 32 + payload + guard bytes (one byte more with `odd`), filled from a seeded byte stream:

    base                      base + guard + 32 (+ 1 with odd)                          end
    | guard before ........... | payload ........................... | guard after ..... |

  * base is a hipMalloc address (256-byte aligned at least; asserted to be 64-byte aligned), guard is a multiple of 64, so the payload
    starts on a 32-byte boundary that is NOT a 64-byte boundary: the alignment the header promises for a device pointer and no better.
    `odd` adds one byte more, for the byte strings documented as "any alignment".
  * the guard is a condition, not a measurement: 256 KiB is twice the largest tile an accepted NTT plan can address (log_e <= 12:
    4096 x 32 bytes = 128 KiB) and far above every other kernel's unit of work.  A stray access of one unit of work stays inside
    memory this buffer owns; nothing is ever placed at the end of an allocation and nothing is freed between a call and its check.
  * the top byte of every aligned 32-byte word of the stream is at least 0x80: every such word is at least 2^255 as a little-endian
    integer, so it is no reduced Fr or Fp element, and a kernel that reads into a guard and uses what it finds cannot reproduce the
    result of the oracle, which pads with zeros.

check() downloads both guards and compares them with the regenerated stream; assert_unchanged(arr) does the same and compares the
payload with what was uploaded (for a `const` argument)."""
import ctypes as C
import itertools
import numpy as np
import pyref as P
import cref
from helpers import fr_arr
import fixed_base_cases as FB
import generic_msm_cases as G

GUARD = 256 << 10
WORD = 32
_seeds = itertools.count(0x6261)


def pattern(nbytes, seed):
    """the byte stream of an allocation of nbytes whose base is 32-byte aligned"""
    s = np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8)
    s[WORD - 1::WORD] |= 0x80
    return s


def layout(payload_bytes, guard=GUARD, odd=False):
    """(offset of the payload from the base, bytes of the whole allocation)"""
    assert guard % 64 == 0 and guard >= WORD and payload_bytes >= 0
    off = guard + WORD + (1 if odd else 0)
    return off, off + payload_bytes + guard


def describe(got, want, side):
    """None when the guard `side` ('before' or 'after') the payload is unchanged, else the report: side, first and last changed byte as
    offsets from the payload's edge (0 = the byte that touches the payload), how many bytes changed"""
    bad = np.flatnonzero(got != want)
    if not len(bad):
        return None
    if side == "after":
        first, last = int(bad[0]), int(bad[-1])
    else:
        first, last = len(want) - 1 - int(bad[-1]), len(want) - 1 - int(bad[0])
    return f"guard {side} the payload touched: {len(bad)} bytes changed, nearest at offset {first}, farthest at offset {last} from the payload's edge"


class Banded:
    def __init__(self, ctx, payload_bytes, guard=GUARD, odd=False, name="buffer", seed=None):
        self.ctx, self.nbytes, self.guard, self.name = ctx, int(payload_bytes), guard, name
        self.seed = next(_seeds) if seed is None else seed
        self.off, self.total = layout(self.nbytes, guard, odd)
        self.dev = ctx.alloc(self.total)
        self.base = int(self.dev.ptr)
        assert self.base % 64 == 0, "mi_dev_alloc returned less than 64-byte alignment: the payload's address would not be what this file says"
        self.ptr = self.base + self.off
        assert self.ptr % 64 == (33 if odd else 32)
        self._put(self.base, pattern(self.total, self.seed))

    @classmethod
    def of(cls, ctx, arr, odd=False, name="input", guard=GUARD):
        """a buffer that holds exactly arr"""
        arr = np.ascontiguousarray(arr)
        return cls(ctx, arr.nbytes, guard, odd, name).upload(arr)

    # ---- raw copies at any address of the allocation
    def _put(self, ptr, arr):
        if arr.nbytes:
            self.ctx._ck(self.ctx.lib.mi_dev_upload(self.ctx.h, C.c_void_p(ptr), arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes)))

    def _get(self, ptr, nbytes):
        out = np.zeros(nbytes, np.uint8)
        if nbytes:
            self.ctx._ck(self.ctx.lib.mi_dev_download(self.ctx.h, out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(nbytes)))
        return out

    # ---- the payload
    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        self._put(self.ptr, arr)
        return self

    def download(self, shape, dtype=np.uint64):
        out = np.zeros(shape, dtype)
        assert out.nbytes <= self.nbytes
        return self._get(self.ptr, out.nbytes).view(dtype).reshape(out.shape) if out.nbytes else out

    def refill(self):
        """the payload back to the stream's bytes (an output before its next call)"""
        self._put(self.ptr, self.initial())
        return self

    def initial(self):
        return pattern(self.total, self.seed)[self.off:self.off + self.nbytes]

    # ---- the checks
    def report(self):
        want = pattern(self.total, self.seed)
        end = self.off + self.nbytes
        msgs = [describe(self._get(self.base, self.off), want[:self.off], "before"),
                describe(self._get(self.base + end, self.total - end), want[end:], "after")]
        return [f"{self.name} ({self.nbytes} bytes): {m}" for m in msgs if m]

    def check(self):
        msgs = self.report()
        assert not msgs, "; ".join(msgs)

    def assert_unchanged(self, arr):
        """a const argument: the guards are the stream's and the payload is arr, bit for bit"""
        self.check()
        arr = np.ascontiguousarray(arr)
        got = self._get(self.ptr, self.nbytes)
        bad = np.flatnonzero(got != arr.reshape(-1).view(np.uint8))
        assert not len(bad), f"{self.name}: a const input was written: {len(bad)} bytes changed, the first at byte {int(bad[0])}, the last at byte {int(bad[-1])} of {self.nbytes}"

    def free(self):
        self.dev.free()


# ---------------------------------------------------------------------------------------------------- the input sets
r = P.R_MOD
# sizes the rows of tests/test_gpu_buffer_bounds.py call ragged: no multiple of a conversion group (16), a wave (64), a workgroup (256)
# or a sort slice (512)
RAGGED = (15, 17, 63, 65, 130, 257)
FIELD_NS = (1, 63, 65, 257)
GEN_NS = (1, 65, 257)
MSM_NS = (1, 63, 65)
FIXED_NS, FIXED_C = (1, 17, 65), 17
BSM_NS = (1, 15, 17, 65, 257)
CODEC_NS = (1, 63, 65, 257)
VERIFY_NS = (1, 63, 65, 130)
DEFAULT_PLAN, DEFAULT_WAVE = (9, 9, 7), (1, 12)
# (log_n, plan or None, wave-stage knob or None)
NTT_ROWS = [(k, None, None) for k in (0, 1, 2, 5, 6, 7, 9, 10)] + [(10, (6, 3, 3), None), (13, (7, 5, 4), None), (9, None, (1, 12)), (9, None, (0, 12))]
H_ROWS = [(3, None), (7, None), (10, None), (14, (8, 7, 7))]
PROVE_LOG_NS = (8, 10)


def h_constraint_counts(log_n):
    """1, N / 2 + 1, N - 11, N; at N = 8 there is no N - 11"""
    N = 1 << log_n
    return sorted({k for k in (1, N // 2 + 1, N - 11, N) if 1 <= k <= N})


def nonzero_scalars(n, seed):
    """n seeded Montgomery scalars, none of them zero"""
    sc = cref.gen_scalars(n, seed, 0)
    zero = ~sc.any(axis=1)
    sc[zero] = fr_arr([1])[0]
    return sc


def bsm_scalars(n, seed):
    """batch scalar multiplication: 0, 1, r - 1 in front where they fit, 0 (an infinity output) at the ragged end"""
    sc = nonzero_scalars(n, seed)
    for i, v in enumerate((0, 1, r - 1)[:max(n - 1, 0)]):
        sc[i] = fr_arr([v])[0]
    sc[n - 1] = 0
    return sc


# ---- tests/test_gpu_call_history.py
H_LOG_N, H_SHRINK, H_BIG_LOG_N = 10, (1024, 1013, 513, 1), 12
MSM_C, MSM_DIRTY_N = 8, 5000
FIXED_DIRTY_N, FIXED_PROBE_N = 600, 65
BSM_DIRTY_N, BSM_PROBE_N = 1000, 65


def shrinking_vectors(seed):
    """a, b, c of the longest computeH call of the shrinking sequence: every element non-zero, so that every index a shorter call must
    ignore holds something"""
    return tuple(nonzero_scalars(H_SHRINK[0], seed + k) for k in range(3))


def msm_dirty_scalars(seed=7100):
    """the scalar each of the two dirtying generic MSMs has at all its MSM_DIRTY_N places, as an integer: r - 1, then one_value"""
    return {"r_minus_1": r - 1, "one_value": G._one_value(seed)}


def fixed_probe_scalars(n=FIXED_PROBE_N):
    """name -> n Montgomery scalars: the edge scalars of width 17 (cycled), all zeros, a lone non-zero scalar at index 64"""
    edge = G.width_scalars(FIXED_C)
    lone = np.zeros((n, 4), np.uint64); lone[64] = fr_arr([(1 << 200) + 12345])[0]
    return {"edges": fr_arr([edge[i % len(edge)] for i in range(n)]), "zeros": np.zeros((n, 4), np.uint64), "lone_64": lone}


def bsm_probe_scalars(seed):
    """n = 65 with zeros exactly where the dirtying call had its first group of 16 and at the last index"""
    sc = nonzero_scalars(BSM_PROBE_N, seed)
    sc[:16] = 0; sc[BSM_PROBE_N - 1] = 0
    return sc

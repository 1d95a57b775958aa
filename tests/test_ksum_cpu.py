"""CPU suite: kSum of a whole batch over a window table (include/mi355x_groth16_verify_ksum.h) in the host build of its own text
(tests/emu/emu_ksum.cpp over csrc/ksum_ops.cuh, -DMI_CHECK_NOWRAP): the window policy at its budget edges, the cut of a row into slices,
table entries and row sums against integers in the exponent at every width, verify_assemble as the device runs it (one lane per proof
over arrays that lie side by side) against the pairs pyref lays out, and the same text under AddressSanitizer over blocks of exactly
the computed sizes (tests/cpp/ksum_asan.cpp)."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import pyref as P
import verify_cases as V
import ksum_cases as K
from helpers import fr_arr, g1_arr, g2_arr
from gpu_common import ROOT


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    lib = C.CDLL(K.build_emu(str(tmp_path_factory.mktemp("emu") / "libemu_ksum.so")))
    lib.emu_ksum_table_bytes.restype = C.c_uint64
    lib.emu_ksum_slice_terms.restype = C.c_uint64
    return lib


def _bits(emu, ns, budget):
    return emu.emu_ksum_window_bits(C.c_uint(ns), C.c_uint64(budget))


def test_window_policy_at_its_budget_edges(emu):
    assert [K.windows(c) for c in K.WIDTHS] == [32, 64, 127] == [emu.emu_ksum_windows(C.c_uint(c)) for c in K.WIDTHS]
    assert [K.table_bytes(1, c) for c in K.WIDTHS] == [522240, 61440, 24384]
    for ns in (1, 2, 5, 65, 300, 4098):
        for c in K.WIDTHS:
            b = K.table_bytes(ns, c)
            assert emu.emu_ksum_table_bytes(C.c_uint(ns), C.c_uint(c)) == b
            assert _bits(emu, ns, b) == c, "a table that fits exactly is taken"
            assert _bits(emu, ns, b - 1) == (c // 2 if c > 2 else 0), "one byte less: the next width, or none"
        assert _bits(emu, ns, 0) == 0 and _bits(emu, ns, (1 << 64) - 1) == 8
    assert _bits(emu, 0, (1 << 64) - 1) == 0, "a key without bases has no table"
    # what the header says of the default budget
    want = {128: 8, 129: 4, 1092: 4, 1093: 2, 2752: 2, 2753: 0, 4098: 0}
    assert {ns: _bits(emu, ns, K.DEFAULT_BUDGET) for ns in want} == want == {ns: K.window_bits(ns, K.DEFAULT_BUDGET) for ns in want}


def test_the_cut_of_a_row_into_slices(emu):
    sl = lambda ns, c, n: emu.emu_ksum_slices(C.c_uint(ns), C.c_uint(c), C.c_uint64(n))
    assert sl(4, 8, 1) == 128 and sl(1, 8, 1) == 32, "one proof: a lane per term"
    assert sl(65, 8, 1) == 1024 and sl(4096, 4, 1) == 1024, "at most 1024 slices"
    assert sl(4, 8, 16384) == 16 and sl(4096, 4, 16384) == 16, "16384 proofs: 2^18 lanes"
    assert sl(4, 8, 1 << 18) == 1 == sl(4, 8, 1 << 24), "from 2^18 proofs on a lane is a proof"
    for ns, c, n in ((1, 8, 1), (5, 4, 63), (65, 8, 130), (300, 2, 130), (4, 8, 16384), (300, 4, 1 << 24)):
        s = sl(ns, c, n)
        assert s == K.slices(ns, c, n)
        terms = ns * K.windows(c)
        per = emu.emu_ksum_slice_terms(C.c_uint(ns), C.c_uint(c), C.c_uint(s))
        assert per == -(-terms // s) and 1 <= s <= min(terms, K.MAX_SLICES), (ns, c, n)
    assert [emu.emu_ksum_reduce_lanes(C.c_uint(s)) for s in (1, 2, 3, 16, 33, 64, 65, 1024)] == [1, 2, 4, 16, 64, 64, 64, 64]


@pytest.fixture(scope="module")
def tables(emu):
    """the host build's table of every (key kind, width) the tests below read: 3 bases"""
    made = {}

    def get(kind, c, ns=3):
        if (kind, c, ns) not in made:
            exps = K.key_exps(ns, kind)
            k = g1_arr([K.point(e) for e in exps])
            t = np.zeros((ns, K.windows(c), (1 << c) - 1, 8), np.uint64)
            assert t.nbytes == K.table_bytes(ns, c)
            assert emu.emu_ksum_table(V.p_(k), C.c_uint(ns), C.c_uint(c), V.p_(t)) == 0
            made[(kind, c, ns)] = (exps, t)
        return made[(kind, c, ns)]
    return get


@pytest.mark.parametrize("c", K.WIDTHS)
def test_table_entries_are_the_multiples_of_the_bases(tables, c):
    """T[j][w][d - 1] = d 2^(c w) K[1 + j]: the first, the last and seeded entries of every base, the top window among them; a base at
    infinity gives a row of zeros"""
    exps, t = tables("inf", c)
    assert exps[0] == 0 and not t[0].any() and not t[2].any() and t[1].any(axis=-1).all()
    exps, t = tables("plain", c)
    rng = np.random.default_rng(80 + c)
    W, per = K.windows(c), (1 << c) - 1
    picks = {(j, w, d) for j in range(3) for w, d in ((0, 1), (0, per), (W - 1, 1), (W - 1, per), (1, 2))}
    picks |= {(int(rng.integers(3)), int(rng.integers(W)), int(rng.integers(1, per + 1))) for _ in range(12)}
    for j, w, d in sorted(picks):
        want = g1_arr([K.point(d * (1 << (c * w)) * exps[j])])[0]
        assert np.array_equal(t[j, w, d - 1], want), (j, w, d)


@pytest.mark.parametrize("c", K.WIDTHS)
@pytest.mark.parametrize("kind", K.KEY_KINDS)
def test_row_sums_equal_the_sum_in_the_exponent(emu, tables, kind, c):
    """every edge row under the slices the policy chooses for the batch and under forced ones: one slice, one slice per base (equal
    bases then meet in the general addition: its doubling and cancelling branches), more slices than a lane per term needs (empty
    slices), and a prime; a skipped row is infinity whatever its words are"""
    exps, t = tables(kind, c)
    ns = 3
    rows = K.edge_rows(ns)
    scal = K.rows_arr(rows, ns)
    want = K.expected_points(exps, rows)
    assert not want[0].any(), "the all-zero row sums to infinity"
    if kind == "equal":
        assert not want[8].any() and want[7].any(), "scalars that sum to r cancel on equal bases"
    if kind == "opposite":
        assert not want[7].any() and want[8].any(), "equal scalars cancel on opposite bases"
    W = K.windows(c)
    for forced in (0, 1, ns, 7, ns * W, 1024):
        got = np.full((len(rows), 8), 255, np.uint64)
        assert emu.emu_ksum_batch(V.p_(t), C.c_uint(ns), C.c_uint(c), V.p_(scal), None, C.c_size_t(len(rows)), C.c_uint(forced), V.p_(got)) == 0
        assert np.array_equal(got, want), (kind, c, forced, [i for i in range(len(rows)) if not np.array_equal(got[i], want[i])])
    skip = np.zeros(len(rows), np.uint8); skip[[1, 6]] = 1
    junk = scal.copy(); junk[[1, 6]] = np.uint64((1 << 64) - 1)      # words no field element has: never read
    got = np.full((len(rows), 8), 255, np.uint64)
    assert emu.emu_ksum_batch(V.p_(t), C.c_uint(ns), C.c_uint(c), V.p_(junk), V.p_(skip), C.c_size_t(len(rows)), C.c_uint(0), V.p_(got)) == 0
    keep = skip == 0
    assert np.array_equal(got[keep], want[keep]) and not got[~keep].any()


@pytest.mark.parametrize("nc", [0, 1, 2])
def test_verify_assemble_one_lane_per_proof_lays_out_pyref_s_pairs(emu, nc):
    """three proofs side by side: the toy proof, the same with another Krs, and a flagged one whose records are zeros (its pairs are
    infinities); the sums of the rows are pyref's"""
    case = V.toy_case(nc)
    other = dict(case, proof=(case["proof"][0], case["proof"][1], P.g1_mul(P.G1_GEN, 1009)))
    vk, nbp = case["vk"], case["vk"]["nb_public"]
    d, _, ped = V.vk_arrays(vk)
    msm = None
    for s, pt in zip(list(case["public_inputs"]) + list(case["commitment_values"]), vk["k"][1:]):
        msm = P.g1_add(msm, P.g1_mul(pt, s % P.R_MOD))
    n, np_ = 3, 3 + (nc + 1 if nc else 0)
    pd = [V.proof_dict(case), V.proof_dict(other)]
    raw = np.zeros((n, 32), np.uint64); raw[:2] = [x["raw"] for x in pd]
    ar, bs, krs = (np.ascontiguousarray(raw[:, a:b]) for a, b in ((0, 8), (8, 24), (24, 32)))
    cm = np.zeros((n, max(nc, 1), 8), np.uint64); pok = np.zeros((n, 8), np.uint64); fold = np.zeros((n, 4), np.uint64)
    if nc:
        cm[:2] = [x["commitments"] for x in pd]; pok[:2] = [x["pok"] for x in pd]; fold[:2] = [x["fold_challenge"] for x in pd]
    flags = np.array([0, 0, 1], np.uint8)
    msm_arr = np.ascontiguousarray(np.repeat(g1_arr([msm]), n, axis=0))
    p = np.full((n, np_, 8), 255, np.uint64); q = np.full((n, np_, 16), 255, np.uint64)
    k0 = np.ascontiguousarray(d["k"][0])
    assert emu.emu_verify_assemble_arrays(V.p_(k0), V.p_(d["gamma2"]), V.p_(d["delta2"]), V.p_(ped), C.c_uint(nbp - 1), C.c_uint(nc), V.p_(ar), V.p_(bs),
                                          V.p_(krs), V.p_(cm), V.p_(pok), V.p_(fold), V.p_(flags), V.p_(msm_arr), C.c_size_t(n), V.p_(p), V.p_(q)) == 0
    for i, c in enumerate((case, other)):
        want_p, want_q, n_ped = V.emu_pairs(c)
        assert n_ped == np_ - 3 and np.array_equal(p[i], want_p) and np.array_equal(q[i], want_q), (nc, i)
    assert not p[2].any() and not q[2].any()


def test_ksum_text_under_address_sanitizer():
    """tests/cpp/ksum_asan.cpp, its own main, -fsanitize=address,undefined on the host: the build of a table and the sums of a batch over
    heap blocks of exactly the sizes csrc/ksum.hip computes, every width, keys with equal bases and a base at infinity, skipped rows;
    every sum is checked inside the program against double-and-add"""
    pkg = os.path.join(ROOT, "gnark-whir_amd")
    subprocess.check_call(["make", "-C", pkg, "-s", "sanitize-ksum"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([os.path.join(pkg, "build", "ksum_asan")], capture_output=True, text=True, env=env, timeout=600)
    assert res.returncode == 0 and not res.stderr.strip(), f"rc {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-6000:]}"
    assert int(res.stdout.split()[-1]) == 102

"""What tests/test_verify_locate_cpu.py and tests/test_gpu_verify_locate.py share: the host build of the locating batch verifier
(tests/emu/emu_verify_locate.cpp), the packing of a batch of verify_forge inputs into the arrays it takes, and the batches both run."""
import ctypes as C
import functools
import os
import subprocess
import numpy as np
import verify_cases as V
import verify_forge as F
import verify_combine_ref as CR

HERE = os.path.dirname(os.path.abspath(__file__))
STAT_NAMES = ("rounds", "nodes_tested", "judged_alone", "malformed", "rejected")
CAPS = (None, 1, 2)          # the node budgets of a round the cases run under: the default, and two that force deep descents


def build_emu(so):
    """compiled like verify_cases.build_emu: every bound of the arithmetic underneath traps"""
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DMI_CHECK_NOWRAP", "-shared", "-fPIC", "-o", so,
                           os.path.join(HERE, "emu", "emu_verify_locate.cpp")])
    return so


def _packed(vk, inputs):
    d, nbp, ped = V.vk_arrays(vk)
    nc = 0 if ped is None else len(ped)

    def stack(name, shape):
        rows = [np.zeros(shape, np.uint64) if x.get(name) is None else np.asarray(x[name], np.uint64).reshape(shape) for x in inputs]
        return np.ascontiguousarray(np.stack(rows)) if rows and int(np.prod(shape)) else None
    raw, cm, pok = stack("raw", (32,)), stack("commitments", (nc, 8)), stack("pok", (8,)) if nc else None
    pub, cv = stack("public_inputs", (nbp - 1, 4)), stack("commitment_values", (nc, 4))
    fold = stack("fold_challenge", (4,)) if nc > 1 else None
    keep = (d, ped, raw, cm, pok, pub, cv, fold)
    return keep, [V.p_(d["k"]), V.p_(d["alpha1"]), V.p_(d["beta2"]), V.p_(d["gamma2"]), V.p_(d["delta2"]), V.p_(ped), C.c_uint(nbp), C.c_uint(nc),
                  V.p_(raw), V.p_(cm), V.p_(pok), V.p_(pub), V.p_(cv), V.p_(fold), C.c_size_t(len(inputs))]


def emu_verify_locate(emu, vk, inputs, seed, cap=None):
    """-> (verdicts list, stats dict) of the host build"""
    keep, args = _packed(vk, inputs)
    out, st = np.full(max(len(inputs), 1), 255, np.uint8), np.zeros(5, np.uint64)
    assert emu.emu_verify_locate(*args, seed, C.c_uint(cap or 0), V.p_(out), V.p_(st)) == 0
    return [int(v) for v in out[:len(inputs)]], dict(zip(STAT_NAMES, (int(x) for x in st)))


def emu_verify_each(emu, vk, inputs):
    """every proof alone through the host build's per-proof verifier"""
    keep, args = _packed(vk, inputs)
    out = np.full(max(len(inputs), 1), 255, np.uint8)
    assert emu.emu_verify_each(*args, V.p_(out)) == 0
    return [int(v) for v in out[:len(inputs)]]


def emu_sum_tree(emu, pts):
    pts = np.ascontiguousarray(pts, np.uint64).reshape(-1, 8)
    n, m, total = len(pts), len(pts), 0
    while True:
        m = (m + 7) // 8; total += m
        if m <= 1:
            break
    out = np.zeros((total, 8), np.uint64)
    assert emu.emu_g1_sum_tree(V.p_(pts), C.c_size_t(n), V.p_(out)) == 0
    return out


def emu_points(emu, rs, krs, cm=None, pok=None, fold=None):
    krs = np.ascontiguousarray(krs, np.uint64).reshape(-1, 8); n = len(krs)
    nc = 0 if cm is None else np.asarray(cm).reshape(n, -1, 8).shape[1]
    na = 1 + (2 if nc else 0) + (nc if nc > 1 else 0)
    kk = np.array([[k & (1 << 64) - 1, k >> 64] for k in rs], np.uint64)
    cont = lambda a: None if a is None else np.ascontiguousarray(a, np.uint64)
    cm, pok, fold = cont(cm), cont(pok), cont(fold)
    out = np.zeros((na, n, 8), np.uint64)
    assert emu.emu_locate_points(V.p_(kk), V.p_(krs), V.p_(cm), V.p_(pok), V.p_(fold), C.c_uint(nc), C.c_size_t(n), V.p_(out)) == 0
    return out


def emu_colsums(emu, scal, rs, level, nodes):
    n = len(rs)
    scal = np.ascontiguousarray(scal, np.uint64).reshape(n, -1, 4); ns = scal.shape[1]
    rr = np.zeros((n, 4), np.uint64)
    rr[:, 0] = [k & (1 << 64) - 1 for k in rs]; rr[:, 1] = [k >> 64 for k in rs]
    nd = np.ascontiguousarray(nodes, np.uint32)
    out = np.zeros((len(nd), ns + 1, 4), np.uint64)
    assert emu.emu_locate_colsums(V.p_(scal) if ns else None, C.c_uint(ns), V.p_(rr), C.c_size_t(n), C.c_uint(level), V.p_(nd), C.c_size_t(len(nd)), V.p_(out)) == 0
    return out


# ---------------------------------------------------------------------------------------------------- the batches both suites run
@functools.lru_cache(maxsize=None)
def honest_130(shape=(3, 1)):
    """130 accepted proofs of one key (130 -> 17 -> 3 -> 1: a two-proof last level-1 node under a one-child last level-2 node)"""
    key = F.forge_key(*shape)
    return key, tuple(dict(F.honest(key, 1300 + i), name=f"entry {i}") for i in range(130))


@functools.lru_cache(maxsize=None)
def inputs_130(shape=(3, 1)):
    return tuple(F.verify_input(c) for c in honest_130(shape)[1])


BAD_POSITION_NAMES = ("a", "b", "c", "d")


@functools.lru_cache(maxsize=None)
def bad_position_cases():
    """{letter: (name, key, cases, inputs)}: the 130 with the issue's four sets of bad positions.  Inputs of untouched proofs are shared."""
    key, base = honest_130()
    ins = inputs_130()
    out = {}
    for name, at, shift in (("a: first node", (0,), lambda c: CR.shift_groth(key, c, CR.T)),
                            ("b: the two-proof last node", (129,), lambda c: CR.shift_groth(key, c, CR.T)),
                            ("c: neighbours in different nodes", (63, 64), lambda c: CR.shift_groth(key, c, CR.T)),
                            ("d: the same node, Pedersen", (8, 15), lambda c: CR.shift_pedersen(c, CR.T))):
        cases, inputs = list(base), list(ins)
        for i in at:
            cases[i] = shift(base[i])
            inputs[i] = F.verify_input(cases[i])
        out[name[0]] = (name, key, cases, inputs)
    return out


def precedence_batch():
    """key (3, 3), 9 proofs: 2 has both defects (-> 1), 7 the Pedersen defect alone (-> 2)"""
    key = F.forge_key(3, 3)
    cases = [dict(F.honest(key, 1500 + i), name=f"entry {i}") for i in range(9)]
    cases[2] = CR.shift_pedersen(CR.shift_groth(key, cases[2], CR.T), CR.T)
    cases[7] = CR.shift_pedersen(cases[7], CR.T)
    return key, cases


def crafted_batches():
    """[(name, key, cases, seed, crafted_for_seed)]: defects r_5 t at 3 and -r_3 t at 5 of 20 proofs under SEED_A's coefficients of a batch
    of 20 (node (1, 0) passes under SEED_A: the nodes reuse the batch's r_i), an independent Groth16 defect at 17; the same batch under
    SEED_B; and the crafted pair alone (verify_combine_ref.cancelling_batches' pair: coefficients of a batch of 2)"""
    out = []
    for shape, what in (((3, 1), "groth"), ((3, 3), "pedersen")):
        key = F.forge_key(*shape)
        shift = (lambda c, t: CR.shift_groth(key, c, t)) if what == "groth" else CR.shift_pedersen
        cases = [dict(F.honest(key, 1700 + i), name=f"entry {i}") for i in range(20)]
        rs = CR.coefficients(CR.SEED_A, 20)
        cases[3], cases[5] = shift(cases[3], rs[5] * CR.T), shift(cases[5], -rs[3] * CR.T)
        cases[17] = CR.shift_groth(key, cases[17], 1)
        out.append((f"{what}: crafted for SEED_A", key, cases, CR.SEED_A, True))
        out.append((f"{what}: the same under SEED_B", key, cases, CR.SEED_B, False))
        r0, r1 = CR.coefficients(CR.SEED_A, 2)
        h0, h1 = F.honest(key, 300), F.honest(key, 301)
        out.append((f"{what}: the crafted pair alone", key, [shift(h0, r1 * CR.T), shift(h1, -r0 * CR.T)], CR.SEED_A, True))
    return out

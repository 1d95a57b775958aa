"""CPU suite: gnark-whir_amd/csrc/key_plan.h compiled with g++ (tests/emu/emu_key_plan.cpp) -- the fixed-base table plan against
expectations worked out by hand from the rule, the walk over the wire masks against numpy."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
M = 1 << 20
# tables of 2^20 points: windows x points x bytes per point
NEED_Z, NEED_B, NEED_AK = 13 * M * 64, 16 * M * 192, 14 * M * 128


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu") / "libemu_key_plan.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "emu", "emu_key_plan.cpp")])
    lib = C.CDLL(so)
    lib.emu_msm_nwin.restype = C.c_uint32
    return lib


def plan(emu, knob, budget, n_ak, n_b, n_z):
    out = (C.c_uint32 * 3)()
    emu.emu_fixed_base_plan((C.c_uint32 * 3)(*knob), C.c_uint64(budget), C.c_uint64(n_ak), C.c_uint64(n_b), C.c_uint64(n_z), out)
    return tuple(out)


def test_window_counts(emu):
    assert [emu.emu_msm_nwin(c) for c in (1, 2, 16, 17, 18, 19, 20, 21, 22, 128, 255, 256)] == [256, 128, 16, 16, 15, 14, 13, 13, 12, 2, 2, 1]


def test_needs_are_the_hand_worked_figures():
    assert (NEED_Z, NEED_B, NEED_AK) == (872415232, 3221225472, 1879048192)
    assert NEED_Z + NEED_B + NEED_AK == 5972688896 and NEED_Z + NEED_AK == 2751463424 and NEED_B + NEED_AK == 5100273664


@pytest.mark.parametrize("knob,budget,sizes,want", [
    ((0, 0, 0), 5972688896, (M, M, M), (19, 17, 20)),          # all three fit exactly
    ((0, 0, 0), 5972688895, (M, M, M), (0, 17, 20)),           # one byte short: A+K, the last considered, goes without
    ((0, 0, 0), 2751463424, (M, M, M), (19, 0, 20)),           # B is skipped but A+K still fits what Z left
    ((0, 0, 0), 872415231, (M, M, M), (0, 0, 0)),              # not even Z
    ((0, 0, 0), 5972688896, (M - 1, M, M), (0, 17, 20)),       # a group below 2^20 points gets none ...
    ((0, 0, 0), 5972688896, (M, M - 1, M), (19, 0, 20)),
    ((0, 0, 0), 5972688896, (M, M, M - 1), (19, 17, 0)),
    ((0, 0, 0), 5972688896 - NEED_B, (M, M - 1, M), (19, 0, 20)),   # ... and consumes nothing: the others fit in exactly their own needs
    ((0, 0, 0), 5972688896 - NEED_Z, (M, M, M - 1), (19, 17, 0)),
    ((22, 1, 0), 0, (1000, 1000, 1000), (22, 0, 0)),           # forced, never, automatic below the threshold
    ((0, 0, 22), 5100273664, (M, M, M), (19, 17, 22)),         # a forced width consumes no budget
])
def test_fixed_base_plan(emu, knob, budget, sizes, want):
    assert plan(emu, knob, budget, *sizes) == want


def wire_range_of(nb_wires, world, r, share):
    """the wire cut of a sharded key (group.hip): the lead takes share / 1000 of an even share, the others split the rest"""
    even = lambda total, w, k: (total * k // w, total * (k + 1) // w)
    if share >= 1000 or world <= 1:
        return even(nb_wires, world, r)
    lead_n = nb_wires * share // (1000 * world)
    if r == 0:
        return 0, lead_n
    a, b = even(nb_wires - lead_n, world - 1, r - 1)
    return lead_n + a, lead_n + b


def walk(emu, inf_a, inf_b, nb_public, committed, w_lo, w_hi):
    nw = len(inf_a)
    cap = max(w_hi - w_lo, 1)
    idx = [np.full(cap, 0xFFFFFFFF, np.uint32) for _ in range(3)]
    counts = (C.c_uint64 * 9)()
    ia, ib = np.ascontiguousarray(inf_a, dtype=np.uint8), np.ascontiguousarray(inf_b, dtype=np.uint8)
    cw = np.ascontiguousarray(committed, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    emu.emu_wire_indices(p(ia), p(ib), C.c_uint64(nw), C.c_uint64(nb_public), p(cw), C.c_uint64(len(cw)), C.c_uint64(w_lo), C.c_uint64(w_hi),
                         *[x.ctypes.data_as(C.c_void_p) for x in idx], counts)
    c = [int(v) for v in counts]
    return [idx[k][:c[k]].astype(np.int64) for k in range(3)], c[3:6], c[6:9]


def reference(inf_a, inf_b, nb_public, committed):
    nw = len(inf_a)
    a, b = np.flatnonzero(np.asarray(inf_a) == 0), np.flatnonzero(np.asarray(inf_b) == 0)
    k = np.array(sorted(set(range(nb_public, nw)) - set(int(c) for c in committed)), dtype=np.int64)
    return [a.astype(np.int64), b.astype(np.int64), k]


def check_cuts(emu, inf_a, inf_b, nb_public, committed, cuts):
    """cuts: consecutive ranges that cover [0, nb_wires).  The parts' lists, shifted by w_lo, concatenate to the whole key's; each part
    reports the whole key's counts and, as a0 / b0 / k0, the points of the wires before it"""
    whole = reference(inf_a, inf_b, nb_public, committed)
    got, totals, offs = walk(emu, inf_a, inf_b, nb_public, committed, 0, len(inf_a))
    assert all(np.array_equal(g, w) for g, w in zip(got, whole)) and totals == [len(w) for w in whole] and offs == [0, 0, 0]
    parts = [[], [], []]
    for lo, hi in cuts:
        got, totals, offs = walk(emu, inf_a, inf_b, nb_public, committed, lo, hi)
        assert totals == [len(w) for w in whole], (lo, hi)
        assert offs == [int((w < lo).sum()) for w in whole], (lo, hi)
        for k in range(3):
            assert all(0 <= v < hi - lo for v in got[k]), (lo, hi, k)
            parts[k].append(got[k] + lo)
    for k in range(3):
        assert np.array_equal(np.concatenate(parts[k]) if parts[k] else np.zeros(0, np.int64), whole[k]), k


def masks(nw, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 100, nw) < 10).astype(np.uint8), (rng.integers(0, 100, nw) < 50).astype(np.uint8)


@pytest.mark.parametrize("nw", [0, 1, 67])
@pytest.mark.parametrize("share", [1000, 500, 0])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_mask_walk_over_the_cuts_of_a_sharded_key(emu, nw, world, share):
    inf_a, inf_b = masks(nw, 7 * nw + world)
    nb_public = min(nw, 9)   # at 67 wires and 8 ranks the public wires span the first cut (and the lead's, whatever its share)
    committed = [c for c in (9, 10, 33, 66) if nb_public <= c < nw]   # the first and the last private wire among them
    cuts = [wire_range_of(nw, world, r, share) for r in range(world)]
    assert cuts[0][0] == 0 and cuts[-1][1] == nw and all(cuts[i][1] == cuts[i + 1][0] for i in range(world - 1))
    check_cuts(emu, inf_a, inf_b, nb_public, committed, cuts)


def test_mask_walk_edges(emu):
    nw = 67
    inf_a, inf_b = masks(nw, 3)
    # committed wires at both ends of a range, public wires that span a cut, empty ranges (at the start, inside, at the end)
    check_cuts(emu, inf_a, inf_b, 20, [20, 39, 40, 66], [(0, 0), (0, 13), (13, 13), (13, 20), (20, 40), (40, 40), (40, 67), (67, 67)])
    # all wires public; no wire public and every wire committed; no mask bit set; every mask bit set
    check_cuts(emu, inf_a, inf_b, nw, [], [(0, 30), (30, 67)])
    check_cuts(emu, inf_a, inf_b, 0, list(range(nw)), [(0, 30), (30, 67)])
    check_cuts(emu, np.zeros(nw, np.uint8), np.zeros(nw, np.uint8), 5, [6], [(0, 5), (5, 6), (6, 7), (7, 67)])
    check_cuts(emu, np.ones(nw, np.uint8), np.ones(nw, np.uint8), 5, [6], [(0, 33), (33, 67)])
    # w_lo == nb_wires: nothing in range, the offsets are the whole key's counts
    whole = reference(inf_a, inf_b, 20, [20, 66])
    got, totals, offs = walk(emu, inf_a, inf_b, 20, [20, 66], nw, nw)
    assert [len(g) for g in got] == [0, 0, 0] and totals == offs == [len(w) for w in whole]

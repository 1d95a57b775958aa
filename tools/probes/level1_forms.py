"""Every form of the MSM's level-1 launch on one context, each checked against the oracle -- what parity alone cannot show is WHICH kernel
ran, so run it under a kernel trace and compare the launch lists of two builds (tools/probes/compare_kernel_traces.py):
    rocprofv3 --kernel-trace -- python3 tools/probes/level1_forms.py
Per form one G1 MSM of 2^14 + 5 pairs and one G2 MSM of 2^12 + 5 pairs, fixed-base with c = 17 (the tables in the R' packed form wherever the
29-bit kernels are on: the generic entry points switch to them only from 2^16 / 2^14 pairs).  Scalars of the witness-like mix, items of 4 and
2 and the finisher allowed from level 0, so that the levels above and the finisher run at this size.  The batch-affine rule needs buckets of
>= 32 entries: its forms also run the generic G1 MSM of 2^16 pairs with 8-bit windows (the shape of the suite's batch-affine test)."""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import bench  # noqa: E402
import cref  # noqa: E402

B = bench._binding()
C17 = 17
ctx = B.Context(0)
lib, h = ctx.lib, ctx.h


def eq(got, want):   # (both sides are normalised Jacobian words, as in smoke())
    return np.array_equal(np.asarray(got), np.asarray(want))


class Case:
    def __init__(self, g2, n, seed):
        self.g2, self.n = g2, n
        self.pts = (cref.gen_g2 if g2 else cref.gen_g1)(n, seed)
        self.sc = cref.gen_scalars(n, seed + 1, 1)
        self.want = (cref.msm_g2 if g2 else cref.msm_g1)(self.pts, self.sc)
        base = ctx.to_dev(self.pts)
        self.dsc = ctx.to_dev(self.sc)
        self.std = ctx.msm_precompute(base.ptr, n, C17, g2=g2)
        self.rp = ctx.msm_precompute(base.ptr, n, C17, g2=g2)
        ctx.msm_table_to_rprime(self.rp.ptr, ((256 + C17 - 1) // C17) * n, g2=g2)

    def run(self, limb29):
        tab, flags = (self.rp, 2) if limb29 else (self.std, 0)
        return eq(ctx.msm_fixed_dev(tab.ptr, self.dsc.ptr, self.n, C17, flags=flags, g2=self.g2), self.want)


g1, g2 = Case(False, (1 << 14) + 5, 0x4c31), Case(True, (1 << 12) + 5, 0x4c32)
ba_pts, ba_sc = cref.gen_g1(1 << 16, 188), cref.gen_scalars(1 << 16, 189, 1)
ba_want = cref.msm_g1(ba_pts, ba_sc)
DEFAULTS = dict(l1_wg=4, l1_waves=3, g2_wg=1, finisher=1)
bad = 0


def form(name, limb29=1, ba=0, **knobs):
    global bad
    assert lib.mi_debug_set_msm_limb29(h, limb29) == 0 and lib.mi_debug_set_msm_batch_affine(h, ba) == 0
    for k, v in {**DEFAULTS, **knobs}.items():
        ctx.set_knob(k, v)
    ok = [g1.run(limb29), g2.run(limb29)]
    if ba:
        assert lib.mi_debug_set_msm_plan(h, 8, 0, 0, 0, 0) == 0
        ctx.set_knob("item_l1", 0)
        ok.append(eq(ctx.msm_g1(ba_pts, ba_sc), ba_want))
        assert lib.mi_debug_set_msm_plan(h, 0, 0, 0, 0, 0) == 0
        ctx.set_knob("item_l1", 4); ctx.set_knob("item_l2", 2)
    bad += ok.count(False)
    print(f"{name:40s} {'ok' if all(ok) else 'MISMATCH ' + str(ok)}", flush=True)


ctx.set_knob("item_l1", 4); ctx.set_knob("item_l2", 2); ctx.set_knob("finisher_min_level", 0)
for wg in (1, 2, 4):
    for waves in (2, 3):
        form(f"l1_wg={wg} l1_waves={waves} g2_wg={wg}", l1_wg=wg, l1_waves=waves, g2_wg=wg)
for limb29 in (0, 1, 2):
    form(f"limb29={limb29}", limb29=limb29)
for ba in (0, 2):
    form(f"batch-affine rounds={ba}", ba=ba)
for fin in (1, 0):
    form(f"finisher={fin}", finisher=fin)
ctx.close()
print("level1_forms:", "all forms agree with the oracle" if not bad else f"{bad} MISMATCHES")
sys.exit(1 if bad else 0)

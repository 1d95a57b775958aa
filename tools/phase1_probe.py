"""Times a phase-1 ceremony on the device (include/mi355x_groth16_phase1.h, csrc/phase1.hip, csrc/scale_powers.cuh) and its handover
to phase 2.

    python tools/phase1_probe.py LOG_N [--sweep] [--repeats 3] [--widths 0,2,3,4,5] [--window W] [--chunk C] [--no-phase2] [--write profiles/phase1.txt]

  --sweep     the scalar multiplication of a contribution by every lane text: for w = 0 (the bit-by-bit xyzz_scale of the point NTT on the
              same scalars: the baseline) and w = 2, 3, 4, 5, one plain mi_phase1_contribute on a state of 2^LOG_N, --repeats times, the
              widths ALTERNATING inside each repeat (w = 0, 2, .., 5, then again) so that drift hits all of them alike; per row the device
              time of the scalar multiplications and of the conversions to affine (mi_phase1_get_stats), the median and the spread
              (min .. max) over the repeats.  The rows keep being re-randomised: every contribution multiplies dense points by dense scalars
  otherwise   init, ONE proved contribution (nonces from the operating system), mi_phase1_check, export, and phase 2 for the synthetic
              circuit of tools/phase2_probe.py both ways (mi_phase2_init_from_phase1 on the device rows; mi_phase2_init on the exported
              ones), wall times, the contribution's rows by phase and the peak of its own device allocations
  --window W  the knob "scale_powers_window" for the run (0, 2..5); --chunk C the knob "scale_powers_chunk" (lanes per chunk)
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np  # noqa: E402
import cref  # noqa: E402
import dlog_keys as D  # noqa: E402
import setup_cases as S  # noqa: E402
from gpu_common import load_binding  # noqa: E402

ROW_NAMES = ("tau_g1", "alpha_tau_g1", "beta_tau_g1", "tau_g2")


def rows_text(s):
    return " ".join(f"{n}: mul_ms={s['scalar_mul_ms'][i]:.1f} affine_ms={s['affine_ms'][i]:.1f}" for i, n in enumerate(ROW_NAMES))


def sweep(ctx, a, say):
    st = ctx.phase1_init(a.log_n)
    widths = tuple(int(w) for w in a.widths.split(","))
    seen = {w: [] for w in widths}
    try:
        f = cref.gen_scalars(3, 11, 0)
        ctx.phase1_contribute(st, f[0], f[1], f[2])   # away from the generator rows, and the warm-up
        for rep in range(a.repeats):
            for w in widths:
                ctx.set_knob("scale_powers_window", w)
                f = cref.gen_scalars(3, 100 + 10 * rep + w, 0)
                ctx.phase1_contribute(st, f[0], f[1], f[2])
                s = ctx.phase1_stats()
                seen[w].append(s)
                say(f"sweep log_n={a.log_n} repeat={rep} w={w} chunk={s['chunk']} total_ms={s['total_ms']:.1f} {rows_text(s)} peak_device_bytes={s['peak_bytes']}")
        base = statistics.median(sum(s["scalar_mul_ms"]) for s in seen[widths[0]])
        for w in widths:
            mul = [sum(s["scalar_mul_ms"]) for s in seen[w]]
            aff = [sum(s["affine_ms"]) for s in seen[w]]
            per_row = " ".join(f"{n}={statistics.median(s['scalar_mul_ms'][i] for s in seen[w]):.1f}" for i, n in enumerate(ROW_NAMES))
            say(f"summary log_n={a.log_n} w={w} repeats={a.repeats} scalar_mul_ms median={statistics.median(mul):.1f} min={min(mul):.1f} max={max(mul):.1f} "
                f"({per_row}) affine_ms median={statistics.median(aff):.1f} min={min(aff):.1f} max={max(aff):.1f} first_width_over_this={base / statistics.median(mul):.2f}")
        mask = ctx.phase1_check(st)
        say(f"sweep log_n={a.log_n} rows_after_{1 + a.repeats * len(widths)}_contributions check_mask={mask}")
    finally:
        ctx.phase1_free(st)


def ceremony(ctx, B, a, say):
    N = 1 << a.log_n
    t0 = time.perf_counter()
    st = ctx.phase1_init(a.log_n)
    say(f"init log_n={a.log_n} wall_ms={(time.perf_counter() - t0) * 1e3:.1f}")
    p2 = []
    try:
        f = cref.gen_scalars(3, 21, 0)
        t0 = time.perf_counter()
        rec = ctx.phase1_contribute_proved(st, f[0], f[1], f[2])
        wall = time.perf_counter() - t0
        s = ctx.phase1_stats()
        say(f"contribute_proved log_n={a.log_n} w={s['window']} chunk={s['chunk']} wall_ms={wall * 1e3:.1f} total_ms={s['total_ms']:.1f} {rows_text(s)} "
            f"peak_device_bytes={s['peak_bytes']} ({s['peak_bytes'] / 2**30:.2f} GiB) ctx_ledger={ctx.mem_ledger()}")
        gen = ctx.batch_scalar_mul(D.G1, D.ONE.reshape(1, 4))[0]
        say(f"records_verify first_bad={B.phase1_records_verify(np.stack([gen] * 3), bytes(32), 0, rec.reshape(1, -1))} (1: the record holds)")
        t0 = time.perf_counter()
        mask = ctx.phase1_check(st)
        say(f"check log_n={a.log_n} mask={mask} wall_ms={(time.perf_counter() - t0) * 1e3:.1f}")
        ctx.trim()
        if a.no_phase2:
            return
        t0 = time.perf_counter()
        r1cs = S.synth_r1cs(N - 100, nb_wires=N - 1000, nb_public=4097, seed=2300 + a.log_n, per_row=3, n_coeffs=1 << 12, n_heavy=64,
                            commitments=1, n_committed=N >> 5)
        sigma = cref.gen_scalars(1, 31, 0)
        print(f"circuit built in {time.perf_counter() - t0:.1f} s", flush=True)
        t0 = time.perf_counter()
        p2.append(ctx.phase2_init_from_phase1(r1cs, st, [sigma[0]]))
        s2 = ctx.phase2_stats()
        say(f"phase2_init_from_phase1 log_n={a.log_n} wall_ms={(time.perf_counter() - t0) * 1e3:.1f} total_ms={s2['total_ms']:.1f} upload_ms={s2['upload_ms']:.1f} "
            f"check_ms={s2['check_ms']:.1f} peak_device_bytes={s2['peak_bytes']} ({s2['peak_bytes'] / 2**30:.2f} GiB)")
        t0 = time.perf_counter()
        rows = ctx.phase1_export(st)
        say(f"export log_n={a.log_n} wall_ms={(time.perf_counter() - t0) * 1e3:.1f}")
        t0 = time.perf_counter()
        p2.append(ctx.phase2_init(r1cs, rows, [sigma[0]]))
        s2 = ctx.phase2_stats()
        say(f"phase2_init_from_export log_n={a.log_n} wall_ms={(time.perf_counter() - t0) * 1e3:.1f} total_ms={s2['total_ms']:.1f} upload_ms={s2['upload_ms']:.1f}")
        z = [ctx.phase2_array(h, B.PHASE2_G1_Z) for h in p2]
        say(f"handover log_n={a.log_n} both_routes_give_the_same_Z={np.array_equal(z[0], z[1])}")
    finally:
        for h in p2:
            ctx.phase2_free(h)
        ctx.phase1_free(st)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("log_n", type=int)
    ap.add_argument("--sweep", action="store_true", help="time a contribution by the baseline and by every window width")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--widths", default="0,2,3,4,5", help="the widths of the sweep, in the order they alternate; the first is the yardstick of the summary")
    ap.add_argument("--window", type=int, default=None, help="knob scale_powers_window for the ceremony run")
    ap.add_argument("--chunk", type=int, default=None, help="knob scale_powers_chunk")
    ap.add_argument("--no-phase2", action="store_true", help="leave the handover out")
    ap.add_argument("--write", default=None, help="append the result lines to this file")
    a = ap.parse_args()
    B = load_binding()
    ctx = B.Context(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    try:
        if a.window is not None:
            ctx.set_knob("scale_powers_window", a.window)
        if a.chunk is not None:
            ctx.set_knob("scale_powers_chunk", a.chunk)
        if a.sweep:
            sweep(ctx, a, say)
        else:
            ceremony(ctx, B, a, say)
    finally:
        ctx.close()
        if a.write:
            with open(a.write, "a") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

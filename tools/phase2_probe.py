"""Times phase-2 key generation from a powers-of-tau SRS (mi_phase2_init / contribute / seal, csrc/phase2.hip) beside groth16.Setup
on the same circuit.

    python tools/phase2_probe.py LOG_N [--check] [--write profiles/phase2.txt]

For a seeded synthetic R1CS of the benchmark's shape (2^LOG_N - 100 constraints, 2^LOG_N - 1000 wires, three entries per live row and
matrix, one BSB22 commitment over N / 32 wires; tests/setup_cases.py, the circuit of tools/setup_probe.py) it prints

  srs         building the SRS from a seeded trapdoor: the powers on the host (the oracle's vector Fr), the points by
              mi_batch_scalar_mul_g1 / _g2 -- the probe's own preparation, not part of phase 2
  init        mi_phase2_init, ONE run (no warm-up: a ceremony derives a key once): wall time, the device time of every phase from HIP
              events on the context's stream (mi_phase2_get_stats) and the peak of the call's device allocations
  contribute  mi_phase2_contribute with a delta and a sigma factor, wall time
  seal        mi_phase2_seal, wall time (the copy of the arrays and everything mi_pk_load_dev does: tables, expansions)
  setup       mi_groth16_setup for the trapdoor (tau, alpha, beta, 1, 1, sigma) on the same circuit, second run, as tools/setup_probe.py
              times it: what the same key costs when the trapdoor is known
  --check     the compressed streams of the state equal mi_groth16_setup_to_streams's, before and after the contribution

The checks of a ceremony (include/mi355x_groth16_phase2_check.h); with either flag the legs above from init on are left out:
  --check-srs mi_srs_check_powers over the probe's SRS with the operating system's seed, ONE run: wall time, the time of every phase
              (mi_srs_check_get_stats: the host's clock around work that is waited for), the peak of the call's device allocations
              and the mask (0: the SRS is honest)
  --verify    two states from the same SRS (their mi_phase2_init times are this run's yardstick), one mi_phase2_contribute_proved on
              the first, its Z, K and delta points handed to mi_phase2_verify_adopt on the second, ONE run: wall time, phases
              (mi_phase2_verify_get_stats), peak, the mask (0: adopted) and whether the adopter's Z then equals the contributor's;
              then one mi_phase2_contribute_sigma_proved on the first and its BasisExpSigma and [-sigma]2 handed to
              mi_phase2_verify_adopt_sigma on the second, timed the same way (one commitment over N / 32 wires)
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np  # noqa: E402
import pyref as P  # noqa: E402
import cref  # noqa: E402
import dlog_keys as D  # noqa: E402
import setup_cases as S  # noqa: E402
from gpu_common import load_binding  # noqa: E402

MUL = 2


def build_srs(ctx, N, td):
    pw = D.powers(td["tau"], 2 * N)
    return {"tau_g1": ctx.batch_scalar_mul(D.G1, pw),
            "alpha_tau_g1": ctx.batch_scalar_mul(D.G1, D._op(MUL, pw[:N], D._bc(td["alpha"], N))),
            "beta_tau_g1": ctx.batch_scalar_mul(D.G1, D._op(MUL, pw[:N], D._bc(td["beta"], N))),
            "tau_g2": ctx.batch_scalar_mul(D.G2, np.ascontiguousarray(pw[:N]), g2=True),
            "beta_g2": ctx.batch_scalar_mul(D.G2, td["beta"].reshape(1, 4), g2=True)[0]}


def phases(s):
    return " ".join(f"{k}={s[k]:.1f}" for k in ("total_ms", "upload_ms", "point_check_ms", "coeff_ms", "msm_g1_ms", "msm_g2_ms", "pairing_ms")) + \
        f" peak_device_bytes={s['peak_bytes']} ({s['peak_bytes'] / 2**30:.2f} GiB)"


def check_legs(ctx, B, a, N, r1cs, srs, td, say):
    if a.check_srs:
        t0 = time.perf_counter()
        mask = ctx.srs_check_powers(srs, N)
        wall = time.perf_counter() - t0
        say(f"check_srs log_n={a.log_n} mask={mask} wall_ms={wall * 1e3:.1f} {phases(ctx.srs_check_stats())} ctx_ledger={ctx.mem_ledger()}")
        ctx.trim()
    if a.verify:
        states = []
        try:
            for who in ("contributor", "verifier"):
                t0 = time.perf_counter()
                states.append(ctx.phase2_init(r1cs, srs, [td["sigma"][0]]))
                say(f"init log_n={a.log_n} state={who} wall_ms={(time.perf_counter() - t0) * 1e3:.1f} total_ms={ctx.phase2_stats()['total_ms']:.1f}")
            st, v = states
            delta = cref.gen_scalars(1, 99, 0)[0]
            t0 = time.perf_counter()
            rec = ctx.phase2_contribute_proved(st, delta)
            say(f"contribute_proved log_n={a.log_n} wall_ms={(time.perf_counter() - t0) * 1e3:.1f}")
            z, k = ctx.phase2_array(st, B.PHASE2_G1_Z), ctx.phase2_array(st, B.PHASE2_G1_K)
            d2 = ctx.batch_scalar_mul(D.G2, delta.reshape(1, 4), g2=True)[0]
            ctx.trim()
            t0 = time.perf_counter()
            mask, first_bad = ctx.phase2_verify_adopt(v, z, k, rec[:8], d2, rec.reshape(1, -1))
            wall = time.perf_counter() - t0
            say(f"verify_adopt log_n={a.log_n} points_z={len(z)} points_k={len(k)} mask={mask} first_bad_record={first_bad} wall_ms={wall * 1e3:.1f} "
                f"{phases(ctx.srs_check_stats(verify=True))} adopted_z_equals_contributors={np.array_equal(ctx.phase2_array(v, B.PHASE2_G1_Z), z)}")
            sf = cref.gen_scalars(1, 98, 0)
            t0 = time.perf_counter()
            step, h = ctx.phase2_contribute_sigma_proved(st, sf)
            say(f"contribute_sigma_proved log_n={a.log_n} commitments=1 wall_ms={(time.perf_counter() - t0) * 1e3:.1f}")
            bes, gs = ctx.phase2_array(st, B.PHASE2_BASIS + 1), ctx.phase2_get_pedersen_vk(st, 1)[:, 1].copy()
            ctx.trim()
            t0 = time.perf_counter()
            mask, bad, first_bad = ctx.phase2_verify_adopt_sigma(v, [bes], gs, step[None], [h])
            wall = time.perf_counter() - t0
            say(f"verify_adopt_sigma log_n={a.log_n} commitments=1 points_committed={len(bes)} mask={mask} bad_commitments={bad} first_bad_record={first_bad} "
                f"wall_ms={wall * 1e3:.1f} {phases(ctx.srs_check_stats(verify=True))} "
                f"adopted_bes_equals_contributors={np.array_equal(ctx.phase2_array(v, B.PHASE2_BASIS + 1), bes)}")
        finally:
            for s in states:
                ctx.phase2_free(s)


def write_lines(a, lines):
    if a.write:
        with open(a.write, "a") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("log_n", type=int)
    ap.add_argument("--check", action="store_true", help="compare the state's compressed streams with Setup's")
    ap.add_argument("--write", default=None, help="append the result lines to this file")
    ap.add_argument("--check-srs", action="store_true", help="time mi_srs_check_powers over the SRS")
    ap.add_argument("--verify", action="store_true", help="time mi_phase2_verify_adopt of one proved contribution, then the same for sigma")
    a = ap.parse_args()
    B = load_binding()
    ctx = B.Context(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    try:
        N = 1 << a.log_n
        t0 = time.perf_counter()
        r1cs = S.synth_r1cs(N - 100, nb_wires=N - 1000, nb_public=4097, seed=2300 + a.log_n, per_row=3, n_coeffs=1 << 12, n_heavy=64,
                            commitments=1, n_committed=N >> 5)
        td = S.synth_trapdoor(a.log_n, n_sigma=1)
        td["gamma"] = td["delta"] = D.ONE
        print(f"circuit built in {time.perf_counter() - t0:.1f} s", flush=True)
        t0 = time.perf_counter()
        srs = build_srs(ctx, N, td)
        ctx.trim()
        say(f"srs log_n={a.log_n} points_g1={4 * N} points_g2={N} build_s={time.perf_counter() - t0:.1f} (the probe's preparation)")
        if a.check_srs or a.verify:
            check_legs(ctx, B, a, N, r1cs, srs, td, say)
            write_lines(a, lines)
            return
        t0 = time.perf_counter()
        st = ctx.phase2_init(r1cs, srs, [td["sigma"][0]])
        wall = time.perf_counter() - t0
        s = ctx.phase2_stats()
        say(f"init log_n={a.log_n} entries={s['entries']} wall_ms={wall * 1e3:.1f} total_ms={s['total_ms']:.1f} upload_ms={s['upload_ms']:.1f} check_ms={s['check_ms']:.1f} "
            f"point_ntt_g1_ms={s['point_ntt_g1_ms']:.1f} point_ntt_g2_ms={s['point_ntt_g2_ms']:.1f} sparse_g1_ms={s['sparse_g1_ms']:.1f} "
            f"sparse_g2_ms={s['sparse_g2_ms']:.1f} z_ms={s['z_ms']:.2f} affine_ms={s['affine_ms']:.1f} long_columns={s['long_columns']} chunks={s['chunks']} "
            f"peak_device_bytes={s['peak_bytes']} ({s['peak_bytes'] / 2**30:.2f} GiB) ctx_ledger={ctx.mem_ledger()}")
        try:
            if a.check:
                want = ctx.setup_to_streams(r1cs, td, B.KEYFILE_COMPRESSED, cap=1 << 31 if a.log_n > 16 else 1 << 26, build=False)[:2]
                got = ctx.phase2_to_streams(st, B.KEYFILE_COMPRESSED, cap=len(want[0]))
                say(f"check log_n={a.log_n} streams_equal_setup_before_contribution={got == want}")
            delta, sf = cref.gen_scalars(2, 99, 0)
            t0 = time.perf_counter()
            ctx.phase2_contribute(st, delta, sf.reshape(1, 4))
            say(f"contribute log_n={a.log_n} wall_ms={(time.perf_counter() - t0) * 1e3:.1f}")
            t0 = time.perf_counter()
            pkh, peds, _ = ctx.phase2_seal(st, r1cs["nb_public"] + 1, 1)
            ctx.sync()
            say(f"seal log_n={a.log_n} wall_ms={(time.perf_counter() - t0) * 1e3:.1f} table_plan={ctx.pk_table_plan(pkh)}")
            ctx.pk_free(pkh); ctx.pedersen_pk_free(peds[0])
            td2 = dict(td, delta=delta, sigma=[D._op(MUL, td["sigma"][0].reshape(1, 4), sf.reshape(1, 4))[0]])
            if a.check:
                want = ctx.setup_to_streams(r1cs, td2, B.KEYFILE_COMPRESSED, cap=1 << 31 if a.log_n > 16 else 1 << 26, build=False)[:2]
                got = ctx.phase2_to_streams(st, B.KEYFILE_COMPRESSED, cap=len(want[0]))
                say(f"check log_n={a.log_n} streams_equal_setup_after_contribution={got == want}")
        finally:
            ctx.phase2_free(st)
        ctx.trim()
        for run in ("warm-up", "timed"):
            t0 = time.perf_counter()
            pkh, peds, _ = ctx.setup(r1cs, td)
            wall = time.perf_counter() - t0
            ss = ctx.setup_stats()
            ctx.pk_free(pkh); ctx.pedersen_pk_free(peds[0])
        say(f"setup log_n={a.log_n} wall_ms={wall * 1e3:.1f} total_ms={ss['total_ms']:.1f} sparse_ms={ss['sparse_ms']:.2f} points_ms={ss['points_ms']:.1f} "
            f"handover_ms={ss['handover_ms']:.1f} (the same key from the trapdoor in the clear)")
    finally:
        ctx.close()
    write_lines(a, lines)


if __name__ == "__main__":
    main()

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("log_n", type=int)
    ap.add_argument("--check", action="store_true", help="compare the state's compressed streams with Setup's")
    ap.add_argument("--write", default=None, help="append the result lines to this file")
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
    if a.write:
        with open(a.write, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

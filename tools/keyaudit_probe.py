"""Times the audit of a key against its circuit and SRS (mi_key_audit, csrc/keyaudit.hip) beside the derivation it replaces.

    python tools/keyaudit_probe.py LOG_N [--write profiles/keyaudit.txt]

The circuit and the SRS are those of tools/phase2_probe.py (2^LOG_N - 100 constraints, 2^LOG_N - 1000 wires, three entries per live row
and matrix, one BSB22 commitment over N / 32 wires).  In ONE run it prints

  srs        building the SRS (the probe's preparation)
  init       mi_phase2_init, ONE run: the derivation, this run's yardstick
  contribute one mi_phase2_contribute_proved, so that delta is not 1
  audit      mi_key_audit of that key with the operating system's seed, ONE run each: from the state (the claim borrows its arrays) and
             from its two compressed streams (mi_key_claim_from_streams: decode and point checks timed apart) -- wall time, every phase
             (mi_key_audit_get_stats: the host's clock around work that is waited for), the peak of the call's device allocations, the
             mask (0: the key is the circuit's) and the audit's total as a fraction of this run's mi_phase2_init
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import cref  # noqa: E402
import dlog_keys as D  # noqa: E402
import setup_cases as S  # noqa: E402
from gpu_common import load_binding  # noqa: E402
from phase2_probe import build_srs  # noqa: E402

PHASES = ("total_ms", "upload_ms", "point_check_ms", "coeff_ms", "sparse_ms", "transform_ms", "srs_msm_g1_ms", "srs_msm_g2_ms", "key_msm_g1_ms",
          "key_msm_g2_ms", "pairing_ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("log_n", type=int)
    ap.add_argument("--write", default=None, help="append the result lines to this file")
    a = ap.parse_args()
    B = load_binding()
    ctx = B.Context(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def audit(source, claim, init_ms):
        t0 = time.perf_counter()
        mask = ctx.key_audit(r1cs, claim, srs=srs)
        wall = (time.perf_counter() - t0) * 1e3
        s = ctx.key_audit_stats()
        say(f"audit log_n={a.log_n} from={source} mask={mask} wall_ms={wall:.1f} " + " ".join(f"{k}={s[k]:.1f}" for k in PHASES) +
            f" relations={s['relations']} peak_device_bytes={s['peak_bytes']} ({s['peak_bytes'] / 2**30:.2f} GiB)"
            f" audit_over_init={s['total_ms'] / init_ms:.4f} ctx_ledger={ctx.mem_ledger()}")

    try:
        N = 1 << a.log_n
        r1cs = S.synth_r1cs(N - 100, nb_wires=N - 1000, nb_public=4097, seed=2300 + a.log_n, per_row=3, n_coeffs=1 << 12, n_heavy=64,
                            commitments=1, n_committed=N >> 5)
        td = S.synth_trapdoor(a.log_n, n_sigma=1)
        td["gamma"] = td["delta"] = D.ONE
        t0 = time.perf_counter()
        srs = build_srs(ctx, N, td)
        ctx.trim()
        say(f"srs log_n={a.log_n} points_g1={4 * N} points_g2={N} build_s={time.perf_counter() - t0:.1f} (the probe's preparation)")
        t0 = time.perf_counter()
        st = ctx.phase2_init(r1cs, srs, [td["sigma"][0]])
        wall = (time.perf_counter() - t0) * 1e3
        s = ctx.phase2_stats()
        init_ms = s["total_ms"]
        say(f"init log_n={a.log_n} entries={s['entries']} wall_ms={wall:.1f} total_ms={init_ms:.1f} peak_device_bytes={s['peak_bytes']} ({s['peak_bytes'] / 2**30:.2f} GiB)")
        try:
            ctx.phase2_contribute_proved(st, cref.gen_scalars(1, 99, 0)[0])
            ctx.trim()
            cl = ctx.key_claim_from_phase2(st)
            try:
                audit("state", cl, init_ms)
            finally:
                ctx.key_claim_free(cl)
            cap = 1 << 31 if a.log_n > 20 else 1 << 28
            pk, vk = ctx.phase2_to_streams(st, B.KEYFILE_COMPRESSED, cap=cap)
        finally:
            ctx.phase2_free(st)
        ctx.trim()
        t0 = time.perf_counter()
        cl = ctx.key_claim_from_streams(pk, vk)
        wall = (time.perf_counter() - t0) * 1e3
        k = ctx.keyfile_stats()
        say(f"claim_from_streams log_n={a.log_n} pk_bytes={len(pk)} vk_bytes={len(vk)} wall_ms={wall:.1f} pk_upload_ms={k['upload_ms']:.1f} pk_decode_ms={k['decode_ms']:.1f} "
            f"pk_subgroup_ms={k['subgroup_ms']:.1f} (the wall time also holds the copy of the streams into the binding's buffers)")
        try:
            audit("streams", cl, init_ms)
        finally:
            ctx.key_claim_free(cl)
    finally:
        ctx.close()
    if a.write:
        with open(a.write, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

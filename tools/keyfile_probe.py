"""Times the key-file entry points (include/mi355x_groth16_keyfile.h, csrc/keyfile.hip) on a key mi_groth16_setup makes.

    python tools/keyfile_probe.py LOG_N [--repeats 3] [--write profiles/keyfile.txt]

The key is the one tools/setup_probe.py times: a seeded synthetic R1CS of the benchmark's shape (2^LOG_N - 100 constraints, 2^LOG_N - 1000
wires, one BSB22 commitment over N / 32 wires; tests/setup_cases.py), so every G2 point is a real member of the r-torsion.  Each figure is
the median of --repeats runs after one warm-up run of the same call; times are host clocks around calls that end in a device
synchronise (mi_keyfile_get_stats for the phases), the shader clock is sampled read-only while the timed runs go.

  write     mi_groth16_setup_to_stream's writer (mi_pk_write_dev), both encodings: encode kernels, copies to the host
  baseline  mi_pk_load_raw on the raw stream (no curve or subgroup check), as on the parent commit
  load      mi_pk_load_stream on the raw stream (curve + subgroup checks), on the compressed stream with and without the membership
            test, each split into upload / decode / subgroup / key build
  member    the membership test of G2.B by the endomorphism (63-bit multiple) against g2_in_subgroup's [r] Q (MI_KEYFILE_SUBGROUP_BY_R)
  kernels   the resource table of the new kernels (tools/kernel_resources.py: compiled, not measured)
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import setup_cases as S  # noqa: E402
from gpu_common import load_binding  # noqa: E402
from benchlib.clocks import ClockSampler  # noqa: E402

KERNELS = ["k_keyfile_decode_g1_compressed", "k_keyfile_decode_g1_raw", "k_keyfile_decode_g2_compressed", "k_keyfile_decode_g2_raw", "k_keyfile_subgroup_psi",
           "k_keyfile_subgroup_by_r", "k_keyfile_encode_g1_compressed", "k_keyfile_encode_g1_raw", "k_keyfile_encode_g2_compressed", "k_keyfile_encode_g2_raw"]


def kernel_table():
    """compiled resources of keyfile.hip's kernels, in source order (needs hipcc, no GPU)"""
    import kernel_resources as KR
    rows = KR.kernels_of(os.path.join(KR.CSRC, "keyfile.hip"))
    out = []
    for r in rows:
        name = next((k for k in sorted(KERNELS, key=len, reverse=True) if k in r["symbol"]), r["symbol"])
        alloc = (r["vgpr"] + 7) // 8 * 8
        out.append(f"kernel {name} vgpr+agpr={r['vgpr']} (agpr {r['agpr']}) sgpr={r['sgpr']} scratch_bytes={r['scratch']} lds={r['lds_static']} "
                   f"waves_per_simd={min(8, 512 // alloc)}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("log_n", type=int)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--write", default=None, help="append the result lines to this file")
    ap.add_argument("--kernels-only", action="store_true", help="print the resource table alone (it compiles keyfile.hip; no GPU needed)")
    ap.add_argument("--no-kernels", action="store_true", help="leave the resource table out (no compile on the GPU machine)")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    if not a.kernels_only:
        B = load_binding()
        ctx = B.Context(0)
        try:
            N = 1 << a.log_n
            r1cs = S.synth_r1cs(N - 100, nb_wires=N - 1000, nb_public=4097, seed=2300 + a.log_n, per_row=3, n_coeffs=1 << 12, n_heavy=64, commitments=1,
                                n_committed=N >> 5)
            td = S.synth_trapdoor(a.log_n, n_sigma=1)
            removed = sorted(int(x) for ws, cw in r1cs["commitments"] for x in list(ws) + [cw])
            blobs = {}
            for enc, label in ((B.KEYFILE_COMPRESSED, "compressed"), (B.KEYFILE_RAW, "raw")):
                try:
                    ctx.setup_to_stream(r1cs, td, enc, cap=0, build=False)
                except B.MiError:
                    pass
                cap = ctx.keyfile_len
                runs = []
                for _ in range(a.repeats + 1):
                    blobs[enc] = ctx.setup_to_stream(r1cs, td, enc, cap=cap, build=False)[0]
                    runs.append(ctx.keyfile_stats())
                med = {k: statistics.median(r[k] for r in runs[1:]) for k in runs[0]}
                say(f"write log_n={a.log_n} {label} bytes={len(blobs[enc])} encode_ms={med['decode_ms']:.2f} copy_to_host_ms={med['upload_ms']:.1f} total_ms={med['total_ms']:.1f}")
            clocks = ClockSampler(0).start()

            def timed(label, call):
                runs = []
                for _ in range(a.repeats + 1):
                    t0 = time.perf_counter()
                    pkh, peds = call()
                    ctx.sync()
                    wall = (time.perf_counter() - t0) * 1e3
                    st = dict(ctx.keyfile_stats(), wall_ms=wall)
                    for pd in peds:
                        ctx.pedersen_pk_free(pd)
                    ctx.pk_free(pkh)
                    runs.append(st)
                med = {k: statistics.median(r[k] for r in runs[1:]) for k in runs[0]}
                spread = max(r["wall_ms"] for r in runs[1:]) - min(r["wall_ms"] for r in runs[1:])
                return med, spread
            med, spread = timed("baseline", lambda: ctx.pk_load_raw(blobs[B.KEYFILE_RAW], r1cs["nb_public"], removed))
            say(f"baseline log_n={a.log_n} mi_pk_load_raw raw_stream wall_ms={med['wall_ms']:.1f} spread_ms={spread:.1f} (no curve check, no membership test)")
            subgroup = {}
            for label, enc, flags in (("raw+checks", B.KEYFILE_RAW, 0), ("compressed+checks", B.KEYFILE_COMPRESSED, 0),
                                      ("compressed,no_membership_test", B.KEYFILE_COMPRESSED, B.KEYFILE_NO_SUBGROUP_CHECK),
                                      ("compressed+checks_by_r", B.KEYFILE_COMPRESSED, B.KEYFILE_SUBGROUP_BY_R)):
                med, spread = timed(label, lambda: ctx.pk_load_stream(blobs[enc], r1cs["nb_public"], removed, flags))
                subgroup[label] = med["subgroup_ms"]
                say(f"load log_n={a.log_n} mi_pk_load_stream {label} wall_ms={med['wall_ms']:.1f} spread_ms={spread:.1f} upload_ms={med['upload_ms']:.1f} "
                    f"decode_ms={med['decode_ms']:.1f} subgroup_ms={med['subgroup_ms']:.1f} build_ms={med['build_ms']:.1f}")
            info, _ = B.pk_stream_inspect(blobs[B.KEYFILE_COMPRESSED])
            say(f"member log_n={a.log_n} g2_points={info.n_g2_b + 2} psi_ms={subgroup['compressed+checks']:.2f} by_r_ms={subgroup['compressed+checks_by_r']:.2f} "
                f"(k_keyfile_subgroup_psi against k_keyfile_subgroup_by_r over the same decoded points, host clock to the synchronise)")
            ck = clocks.stop()
            say(f"clocks {ck}" if ck else "clocks not readable on this machine")
        finally:
            ctx.close()
    for row in ([] if a.no_kernels else kernel_table()):
        say(row)
    if a.write:
        with open(a.write, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Times groth16.Setup on the device (mi_groth16_setup, csrc/setup.hip) against what a caller could do before it existed.

    python tools/setup_probe.py LOG_N [--skip-baseline] [--write profiles/r07_setup.txt]

Prints, for a seeded synthetic R1CS of the benchmark's shape (2^LOG_N - 100 constraints, 2^LOG_N - 1000 wires, three entries per live
row and matrix, one BSB22 commitment over N / 32 wires; tests/setup_cases.py):

  setup     mi_groth16_setup, second run (the first warms the context's workspaces up): total wall time and the device time of every
            phase from HIP events on the context's stream (mi_groth16_setup_get_stats)
  baseline  the same key without the new entry point: the exponents on the host with the oracle's vector arithmetic (cref.field_op,
            OpenMP, 16 threads where the machine has them), then mi_batch_scalar_mul_g1/g2_dev and mi_pk_load_dev.  Never gnark: it cannot be
            built here, and CPU figures of this project are never gnark's
  sparse    the transposed sparse product alone (mi_groth16_setup_exponents' sort + sum phases) on the two skew extremes of the tests --
            one wire in every row of A, wire 0 in half the rows of B, 200 wires of 2^10 entries, against uniformly random columns -- with
            its byte floor: entries x (4 + 4 + 32 gathered) bytes over the 6.3 TB/s a streaming kernel reaches on this part
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
from helpers import fr_arr  # noqa: E402
from gpu_common import load_binding  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
ADD, SUB, MUL = 0, 1, 2


def host_columns(r1cs, name, L):
    """M_j for every wire on the host, vectorised: the products in column order, columns of up to 64 entries summed rank by rank (entries
    of one rank have distinct columns), longer ones by a pairwise tree each"""
    rp, col, cf = r1cs[name]
    nw = r1cs["nb_wires"]
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp).astype(np.int64))
    prod = D._op(MUL, r1cs["coeffs"][cf], L[rows])
    order = np.argsort(col, kind="stable")
    cs, prod = col[order], prod[order]
    cnt = np.bincount(cs, minlength=nw)
    start = np.concatenate([[0], np.cumsum(cnt)])
    out = np.zeros((nw, 4), np.uint64)
    rank = np.arange(len(cs)) - start[cs]
    long_cols = np.nonzero(cnt > 64)[0]
    short = cnt[cs] <= 64
    for r in range(int(cnt[cnt <= 64].max(initial=0))):
        m = short & (rank == r)
        out[cs[m]] = D._op(ADD, out[cs[m]], prod[m])
    for j in long_cols:
        out[j] = D.fr_sum(prod[start[j]:start[j + 1]])
    return out


def host_exponents(r1cs, td):
    nw = r1cs["nb_wires"]
    L, dom = S.lagrange_rows(r1cs["n_constraints"], td["tau"])
    A, B, C = (host_columns(r1cs, n, L) for n in "ABC")
    t = D._op(ADD, D._op(ADD, D._op(MUL, A, D._bc(td["beta"], nw)), D._op(MUL, B, D._bc(td["alpha"], nw))), C)
    inv = lambda x: fr_arr([P.fr_inv(D._int(x))])[0]
    K, Kg = D._op(MUL, t, D._bc(inv(td["delta"]), nw)), D._op(MUL, t, D._bc(inv(td["gamma"]), nw))
    return {"a": A, "b": B, "c": C, "k": K, "k_gamma": Kg, "infinity_a": (~A.any(axis=1)).astype(np.uint8),
            "infinity_b": (~B.any(axis=1)).astype(np.uint8)}, dom.log_n


def baseline(ctx, r1cs, td):
    t0 = time.perf_counter()
    ex, log_n = host_exponents(r1cs, td)
    e = S.dlog_exps(r1cs, td, ex, log_n)
    scal, _ = D._key_scalars(e)
    committed = r1cs["commitments"][0][0]
    scal["basis"] = ex["k_gamma"][committed]
    scal["basis_sigma"] = D._op(MUL, scal["basis"], D._bc(td["sigma"][0], len(committed)))
    t_host = time.perf_counter() - t0
    t0 = time.perf_counter()
    arrays, bufs = {}, []
    for name, sc in scal.items():
        g2 = name == "g2_b"
        ds = ctx.to_dev(sc)
        out = ctx.alloc(max((128 if g2 else 64) * sc.shape[0], 32))
        ctx.batch_scalar_mul_dev(D.G2 if g2 else D.G1, ds.ptr, sc.shape[0], out.ptr, g2=g2)
        ctx.sync()
        ds.free()
        arrays[name] = (out.ptr, sc.shape[0]); bufs.append(out)
    pk = D._pk_dict(e, {k: v for k, v in arrays.items() if not k.startswith("basis")})
    pkh = ctx.pk_load(pk, device_points=True)
    ctx.sync()
    t_dev = time.perf_counter() - t0
    ctx.pk_free(pkh)
    for b in bufs:
        b.free()
    return t_host, t_dev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("log_n", type=int)
    ap.add_argument("--skip-baseline", action="store_true")
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
        r1cs = S.synth_r1cs(N - 100, nb_wires=N - 1000, nb_public=4097, seed=2300 + a.log_n, per_row=3, n_coeffs=1 << 12, n_heavy=64,
                            commitments=1, n_committed=N >> 5)
        td = S.synth_trapdoor(a.log_n, n_sigma=1)
        for run in ("warm-up", "timed"):
            t0 = time.perf_counter()
            pkh, peds, _ = ctx.setup(r1cs, td)
            wall = time.perf_counter() - t0
            st = ctx.setup_stats()
            plan = ctx.pk_table_plan(pkh)
            ctx.pk_free(pkh); ctx.pedersen_pk_free(peds[0])
        fr_half = st["lagrange_ms"] + st["sparse_ms"] + st["elementwise_ms"]
        say(f"setup log_n={a.log_n} entries={st['entries']} wall_ms={wall * 1e3:.1f} total_ms={st['total_ms']:.1f} upload_ms={st['upload_ms']:.1f} "
            f"lagrange_ms={st['lagrange_ms']:.2f} sparse_ms={st['sparse_ms']:.2f} (sort {st['sparse_sort_ms']:.2f} + sum {st['sparse_sum_ms']:.2f}) "
            f"elementwise_ms={st['elementwise_ms']:.2f} points_ms={st['points_ms']:.1f} handover_ms={st['handover_ms']:.1f} "
            f"fr_half_ms={fr_half:.2f} long_columns={st['long_columns']} chunks={st['chunks']} table_plan={plan}")
        if not a.skip_baseline:
            t_host, t_dev = baseline(ctx, r1cs, td)
            say(f"baseline log_n={a.log_n} host_exponents_s={t_host:.1f} ({cref.num_threads()} threads) upload_scalar_mul_pk_load_dev_s={t_dev:.2f} "
                f"total_s={t_host + t_dev:.1f}")
        ctx.trim()
        n = N - 1234
        for label, kw in (("skewed", dict(skew=True, n_heavy=200)), ("uniform", dict(skew=False, n_heavy=0))):
            rs = S.synth_r1cs(n, nb_wires=N + 777, nb_public=33, seed=7, per_row=4, n_coeffs=1 << 16, **kw)
            for _ in range(2):
                ctx.setup_exponents(rs, td, want=())
                st = ctx.setup_stats()
            floor_ms = st["entries"] * 40 / HBM_BYTES_PER_S * 1e3
            say(f"sparse log_n={a.log_n} {label} entries={st['entries']} sort_ms={st['sparse_sort_ms']:.3f} sum_ms={st['sparse_sum_ms']:.3f} "
                f"sparse_ms={st['sparse_ms']:.3f} byte_floor_ms={floor_ms:.3f} long_columns={st['long_columns']} chunks={st['chunks']}")
    finally:
        ctx.close()
    if a.write:
        with open(a.write, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

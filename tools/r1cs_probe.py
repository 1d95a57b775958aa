"""Measures the device-resident R1CS (include/mi355x_groth16_r1cs.h, csrc/r1cs.hip) against the entry points that take a, b from the host.

    python tools/r1cs_probe.py LOG_N [--pairs 5] [--jobs 12] [--eval-only] [--write profiles/r1cs_prove.txt]

On the benchmark-shaped synthetic R1CS (2^LOG_N - 100 constraints, 2^LOG_N - 1000 wires, three entries per live row and matrix, one BSB22
commitment over N / 32 wires; tests/setup_cases.py), one key from mi_groth16_setup, after a warm-up of every path:

  eval      A W + B W alone (mi_r1cs_eval_dev, device time from mi_r1cs_get_stats): entries per second and the byte floor, entries x 40 B
            (8 B entry + 32 B gathered) plus the outputs over the 8 TB/s HBM peak bench.py's roofline uses.  --eval-only stops here (the
            form to run under a kernel trace)
  latency   one proof from host memory: mi_groth16_prove_w(W) against mi_groth16_prove(W, a, b, NULL), alternating, every pair
  pool      three in flight, host inputs, --jobs proofs per batch: mi_prover_submit_w_bsb22 against mi_prover_submit_bsb22, alternating
            batches, every pair
The comparison is always against the existing entry point in the same process on the same key; medians and the spread (min .. max) of
each side are printed beside the pairs, and the PCIe bytes per proof of each path.
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
import cref  # noqa: E402
import dlog_keys as D  # noqa: E402
import setup_cases as S  # noqa: E402
import r1cs_cases as RC  # noqa: E402
from gpu_common import load_binding  # noqa: E402

HBM_PEAK_BYTES_PER_S = 8.0e12


def med(x):
    return float(np.median(x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("log_n", type=int)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--jobs", type=int, default=12)
    ap.add_argument("--eval-only", action="store_true")
    ap.add_argument("--write", default=None, help="append the result lines to this file")
    a = ap.parse_args()
    B = load_binding()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    N = 1 << a.log_n
    r1cs = S.synth_r1cs(N - 100, nb_wires=N - 1000, nb_public=4097, seed=2300 + a.log_n, per_row=3, n_coeffs=1 << 12, n_heavy=64,
                        commitments=1, n_committed=N >> 5)
    nc, nw = r1cs["n_constraints"], r1cs["nb_wires"]
    W = cref.gen_scalars(nw, 31, 1); W[0] = D.ONE
    pool = B.Prover(0, 3)
    try:
        c0 = pool.ctx(0)
        rh = c0.r1cs_load(r1cs)
        dW = c0.to_dev(W); da = c0.alloc(32 * nc + 32); db = c0.alloc(32 * nc + 32)
        ms = []
        for _ in range(2 + a.pairs):
            c0._ck(c0.lib.mi_r1cs_eval_dev(c0.h, rh, B._p(dW.ptr), B.R1CS_A | B.R1CS_B, B._p(da.ptr), B._p(db.ptr), None))
            c0.sync()
            st = c0.r1cs_stats()
            ms.append(st["eval_ms"])
        ms = ms[2:]
        floor_ms = (st["entries"] * 40 + 2 * nc * 32) / HBM_PEAK_BYTES_PER_S * 1e3
        say(f"eval log_n={a.log_n} A+B entries={st['entries']} long_rows={st['long_rows']} pieces={st['pieces']} eval_ms={[round(x, 3) for x in ms]} "
            f"median_ms={med(ms):.3f} entries_per_s={st['entries'] / (med(ms) * 1e-3):.3e} byte_floor_ms={floor_ms:.3f} floor_frac={floor_ms / med(ms):.2f} "
            f"resident_GB={c0.r1cs_bytes(rh) / 1e9:.3f}")
        if a.eval_only:
            return
        av, bv = da.download((nc, 4)), db.download((nc, 4))      # a = A W, b = B W for the existing entry points (checked by the tests)
        td = S.synth_trapdoor(a.log_n, n_sigma=1)
        pkh, peds, _ = c0.setup(r1cs, td)
        r, s = cref.gen_scalars(2, 51, 0)
        ch = cref.gen_scalars(1, 52, 0)[0]
        vals = np.ascontiguousarray(W[r1cs["commitments"][0][0]])
        say(f"bytes log_n={a.log_n} pcie_per_proof: existing (W, a, b) {(nw + 2 * nc) * 32 / 1e6:.1f} MB, from W {nw * 32 / 1e6:.1f} MB (+ {vals.nbytes / 1e6:.1f} MB committed values on both)")
        # ---- one proof from host memory, on a context of its own
        ctx = B.Context(0)
        try:
            def old():
                t0 = time.perf_counter(); p, _ = ctx.prove(pkh, W, av, bv, None, r, s); return (time.perf_counter() - t0) * 1e3, p
            def new():
                t0 = time.perf_counter(); p, _ = ctx.prove_w(pkh, rh, W, r, s); return (time.perf_counter() - t0) * 1e3, p
            for _ in range(2):
                _, p_old = old(); _, p_new = new()
            assert np.array_equal(p_old["raw"], p_new["raw"])
            pairs = [(old()[0], new()[0]) for _ in range(a.pairs)]
            o, n_ = [x for x, _ in pairs], [y for _, y in pairs]
            say(f"latency log_n={a.log_n} ms (prove(W,a,b), prove_w(W)) pairs={[(round(x, 2), round(y, 2)) for x, y in pairs]} "
                f"median {med(o):.2f} vs {med(n_):.2f}; spread {min(o):.2f}..{max(o):.2f} vs {min(n_):.2f}..{max(n_):.2f}; eval inside prove_w {ctx.r1cs_stats()['eval_ms']:.3f} ms")
        finally:
            ctx.close()
        # ---- the pool, three in flight
        def batch(fn):
            t0 = time.perf_counter()
            res = [pool.wait(t) for t in [fn() for _ in range(a.jobs)]]
            return a.jobs / (time.perf_counter() - t0), res
        f_old = lambda: pool.submit_bsb22(pkh, W, av, bv, None, r, s, [(peds[0], vals)], ch)
        f_new = lambda: pool.submit_w_bsb22(pkh, rh, W, r, s, [(peds[0], vals)], ch)
        _, r_old = batch(f_old); _, r_new = batch(f_new)
        assert np.array_equal(r_old[-1][0]["raw"], r_new[-1][0]["raw"]) and np.array_equal(r_old[-1][0]["pok"], r_new[-1][0]["pok"])
        pairs = [(batch(f_old)[0], batch(f_new)[0]) for _ in range(a.pairs)]
        o, n_ = [x for x, _ in pairs], [y for _, y in pairs]
        h_old, h_new = med([st["h2d_ms"] for _, st in r_old]), med([st["h2d_ms"] for _, st in r_new])
        say(f"pool log_n={a.log_n} in_flight=3 jobs={a.jobs} proofs/s (submit_bsb22, submit_w_bsb22) pairs={[(round(x, 2), round(y, 2)) for x, y in pairs]} "
            f"median {med(o):.2f} vs {med(n_):.2f}; spread {min(o):.2f}..{max(o):.2f} vs {min(n_):.2f}..{max(n_):.2f}; upload stage per job {h_old:.1f} vs {h_new:.1f} ms")
        c0.pedersen_pk_free(peds[0]); c0.pk_free(pkh)
        for d in (dW, da, db):
            d.free()
        c0.r1cs_free(rh)
    finally:
        pool.close()
        if a.write:
            with open(a.write, "a") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

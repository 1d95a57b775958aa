"""bench.py --gpus N launched PLAINLY (no torch.distributed.run) must start its N rank processes itself -- children of a process
that never touches the GPU -- and relay rank 0's one JSON line (the driver's multi-GPU command may have exactly the
shape of its 1-GPU command).  --launch-check stops every rank after the rendezvous (gloo, no GPU), so this runs on CPU."""
import json
import os
import subprocess
import sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", [2, 3, 8])
def test_plain_launch_starts_its_ranks_and_prints_one_line(n):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--launch-check"], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, out.stdout
    j = json.loads(lines[0])
    assert j == {"launch_check": True, "world": n, "sum_of_ranks": float(n * (n - 1) // 2)}


def test_more_ranks_than_distinct_gpus_is_refused_with_a_message_unless_it_is_the_declared_rehearsal():
    """`--gpus N` means N ranks on N distinct devices.  A node with fewer GPUs (this container has none; a one-GPU box has
    one) refuses a plain `--gpus 2` with that message and a non-zero status BEFORE any rank starts; the one-GPU rehearsal has to be asked for
    by name (and then fails later here, for want of any GPU -- with the 'no CPU path' message, not the device-count one)."""
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("two GPUs present")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    bench = os.path.join(ROOT, "bench.py")
    r = subprocess.run([sys.executable, bench, "--gpus", "2", "--steps", "1", "--warmup", "0"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode != 0 and "distinct_devices != n_gpus" in r.stderr and "--rehearse-on-one-gpu" in r.stderr
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")], "no JSON line may come out of a refused run"
    if torch.cuda.device_count() == 0:
        r = subprocess.run([sys.executable, bench, "--gpus", "2", "--rehearse-on-one-gpu", "--steps", "1", "--warmup", "0", "--sharded-msm-log-n", "0", "--sharded-prove-log-n", "0"],
                           capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode != 0 and "distinct_devices" not in r.stderr


def test_launcher_given_ranks_are_used_as_they_are():
    """under torch.distributed.run (WORLD_SIZE set) bench.py must NOT start ranks of its own"""
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29517")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--launch-check"], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    assert json.loads(out.stdout.strip().splitlines()[-1])["world"] == 1
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--launch-check"], capture_output=True, text=True, timeout=300, env=env)
    assert bad.returncode != 0 and "WORLD_SIZE=1" in bad.stderr


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_for_tests", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


def test_kernel_names_of_the_counter_passes_are_folded_like_the_committed_summaries():
    b = _bench_module()
    assert b._kernel_short("void k_msm_accum_affine29<4, 3>(Affine<Fe<FpParams> > const*, unsigned int const*)") == "k_msm_accum_affine29"
    assert b._kernel_short("void k_msm_accum_affine_g2_29<1>(Affine<Fp2> const*)") == "k_msm_accum_affine_g2_29"
    assert b._kernel_short("void k_msm2_partition<20u>(Msm2Shape, Fe<FrParams> const*)") == "k_msm2_partition<20u>"
    assert b._kernel_short("k_ntt_pass_wave(Fe<FrParams>*, Fe<FrParams> const*, NttPass, NttTables)") == "k_ntt_pass_wave"


@pytest.mark.gpu
def test_live_counter_pass_sees_the_level1_launch():
    """bench.py's `roofline.traffic` is measured by the run itself: a child `rocprofv3 --pmc FETCH_SIZE` over tools/solo_z_msm.py (small here)"""
    if "rocprof" in os.environ.get("LD_PRELOAD", "") or any(k.startswith(("ROCPROF", "ROCP_")) for k in os.environ):
        pytest.skip("this process already runs under a profiler: profilers are not nested")
    b = _bench_module()
    r = b.live_pmc("solo_z_msm.py", [16, 1], ("FETCH_SIZE",), timeout_s=300)
    assert "error" not in r, r
    k = r["FETCH_SIZE"]["k_msm_accum_affine29"]
    # the fixed-base launch gathers one 64-B point per addition: at least the scalars' 32 B per pair reach the kernel (KB units)
    assert k["launches"] == 2 and k["per_launch"] * 1024.0 > 32.0 * ((1 << 16) - 1)


def test_clock_sampler_reads_rocm_smi_csv(monkeypatch):
    """bench.py's ClockSampler: one sample per rocm-smi answer (csv header + one row), nothing on garbage or a missing tool"""
    b = _bench_module()
    import subprocess as sp
    good = ("device,fclk clock speed:,fclk clock level:,mclk clock speed:,mclk clock level:,sclk clock speed:,sclk clock level:,socclk clock speed:,socclk clock level:,"
            "Current Socket Graphics Package Power (W)\ncard0,(1250Mhz),0,(2000Mhz),0,(2177Mhz),1,(1200Mhz),0,1284.0\n")
    answers = [good, "", "no such tool", good.replace("2177", "2201").replace("1284.0", "1300.0")]

    class R:
        def __init__(self, out): self.stdout = out

    def fake_run(cmd, **kw):
        assert cmd[:3] == ["rocm-smi", "-d", "0"]
        if not answers:
            raise FileNotFoundError("rocm-smi")
        return R(answers.pop(0))
    monkeypatch.setattr(sp, "run", fake_run)
    s = b.ClockSampler(0)
    for _ in range(5):
        s._once()
    assert s.samples == [(2177, 1284.0), (2201, 1300.0)]
    s._stop.set(); s._th.start()
    r = s.stop()
    assert r["samples"] == 2 and r["sclk_mhz_min"] == 2177 and r["sclk_mhz_max"] == 2201 and abs(r["package_power_w_mean"] - 1292.0) < 1e-9


def _load_dump(d):
    """bench.py --dump-outputs DIR back to integers: {name: uint64 limbs (elements, 4)}, plus the proof bytes"""
    import numpy as np
    got = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d) if f.endswith(".npy")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 << 20
    out = {k: (a[..., 0].astype(np.uint64) | (a[..., 1].astype(np.uint64) << np.uint64(32))) for k, a in got.items() if k != "proof_bytes"}
    return out, bytes(got["proof_bytes"].astype(np.uint8))


def test_dump_outputs_hold_the_proof_exactly(tmp_path):
    """--dump-outputs writes float64 files from which the caller's proof (points, commitment, PoK) and its bytes come back bit for bit:
    the golden toy proof, alone (164 bytes) and with one BSB22 commitment (196 bytes), re-serialised by the oracle"""
    import numpy as np
    import cref
    b = _bench_module()
    z = np.load(os.path.join(ROOT, "tests", "golden", "prove_toy1000.npz"))
    raw = np.concatenate([z["ar"], z["bs"], z["krs"]])
    basis, sigma = cref.gen_g1(300, 5), cref.gen_g1(300, 6)
    vals = cref.gen_scalars(300, 7, 1); ch = cref.gen_scalars(1, 8, 0)[0]
    cm = cref.pedersen_msm(basis, vals)
    pok = cref.pedersen_fold(cref.pedersen_msm(sigma, vals).reshape(1, 8), ch)
    cases = (({"ar": z["ar"], "bs": z["bs"], "krs": z["krs"]}, cref.proof_write(raw), ["proof_ar", "proof_bs", "proof_krs", "proof_bytes"]),
             ({"ar": z["ar"], "bs": z["bs"], "krs": z["krs"], "commitment": cm, "pok": pok}, cref.proof_write(raw, cm.reshape(1, 8), pok),
              ["proof_ar", "proof_bs", "proof_krs", "proof_commitment", "proof_pok", "proof_bytes"]))
    for i, (proof, pb, names) in enumerate(cases):
        d = str(tmp_path / f"case{i}")
        assert b.dump_outputs(d, proof, pb) == sorted(names)
        got, got_bytes = _load_dump(d)
        assert got_bytes == pb and len(pb) == (164 if i == 0 else 196)
        assert got["proof_ar"].shape == (2, 4) and got["proof_bs"].shape == (4, 4) and got["proof_krs"].shape == (2, 4)
        for k in proof:
            assert np.array_equal(got["proof_" + k].reshape(-1), np.asarray(proof[k], dtype=np.uint64).reshape(-1)), k
        back = np.concatenate([got["proof_ar"].reshape(-1), got["proof_bs"].reshape(-1), got["proof_krs"].reshape(-1)])
        if i == 0:
            assert cref.proof_write(back) == pb
        else:
            assert cref.proof_write(back, got["proof_commitment"].reshape(1, 8), got["proof_pok"].reshape(-1)) == pb


def test_steps_below_one_are_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0", "--launch-check"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--steps must be at least 1" in r.stderr


# what only a --full run measures and puts in the line
FULL_ONLY_KEYS = ("value_hbm_resident_inputs", "single_proof_latency_ms", "single_proof_latency_host_inputs_ms", "sharded_msm", "sharded_prove",
                  "hbm_ledger_gb", "g1_msm_solo", "g1_msm_z_shaped_solo", "roofline", "roofline_ntt", "random_gather", "valu", "sensitivity", "cpu_baseline")


def test_sharded_legs_are_refused_in_a_plain_run():
    """the sharded legs belong to --full: a plain run that asks for one is refused before anything starts, a --full run takes it"""
    bench = os.path.join(ROOT, "bench.py")
    for opt in ("--sharded-msm-log-n", "--sharded-prove-log-n"):
        r = subprocess.run([sys.executable, bench, opt, "22", "--launch-check"], capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and f"{opt} runs a leg of --full" in r.stderr
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29518")
    for extra in (["--full", "--sharded-msm-log-n", "22"], ["--sharded-msm-log-n", "0", "--sharded-prove-log-n", "0"]):
        r = subprocess.run([sys.executable, bench, "--gpus", "1", "--launch-check"] + extra, capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stderr[-2000:]


@pytest.mark.gpu
def test_plain_run_skips_and_full_run_runs_every_leg_on_a_small_key(rank_launcher):
    """bench.py on a small key.  A plain run reports the timed steps and nothing of --full.  With --full every leg after the timed steps
    runs and reports -- the HBM-resident region, the latencies, the sensitivity legs, the solo kernels, the counter passes, the sharded
    legs (helper process) and the CPU baseline, whose 196 proof bytes must equal the GPU's.  (Both started by the rank launcher: a
    process that never touched the GPU.)"""
    argv = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--log-n", "14", "--steps", "2", "--warmup", "1"]
    lines = []
    for extra in ([], ["--full", "--sharded-msm-log-n", "16", "--sharded-prove-log-n", "16"]):
        (r,) = rank_launcher.run(argv + extra, 1, timeout=900)
        assert r["rc"] == 0, r["stderr"]
        lines.append(json.loads([ln for ln in r["stdout"].splitlines() if ln.startswith("{")][-1]))
    plain, line = lines
    assert plain["full"] is False and plain["steps"] == 2 and plain["proof_bytes"] == 196 and plain["value"] > 0
    assert not set(FULL_ONLY_KEYS) & set(plain), "a plain run ran legs of --full"
    assert plain["proofs_validated"] == "2 timed proofs (196 bytes each) + 0 HBM-resident-input proofs byte-equal to the untimed reference proofs"
    assert line["full"] is True and line["steps"] == 2 and line["proof_bytes"] == 196
    missing = [k for k in FULL_ONLY_KEYS if k not in line]
    assert not missing, missing
    assert line["hbm_ledger_gb"] and line["g1_msm_solo"]["msm_pts_per_s"] > 0 and line["single_proof_latency_host_inputs_ms"] > 0
    assert line["cpu_baseline"]["proof_bytes_match"] and line["cpu_baseline"]["proof_bytes_compared"] == 196
    assert line["value_hbm_resident_inputs"] > 0 and line["proofs_validated"] == "2 timed proofs (196 bytes each) + 2 HBM-resident-input proofs byte-equal to the untimed reference proofs"
    assert {"half_uniform", "uniform", "census"} <= set(line["sensitivity"]) and line["value_census_mix"] > 0
    assert line["sharded_msm"].get("done") and line["sharded_prove"].get("done") and line["sharded_prove"]["equals_unsharded_prove"], (line["sharded_msm"], line["sharded_prove"])
    assert line["roofline_ntt"]["compute_h_solo_ms"] > 0 and line["random_gather"]["ceiling_gathers_per_s"] > 0 and line["valu"]["modmul_ceiling_per_s"] > 0


@pytest.mark.gpu
def test_dump_outputs_are_the_timed_proof_and_repeat_from_run_to_run(tmp_path):
    """bench.py --dump-outputs on a small key: the files hold the 196-byte proof of the last timed step (re-serialised through the
    library's own WriteTo), and two runs with a different number of timed steps dump identical outputs (seeded inputs)"""
    import numpy as np
    from gpu_common import load_binding
    B = load_binding()
    small = ["--log-n", "14", "--warmup", "1", "--no-cpu-baseline", "--no-sensitivity", "--no-solo-legs", "--no-live-pmc", "--no-hbm-resident",
             "--no-clock-samples", "--sharded-msm-log-n", "0", "--sharded-prove-log-n", "0"]
    dumps = []
    for steps in (2, 3):
        d = str(tmp_path / f"steps{steps}")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--dump-outputs", d] + small,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert line["steps"] == steps and line["proofs_validated"].startswith(f"{steps} timed proofs") and line["proof_bytes"] == 196
        dumps.append(_load_dump(d))
    (got, pb), (got2, pb2) = dumps
    assert len(pb) == 196 and pb == pb2 and got.keys() == got2.keys()
    assert all(np.array_equal(got[k], got2[k]) for k in got)
    raw = np.concatenate([got["proof_ar"].reshape(-1), got["proof_bs"].reshape(-1), got["proof_krs"].reshape(-1)])
    assert B.proof_write(raw, got["proof_commitment"].reshape(1, 8), got["proof_pok"].reshape(-1)) == pb

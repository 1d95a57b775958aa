"""Times groth16.Verify on the device (mi_groth16_verify[_batch], csrc/verify.hip) and, beside each of its legs, the same proofs from
their bytes (mi_groth16_verify_bytes[_batch], csrc/verify_bytes.hip): the difference of the two is the cost of decoding and hashing.
Beside each batch leg, the same inputs through mi_groth16_verify_combined (csrc/verify_combined.hip: one verdict for the batch, under a
fixed seed), in the same process: the two calls ALTERNATE, one pair per run, and each gets its median and its min .. max.
Beside each batch leg, a locate leg (mi_groth16_verify_locate, csrc/verify_locate.hip: one verdict per proof by descent): the batch with
b = 0, 1 and 8 proofs tampered (another Krs) at seeded positions through the locate, the combined and the per-proof call, the three
ALTERNATING, with the locate call's stats; then, for the larger batches with b = 1 and 8, the locate call under node budgets of 8, 64 and
512 per round (mi_debug_set_locate_round_nodes): the column the default MI_LOCATE_ROUND_NODES is read from.

    python tools/verify_probe.py [--write profiles/verify.txt] [--batches 64,1024,16384] [--runs 5]
    python tools/verify_probe.py --files [--write profiles/verify.txt]      the files leg alone (files_leg below); --write APPENDS
    python tools/verify_probe.py --wave [--write profiles/verify.txt]       the wave leg alone (wave_leg below); --write APPENDS
    python tools/verify_probe.py --ksum [--write profiles/verify.txt]       the ksum leg alone (ksum_leg below); --write APPENDS

A solvable circuit of 1000 constraints (domain 2^10, 4 public inputs, one BSB22 commitment; tests/r1cs_cases.py), its key from
mi_groth16_setup, one proof through the prover pool.  After a warm-up call, the median wall time of `--runs` calls of one verification
and of batches of the given sizes (the same proof repeated: the arithmetic does not depend on the data).  The times are those of the
whole call, host part included (the G1 checks, one synchronous MSM per proof for kSum, the folds): the library has no per-phase device
timers for Verify yet.  There is no baseline: no CPU pairing exists in this repository and gnark cannot be built here, so no rate is
claimed -- the figures are recorded, nothing more."""
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
import r1cs_cases as RC  # noqa: E402
import bytes_cases as BC  # noqa: E402
from helpers import fr_arr, fr_vals, g1_pts  # noqa: E402
from gpu_common import load_binding  # noqa: E402


def files_leg(B, args):
    """--files: the public inputs as witness bytes (mi_groth16_verify_files_combined, include/mi355x_groth16_vkfile.h) against Montgomery
    words prepared on the host, on a key with 4096 public inputs (SURVEY 8d's count) and one commitment.  The key is made of seeded
    points, not of a circuit, and the proof is five valid points: the verdict is 1 in every leg (asserted equal) and the work is that of
    an accepted batch -- the arithmetic does not depend on the data.  Per batch, medians of `--runs` calls after one warm-up, the calls
    ALTERNATING:
      (a) verify_bytes_combined, the Montgomery inputs prepared beforehand     (b) (a) + the host time of mi_public_witness_read over the batch
      (c) verify_files_combined on the same proofs and the witnesses' bytes
    and, in a group of its own after them (back to back, so that no host-only leg sits in front of a launch), k_witness_decode alone
    over the batch's values through mi_debug_witness_decode_dev, in launches of at most 1024 witnesses;
    then mi_vk_load_stream (compressed, all checks) against mi_vk_load on the same key.  With --write the lines are APPENDED."""
    import pyref as P
    from helpers import g1_arr, g2_arr
    from benchlib.clocks import ClockSampler
    C = B.C
    ctx = B.Context(0)
    n_pub, nc = 4096, 1
    rnd = np.random.default_rng(4096)
    k = cref.gen_g1(n_pub + 1 + nc, 21)
    g2 = lambda e: g2_arr([P.g2_mul(P.G2_GEN, e)])[0]
    vk = {"alpha1": cref.gen_g1(1, 22)[0], "beta1": cref.gen_g1(1, 23)[0], "delta1": cref.gen_g1(1, 24)[0], "beta2": g2(2), "gamma2": g2(3), "delta2": g2(5), "k": k}
    ped = np.stack([np.stack([g2(1), g2(7)])])
    vkh = ctx.vk_load(vk, n_pub + 1, ped)
    vkh.set_public_committed([[]])
    pts = cref.gen_g1(4, 25)
    data = B.proof_write(np.concatenate([pts[0], g2(11), pts[1]]), commitments=np.ascontiguousarray(pts[2]).reshape(1, 8), pok=np.ascontiguousarray(pts[3]))
    pub_ints = [int.from_bytes(rnd.bytes(31), "big") for _ in range(n_pub)]
    pub = fr_arr(pub_ints)
    wit = B.public_witness_write(pub)
    seed = bytes(range(32))
    lines = [f"verify from files (tools/verify_probe.py --files): {n_pub} public inputs, {nc} commitment, a key of seeded points and a proof of valid points",
             f"(verdict 1 in every leg; the work is an accepted batch's); median (min .. max) ms of {args.runs} calls after one warm-up, the legs (a), read, (c) alternating, the kernel timed apart; host clocks"]
    print("\n".join(lines), flush=True)

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    def timed_group(fns):
        for fn in fns:
            fn()
        ts = [[] for _ in fns]
        for _ in range(args.runs):
            for fn, t_ in zip(fns, ts):
                t = time.perf_counter(); fn(); t_.append((time.perf_counter() - t) * 1e3)
        return [(statistics.median(t_), min(t_), max(t_)) for t_ in ts]

    clocks = ClockSampler(0).start()
    pbuf = C.create_string_buffer(data, len(data)); wbuf = C.create_string_buffer(wit, len(wit))
    for nb in [int(x) for x in args.batches.split(",") if x]:
        barr = (B.VerifyBytesInput * nb)(); farr = (B.VerifyFilesInput * nb)()
        for i in range(nb):
            barr[i].proof, barr[i].proof_len, barr[i].public_inputs = C.addressof(pbuf), len(data), pub.ctypes.data
            farr[i].proof, farr[i].proof_len, farr[i].witness, farr[i].witness_len = C.addressof(pbuf), len(data), C.addressof(wbuf), len(wit)
        va, vc = C.c_uint8(255), C.c_uint8(255)
        out = np.zeros((n_pub, 4), np.uint64); got = C.c_size_t()
        lib = ctx.lib
        acall = lambda: ctx._ck(lib.mi_groth16_verify_bytes_combined(ctx.h, vkh.h, barr, C.c_size_t(nb), seed, C.byref(va), None))
        ccall = lambda: ctx._ck(lib.mi_groth16_verify_files_combined(ctx.h, vkh.h, farr, C.c_size_t(nb), seed, C.byref(vc), None))

        def hcall():   # what a caller of (a) does first: every witness of the batch through the host reader
            for _ in range(nb):
                assert lib.mi_public_witness_read(wbuf, C.c_size_t(len(wit)), out.ctypes.data_as(C.c_void_p), C.c_size_t(n_pub), C.byref(got)) == 0
        din = ctx.to_dev(np.frombuffer(wit[12:] * min(nb, 1024), np.uint8)); dout = ctx.alloc(32 * n_pub * min(nb, 1024)); dbad = ctx.to_dev(np.zeros(max(nb, 32), np.uint8))
        reps = (nb + 1023) // 1024   # the debug entry over at most 1024 witnesses at a time: the same lanes, in `reps` launches

        def kcall():
            for _ in range(reps):
                ctx._ck(lib.mi_debug_witness_decode_dev(ctx.h, C.c_void_p(din.ptr), C.c_size_t(min(nb, 1024)), C.c_uint32(n_pub), C.c_void_p(dout.ptr), C.c_void_p(dbad.ptr)))
            ctx.sync()
        (a, alo, ahi), (h, hlo, hhi), (c, clo, chi) = timed_group([acall, hcall, ccall])
        ((kms, klo, khi),) = timed_group([kcall])   # apart from the alternation: behind seconds of host-only work the device has idled
        assert va.value == vc.value == B.VERIFY_PAIRING and np.array_equal(out, pub)
        for b in (din, dout, dbad):
            b.free()
        emit(f"batch of {nb:6d}   (a) bytes_combined {a:10.3f} ({alo:.3f} .. {ahi:.3f})   host witness_read {h:10.3f} ({hlo:.3f} .. {hhi:.3f})   (b) = (a) + read {a + h:10.3f}")
        emit(f"                  (c) files_combined {c:10.3f} ({clo:.3f} .. {chi:.3f})   (c) / (b) {c / (a + h):6.3f}   (c) / (a) {c / a:6.3f}   "
             f"k_witness_decode alone {kms:8.3f} ({klo:.3f} .. {khi:.3f}), {100 * kms / c:5.2f} % of (c)")
    # the key: from its compressed stream, every check on, against mi_vk_load over the same points
    blob = ctx.vk_write(vk, n_pub + 1, ped, [[]], B.KEYFILE_COMPRESSED)
    (ls, llo, lhi), (lp, plo, phi) = timed_group([lambda: ctx.vk_load_stream(blob).free(), lambda: ctx.vk_load(vk, n_pub + 1, ped).free()])
    emit(f"key of {n_pub + 1 + nc} K points   mi_vk_load_stream (compressed, {len(blob)} bytes, all checks) {ls:9.3f} ({llo:.3f} .. {lhi:.3f})   "
         f"mi_vk_load over the points {lp:9.3f} ({plo:.3f} .. {phi:.3f})")
    emit(f"clocks {clocks.stop()}")
    emit("NOT MEASURED: kernel times by a profiler (every figure is a host clock around a call that ends in a device synchronise), other public-input "
         "counts, any figure from gnark")
    if args.write:
        with open(args.write, "a") as f:
            f.write("\n" + "\n".join(lines) + "\n")
    vkh.free(); ctx.close()


def wave_leg(B, ctx, vkh, inp, args, header):
    """--wave: mi_groth16_verify_wave (csrc/verify_wave.hip: one wave per pairing) against the parent's mi_groth16_verify_batch on the
    probe's key and proof, n = 1, 8, 64, 512, 4096 (--wave-batches): the two calls ALTERNATE in this process on this context, one
    warm-up pair and then max(--runs, 5) pairs, whole calls with their host part.  Per leg the median and the spread (max - min).  The
    yardstick is the parent's call in the same run: the wave call counts as faster at an n only where its median is below the
    parent's by more than the larger of the two spreads.  At n = 1 also the phase split of the wave call
    (mi_debug_verify_wave_split), the median of each phase over the same number of calls.  With --write the lines are APPENDED."""
    C = B.C
    runs = max(args.runs, 5)
    lines = [f"verify, one wave per pairing (tools/verify_probe.py --wave): {header}",
             f"mi_groth16_verify_batch (the parent's call) and mi_groth16_verify_wave alternating on one context, {runs} pairs after one warm-up pair, whole calls, host clocks;",
             "median ms (spread = max - min); 'faster' only where the wave median is below the batch median by more than the larger spread"]
    print("\n".join(lines), flush=True)

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    lead = None
    for nb in [int(x) for x in args.wave_batches.split(",") if x]:
        arr, keep = vkh._inputs([inp] * nb)
        out_b, out_w = np.full(nb, 255, np.uint8), np.full(nb, 255, np.uint8)
        bcall = lambda: ctx._ck(ctx.lib.mi_groth16_verify_batch(ctx.h, vkh.h, arr, C.c_size_t(nb), out_b.ctypes.data_as(C.c_void_p)))
        wcall = lambda: ctx._ck(ctx.lib.mi_groth16_verify_wave(ctx.h, vkh.h, arr, C.c_size_t(nb), out_w.ctypes.data_as(C.c_void_p)))
        bcall(); wcall()
        tb, tw = [], []
        for _ in range(runs):
            for fn, ts in ((bcall, tb), (wcall, tw)):
                t = time.perf_counter(); fn(); ts.append((time.perf_counter() - t) * 1e3)
        assert not out_b.any() and not out_w.any()
        mb, mw, sb, sw = statistics.median(tb), statistics.median(tw), max(tb) - min(tb), max(tw) - min(tw)
        verdict = "wave faster" if mb - mw > max(sb, sw) else ("batch faster" if mw - mb > max(sb, sw) else "no difference beyond the spread")
        if verdict == "batch faster" and lead is None:
            lead = nb
        emit(f"n = {nb:5d}   batch {mb:10.3f} ms (spread {sb:.3f}, {100 * sb / mb:.1f} %)   wave {mw:10.3f} ms (spread {sw:.3f}, {100 * sw / mw:.1f} %)   "
             f"batch / wave {mb / mw:6.2f}   {verdict}")
        if nb == 1:
            splits = []
            for _ in range(runs + 1):
                v, ms = vkh.verify_wave_split([inp])
                assert not v.any()
                splits.append(ms)
            med = {k: statistics.median(x[k] for x in splits[1:]) for k in B.VERIFY_WAVE_SPLIT_PHASES}
            emit("            phase split of the wave call at n = 1, ms (host stage with the MSM call by the wall clock, the rest by events on the stream; "
                 "the Bs check and the Miller loops as two launches here, one launch in the product call):")
            emit("            " + "   ".join(f"{k} {med[k]:.3f}" for k in B.VERIFY_WAVE_SPLIT_PHASES) + f"   sum {sum(med.values()):.3f}")
    emit(f"the batch call takes the lead at n = {lead}" if lead else "the batch call takes the lead at none of these n")
    emit("NOT MEASURED: kernel times by a profiler, sizes between these, other keys (more pairs per proof), any CPU verifier (none exists here)")
    if args.write:
        with open(args.write, "a") as f:
            f.write("\n" + "\n".join(lines) + "\n")


def ksum_key_4096(B, ctx):
    """the key of the --files leg: 4096 public inputs and one commitment, seeded points; byte-valued public inputs and a proof of valid
    points (verdict 1 under either stage: the work is an accepted batch's)"""
    import pyref as P
    from helpers import g2_arr
    n_pub = 4096
    g2 = lambda e: g2_arr([P.g2_mul(P.G2_GEN, e)])[0]
    vk = {"alpha1": cref.gen_g1(1, 22)[0], "beta2": g2(2), "gamma2": g2(3), "delta2": g2(5), "k": cref.gen_g1(n_pub + 2, 21)}
    vkh = ctx.vk_load(vk, n_pub + 1, np.stack([np.stack([g2(1), g2(7)])]))
    pts = cref.gen_g1(4, 25)
    rnd = np.random.default_rng(4096)
    inp = {"raw": np.concatenate([pts[0], g2(11), pts[1]]), "public_inputs": fr_arr([int(x) for x in rnd.integers(0, 256, n_pub)]),
           "commitments": np.ascontiguousarray(pts[2]).reshape(1, 8), "pok": np.ascontiguousarray(pts[3]), "commitment_values": cref.gen_scalars(1, 26, 0)}
    return vkh, inp


def ksum_leg(B, ctx, legs, args):
    """--ksum: the stage of the verdict-per-proof bodies through the key's window table (knob "verify_ksum" = 1; csrc/ksum.hip) against
    the older stage, one MSM per proof from the host (knob 0), on the SAME context: mi_groth16_verify_batch and mi_groth16_verify_wave at
    n = 1, 8, 64, 512, 4096, 16384 (--ksum-batches), for each body one warm-up pair (knob 1, knob 0) and then max(--runs, 5) pairs,
    whole calls with their host part.  legs: (header, key, proof, table budget, expected verdict).  Per leg the table's build time and
    bytes, then per size and body the medians and spreads (max - min).  The yardstick is knob 0 in the same run: knob 1 counts as
    faster only where its median is below knob 0's by more than the larger of the two spreads.  With --write the lines are APPENDED."""
    C = B.C
    runs = max(args.runs, 5)
    lines = ["kSum of a whole batch over the key's window table (tools/verify_probe.py --ksum): the knob \"verify_ksum\" at 1 (table) and 0 (one MSM per proof,",
             f"the yardstick) alternating on one context, {runs} pairs after one warm-up pair, whole calls, host clocks; median ms (spread = max - min);",
             "'faster' only where the knob-1 median is below the knob-0 median by more than the larger spread; the knob \"verify_ksum_min_batch\" is at 1 here,",
             "so knob 1 is the table at EVERY size (the library's default keeps the older stage below 8 proofs: the pairs at n = 1 and n = 8 are why)"]
    print("\n".join(lines), flush=True)
    ctx.set_knob("verify_ksum_min_batch", 1)

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    bodies = (("batch", ctx.lib.mi_groth16_verify_batch), ("wave ", ctx.lib.mi_groth16_verify_wave))
    for header, vkh, inp, budget, verdict in legs:
        info = vkh.ksum_prepare(budget)
        emit(f"--- {header}")
        emit(f"    table: budget {info['budget_bytes']} bytes -> c = {info['window_bits']}, {info['windows']} windows, {info['bases']} bases, "
             f"{info['table_bytes']} bytes ({info['table_bytes'] / 2**20:.1f} MiB), built in {info['build_ms']:.3f} ms (wall clock, with its synchronisation)")
        assert info["state"] == B.KSUM_READY
        not_faster = []
        for nb in [int(x) for x in args.ksum_batches.split(",") if x]:
            arr, keep = vkh._inputs([inp] * nb)
            for name, f in bodies:
                outs = {1: np.full(nb, 255, np.uint8), 0: np.full(nb, 255, np.uint8)}

                def call(knob):
                    ctx.set_knob("verify_ksum", knob)
                    t = time.perf_counter()
                    ctx._ck(f(ctx.h, vkh.h, arr, C.c_size_t(nb), outs[knob].ctypes.data_as(C.c_void_p)))
                    return (time.perf_counter() - t) * 1e3
                call(1); call(0)
                ts = {1: [], 0: []}
                for _ in range(runs):
                    for knob in (1, 0):
                        ts[knob].append(call(knob))
                ctx.set_knob("verify_ksum", 1)
                assert (outs[1] == verdict).all() and (outs[0] == verdict).all()
                m1, m0, s1, s0 = statistics.median(ts[1]), statistics.median(ts[0]), max(ts[1]) - min(ts[1]), max(ts[0]) - min(ts[0])
                word = "knob 1 faster" if m0 - m1 > max(s0, s1) else ("knob 0 faster" if m1 - m0 > max(s0, s1) else "no difference beyond the spread")
                if word != "knob 1 faster":
                    not_faster.append((name.strip(), nb))
                emit(f"    n = {nb:5d}  {name}  knob 1 {m1:10.3f} ms (spread {s1:.3f})   knob 0 {m0:10.3f} ms (spread {s0:.3f})   knob 0 / knob 1 {m0 / m1:7.2f}   "
                     f"{m1 / nb:8.4f} against {m0 / nb:8.4f} ms per proof   {word}")
        emit("    knob 1 faster at every size, both bodies" if not not_faster else f"    knob 1 NOT faster at: {not_faster}")
    emit("NOT MEASURED: kernel times by a profiler, sizes between these, other public-input counts and widths than the ones stated, the bytes and files calls "
         "(they run the batch body's stage), any figure from gnark")
    if args.write:
        with open(args.write, "a") as f:
            f.write("\n" + "\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ksum", action="store_true", help="the ksum leg alone (see ksum_leg); --write appends")
    ap.add_argument("--ksum-batches", default="1,8,64,512,4096,16384")
    ap.add_argument("--wave", action="store_true", help="the wave leg alone (see wave_leg); --write appends")
    ap.add_argument("--wave-batches", default="1,8,64,512,4096")
    ap.add_argument("--files", action="store_true", help="the files leg alone (see files_leg); --write appends")
    ap.add_argument("--write")
    ap.add_argument("--batches", default="64,1024,16384")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--combined-only", action="store_true", help="the batch legs time the combined call alone: for a kernel trace of it")
    ap.add_argument("--locate-only", action="store_true", help="the batch legs time one locate call with one tampered proof alone: for a kernel trace of it")
    ap.add_argument("--no-locate", action="store_true", help="skip the locate legs")
    args = ap.parse_args()
    B = load_binding()
    if args.files:
        return files_leg(B, args)
    ctx = B.Context(0)
    n, nab, nb_public = 1000, 400, 5
    r1cs = RC.skewed_r1cs(n, nab, nb_public, 11, long_lens=(16, 17, 64), commitments=1, n_committed=32)
    r1cs["nb_wires"] = nab + n
    r1cs["C"] = (np.arange(n + 1, dtype=np.uint64), (nab + np.arange(n)).astype(np.uint32), np.ones(n, np.uint32))
    W = np.zeros((r1cs["nb_wires"], 4), np.uint64)
    W[:nab] = RC.witness(nab, 12)
    a, b = RC.eval_rows(r1cs, "A", W), RC.eval_rows(r1cs, "B", W)
    W[nab:] = D._op(2, a, b)
    td = S.synth_trapdoor(13, n_sigma=1)
    r, s = cref.gen_scalars(2, 14, 0)
    pkh, peds, vk = ctx.setup(r1cs, td)
    vals = np.ascontiguousarray(W[r1cs["commitments"][0][0]])
    pool = B.Prover(0, 1)
    try:
        cm = pool.commit(peds[0], vals).reshape(1, 8)
        # the bytes leg hashes: the commitment wire's value IS the hash of the commitment, the challenge the hash of that value
        # (tests/bytes_cases.py states both in Python), written into W before the rest of the witness is solved
        values, fold = BC.bsb22_hashes(g1_pts(cm), fr_vals(W[1:nb_public]))
        W[r1cs["commitments"][0][1]] = fr_arr(values)[0]
        ch = fr_arr([fold])[0]
        a, b = RC.eval_rows(r1cs, "A", W), RC.eval_rows(r1cs, "B", W)
        W[nab:] = D._op(2, a, b)
        proof, _ = pool.wait(pool.submit_bsb22(pkh, W, a, b, None, r, s, [(peds[0], vals)], ch))
    finally:
        pool.close()
    vkh = ctx.vk_load(vk, nb_public, ctx.pedersen_vk_make(np.stack(td["sigma"])))
    inp = {"raw": proof["raw"], "public_inputs": np.ascontiguousarray(W[1:nb_public]), "commitments": cm,
           "pok": np.ascontiguousarray(proof["pok"]).reshape(8), "fold_challenge": ch,
           "commitment_values": np.ascontiguousarray(W[[r1cs["commitments"][0][1]]])}
    assert vkh.verify(inp) == B.VERIFY_OK
    data = B.proof_write(inp["raw"], commitments=cm, pok=inp["pok"])
    assert vkh.verify_bytes(data, inp["public_inputs"]) == B.VERIFY_OK
    if args.ksum:
        vkh_files, inp_files = ksum_key_4096(B, ctx)
        ksum_leg(B, ctx, [(f"1000 constraints (domain 2^10), {nb_public - 1} public inputs with full-width values, 1 commitment (5 pairs per proof); the default budget",
                           vkh, inp, 0, B.VERIFY_OK),
                          ("4096 byte-valued public inputs, 1 commitment (5 pairs per proof), a key of seeded points and a proof of valid points "
                           "(verdict 1 under either knob); a budget of 256 MiB", vkh_files, inp_files, 256 << 20, B.VERIFY_PAIRING)], args)
        vkh_files.free(); vkh.free(); ctx.pedersen_pk_free(peds[0]); ctx.pk_free(pkh); ctx.close()
        return
    if args.wave:
        wave_leg(B, ctx, vkh, inp, args, f"1000 constraints (domain 2^10), {nb_public - 1} public inputs, 1 commitment (5 pairs per proof)")
        vkh.free(); ctx.pedersen_pk_free(peds[0]); ctx.pk_free(pkh); ctx.close()
        return
    lines = [f"groth16.Verify on the device: 1000 constraints (domain 2^10), {nb_public - 1} public inputs, 1 commitment (5 pairs per proof)",
             f"median wall time of {args.runs} calls after one warm-up call, host part included; no baseline exists, no rate is claimed"]

    print("\n".join(lines), flush=True)

    def emit(line):     # as it is measured: a long leg is not silent
        lines.append(line)
        print(line, flush=True)

    def timed(fn):
        fn()
        ts = []
        for _ in range(args.runs):
            t = time.perf_counter(); fn(); ts.append((time.perf_counter() - t) * 1e3)
        return statistics.median(ts)

    def timed_pair(fa, fb):
        """one warm-up call of each, then `runs` pairs (a, b), alternating -> [median, min, max] of each, ms"""
        fa(); fb()
        ta, tb = [], []
        for _ in range(args.runs):
            for fn, ts in ((fa, ta), (fb, tb)):
                t = time.perf_counter(); fn(); ts.append((time.perf_counter() - t) * 1e3)
        return [(statistics.median(ts), min(ts), max(ts)) for ts in (ta, tb)]

    def timed_group(fns):
        """one warm-up call of each, then `runs` rounds through all of them, alternating -> (median, min, max) of each, ms"""
        for fn in fns:
            fn()
        ts = [[] for _ in fns]
        for _ in range(args.runs):
            for fn, t_ in zip(fns, ts):
                t = time.perf_counter(); fn(); t_.append((time.perf_counter() - t) * 1e3)
        return [(statistics.median(t_), min(t_), max(t_)) for t_ in ts]

    other_krs = inp["raw"].copy()
    other_krs[24:32] = cref.gen_g1(1, 77)[0]
    tampered = dict(inp, raw=other_krs)
    assert vkh.verify(tampered) == B.VERIFY_PAIRING
    seed = bytes(range(32))

    def locate_leg(nb):
        """the locate, combined and per-proof calls on the same inputs with b tampered proofs, then the node budgets"""
        stats = B.VerifyLocateStats()
        for b in (0, 1, 8):
            pos = sorted(int(x) for x in np.random.default_rng(1000 + nb + b).choice(nb, b, replace=False))
            proofs = [inp] * nb
            for i in pos:
                proofs[i] = tampered
            arr, keep = vkh._inputs(proofs)
            want = np.zeros(nb, np.uint8); want[pos] = B.VERIFY_PAIRING
            out_l, out_b = np.full(nb, 255, np.uint8), np.full(nb, 255, np.uint8)
            one_v = B.C.c_uint8(255)
            lcall = lambda: ctx._ck(ctx.lib.mi_groth16_verify_locate(ctx.h, vkh.h, arr, B.C.c_size_t(nb), seed, out_l.ctypes.data_as(B.C.c_void_p), B.C.byref(stats)))
            ccall = lambda: ctx._ck(ctx.lib.mi_groth16_verify_combined(ctx.h, vkh.h, arr, B.C.c_size_t(nb), seed, B.C.byref(one_v), None))
            bcall = lambda: ctx._ck(ctx.lib.mi_groth16_verify_batch(ctx.h, vkh.h, arr, B.C.c_size_t(nb), out_b.ctypes.data_as(B.C.c_void_p)))
            if args.locate_only:
                if b == 1:
                    emit(f"batch of {nb:6d}       locate alone, 1 tampered {timed(lcall):10.3f} ms   {stats.as_dict()}")
                continue
            (lms, llo, lhi), (cms, clo, chi), (bms, blo, bhi) = timed_group([lcall, ccall, bcall])
            assert np.array_equal(out_l, want) and np.array_equal(out_b, want) and one_v.value == (B.VERIFY_PAIRING if b else B.VERIFY_OK)
            emit(f"  locate, {b} tampered   locate {lms:10.3f} ms ({llo:.3f} .. {lhi:.3f})   combined {cms:10.3f} ms ({clo:.3f} .. {chi:.3f})   "
                 f"per proof {bms:10.3f} ms ({blo:.3f} .. {bhi:.3f})   locate / combined {lms / cms:6.2f}   per proof / locate {bms / lms:7.1f}")
            emit(f"                        {stats.as_dict()}")
            if nb >= 1024 and b:
                cols = []
                for cap in (8, 64, 512):
                    ctx.set_locate_round_nodes(cap)
                    cols.append((cap, timed(lcall), stats.as_dict()))
                    assert np.array_equal(out_l, want)
                ctx.set_locate_round_nodes(0)
                emit("    node budget per round: " + "   ".join(f"{cap}: {ms:9.3f} ms ({st['rounds']} rounds, {st['nodes_tested']} nodes, {st['judged_alone']} alone)"
                                                               for cap, ms, st in cols))

    one, one_b = timed(lambda: vkh.verify(inp)), timed(lambda: vkh.verify_bytes(data, inp["public_inputs"]))
    emit(f"one verification      {one:10.3f} ms   from bytes {one_b:10.3f} ms   decode + hash {one_b - one:9.3f} ms")
    for nb in [int(x) for x in args.batches.split(",") if x]:
        arr, keep = vkh._inputs([inp] * nb)
        out = np.zeros(nb, np.uint8)
        call = lambda: ctx._ck(ctx.lib.mi_groth16_verify_batch(ctx.h, vkh.h, arr, nb, out.ctypes.data_as(B.C.c_void_p)))
        one_v = B.C.c_uint8(255); first = B.C.c_uint64(0)
        ccall = lambda: ctx._ck(ctx.lib.mi_groth16_verify_combined(ctx.h, vkh.h, arr, B.C.c_size_t(nb), seed, B.C.byref(one_v), B.C.byref(first)))
        if args.combined_only:
            emit(f"batch of {nb:6d}       combined alone {timed(ccall):10.3f} ms")
            continue
        if args.locate_only:
            locate_leg(nb)
            continue
        (ms, lo, hi), (cms, clo, chi) = timed_pair(call, ccall)
        assert not out.any() and (one_v.value, first.value) == (B.VERIFY_OK, nb)
        barr = (B.VerifyBytesInput * nb)()
        buf = B.C.create_string_buffer(data, len(data)); pub = np.ascontiguousarray(inp["public_inputs"], np.uint64)
        for i in range(nb):
            barr[i].proof, barr[i].proof_len, barr[i].public_inputs = B.C.addressof(buf), len(data), pub.ctypes.data
        bcall = lambda: ctx._ck(ctx.lib.mi_groth16_verify_bytes_batch(ctx.h, vkh.h, barr, B.C.c_size_t(nb), out.ctypes.data_as(B.C.c_void_p)))
        bms = timed(bcall)
        assert not out.any()
        emit(f"batch of {nb:6d}       {ms:10.3f} ms   {ms / nb:8.4f} ms per proof   from bytes {bms:10.3f} ms   decode + hash {(bms - ms) / nb:8.4f} ms per proof")
        emit(f"  alternating pairs   per proof {ms:10.3f} ms ({lo:.3f} .. {hi:.3f})   combined {cms:10.3f} ms ({clo:.3f} .. {chi:.3f})   "
                     f"{cms / nb:8.4f} ms per proof   per proof / combined {ms / cms:7.1f}")
        if not args.no_locate:
            locate_leg(nb)
    if args.write:
        with open(args.write, "w") as f:
            f.write("\n".join(lines) + "\n")
    vkh.free(); ctx.pedersen_pk_free(peds[0]); ctx.pk_free(pkh); ctx.close()


if __name__ == "__main__":
    main()

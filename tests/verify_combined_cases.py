"""What tests/test_verify_combined_cpu.py and tests/test_gpu_verify_combined.py share: the host build of the combined batch verifier
(tests/emu/emu_verify_combined.cpp) and the packing of a batch of verify_forge inputs into the arrays it takes."""
import ctypes as C
import os
import subprocess
import numpy as np
import verify_cases as V

HERE = os.path.dirname(os.path.abspath(__file__))


def build_emu(so):
    """compiled like verify_cases.build_emu: every bound of the arithmetic underneath traps"""
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DMI_CHECK_NOWRAP", "-shared", "-fPIC", "-o", so,
                           os.path.join(HERE, "emu", "emu_verify_combined.cpp")])
    return so


def emu_coefficients(emu, seed, n):
    out = np.zeros((n, 2), np.uint64)
    assert emu.emu_combine_coefficients(seed, C.c_size_t(n), V.p_(out)) == 0
    return [int(lo) | int(hi) << 64 for lo, hi in out]


def emu_product(emu, x):
    x = np.ascontiguousarray(x, np.uint64).reshape(-1, 48)
    out = np.zeros(48, np.uint64)
    assert emu.emu_fp12_product(V.p_(x), C.c_size_t(len(x)), V.p_(out)) == 0
    return out


def emu_scale128(emu, pts, ks):
    pts = np.ascontiguousarray(pts, np.uint64).reshape(-1, 8)
    kk = np.array([[k & (1 << 64) - 1, k >> 64] for k in ks], np.uint64).reshape(-1, 2)
    out = np.zeros_like(pts)
    assert emu.emu_g1_scale128(V.p_(pts), V.p_(kk), C.c_size_t(len(pts)), V.p_(out)) == 0
    return out


def emu_verify_combined(emu, vk, inputs, seed):
    """vk: pairing_ref's dict; inputs: what binding.VerifyingKey.verify takes, one dict per proof -> (verdict, first_malformed)"""
    d, nbp, ped = V.vk_arrays(vk)
    nc, n = 0 if ped is None else len(ped), len(inputs)

    def stack(name, shape):
        rows = [np.zeros(shape, np.uint64) if x.get(name) is None else np.asarray(x[name], np.uint64).reshape(shape) for x in inputs]
        return np.ascontiguousarray(np.stack(rows)) if rows and int(np.prod(shape)) else None
    raw, cm, pok = stack("raw", (32,)), stack("commitments", (nc, 8)), stack("pok", (8,)) if nc else None
    pub, cv = stack("public_inputs", (nbp - 1, 4)), stack("commitment_values", (nc, 4))
    fold = stack("fold_challenge", (4,)) if nc > 1 else None
    out = np.zeros(2, np.uint64)
    rc = emu.emu_verify_combined(V.p_(d["k"]), V.p_(d["alpha1"]), V.p_(d["beta2"]), V.p_(d["gamma2"]), V.p_(d["delta2"]), V.p_(ped), C.c_uint(nbp),
                                 C.c_uint(nc), V.p_(raw), V.p_(cm), V.p_(pok), V.p_(pub), V.p_(cv), V.p_(fold), C.c_size_t(n), seed, V.p_(out))
    assert rc == 0
    return int(out[0]), int(out[1])

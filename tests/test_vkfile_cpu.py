"""CPU suite of include/mi355x_groth16_vkfile.h: the host-only inspector of a verifying key's stream in both encodings on streams written
in Python (tests/vkfile_cases.py), the witness codec on the host against Python, the sanitizer build of both readers
(gnark-whir_amd/Makefile `sanitize-vkfile`, its own main, nothing preloaded), the per-value text of k_witness_decode
(gnark-whir_amd/csrc/witness_ops.cuh) in the host build tests/emu/emu_witness.cpp with -DMI_CHECK_NOWRAP, and the committed fixture pair."""
import ctypes as C
import os
import random
import re
import struct
import subprocess
import numpy as np
import pytest
import pyref as P
import verify_cases as V
import vkfile_cases as VK
from helpers import fr_arr
from gpu_common import load_binding, ROOT

r = P.R_MOD
PKG = os.path.join(ROOT, "gnark-whir_amd")
HEADER = os.path.join(ROOT, "include", "mi355x_groth16_vkfile.h")


@pytest.fixture(scope="module")
def streams():
    """{(shape, encoding, with lists): (case, lists, blob)} of the four toy keys"""
    out = {}
    for shape in VK.KEY_SHAPES:
        case, lists = VK.toy_key(*shape)
        for e in (VK.RAW, VK.COMPRESSED):
            for full in (False, True):
                ls = lists if full else [[] for _ in lists]
                out[shape, e, full] = (case, ls, VK.write_vk_stream(case["vk"], case["vk"]["ped"], ls, e))
    return out


# ---------------------------------------------------------------------------------------------------- the ABI
def test_library_exports_every_vkfile_symbol():
    B = load_binding()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", src)))
    assert "mi_vk_load_stream" in names and "mi_groth16_verify_files_locate" in names and "mi_groth16_setup_to_streams" in names
    for n in names:
        assert hasattr(B.load(), n), f"{n} declared in mi355x_groth16_vkfile.h but not exported"
    assert sorted(B.VKFILE_EXPORTS) == names
    assert not set(B.VKFILE_EXPORTS) & (set(B.EXPORTS) | set(B.SETUP_EXPORTS) | set(B.R1CS_EXPORTS) | set(B.VERIFY_EXPORTS) | set(B.VERIFY_BYTES_EXPORTS) |
                                        set(B.VERIFY_COMBINED_EXPORTS) | set(B.VERIFY_LOCATE_EXPORTS) | set(B.KEYFILE_EXPORTS))
    assert hasattr(B.load(), "mi_debug_witness_decode_dev") and "mi_debug_witness_decode_dev" in B.EXPORTS
    assert C.sizeof(B.VkStreamInfo) == 8 + 4 + 4 + 8 * 8 + 3 * 128 + 8 + 96 and C.sizeof(B.VkFileDesc) == 3 * 64 + 3 * 128 + 8 + 8 + 4 + 4 + 3 * 8
    assert C.sizeof(B.VerifyFilesInput) == 32


# ---------------------------------------------------------------------------------------------------- the inspector
@pytest.mark.parametrize("shape", VK.KEY_SHAPES)
@pytest.mark.parametrize("encoding", [VK.RAW, VK.COMPRESSED])
def test_inspect_counts_and_offsets(streams, shape, encoding):
    B = load_binding()
    nb_public, nc = shape
    g1, g2 = (32, 64) if encoding == VK.COMPRESSED else (64, 128)
    for full in (False, True):
        case, lists, blob = streams[shape, encoding, full]
        info, enc = B.vk_stream_inspect(blob)
        assert enc == encoding and info.refused == b""
        assert (info.n_k, info.nb_public, info.n_commitment_keys) == (nb_public + nc, nb_public, nc)
        assert (info.off_alpha1, info.off_beta1, info.off_beta2, info.off_gamma2, info.off_delta1, info.off_delta2) == (0, g1, 2 * g1, 2 * g1 + g2, 2 * g1 + 2 * g2, 3 * g1 + 2 * g2)
        assert info.off_k == 3 * g1 + 3 * g2 + 4 and info.off_lists == info.off_k + g1 * info.n_k
        at = info.off_lists + 4
        for k, l in enumerate(lists):
            assert (info.list_len[k], info.off_list[k]) == (len(l), at + 4)
            assert [int.from_bytes(blob[info.off_list[k] + 8 * t:info.off_list[k] + 8 * t + 8], "big") for t in range(len(l))] == l
            at += 4 + 8 * len(l)
        assert info.off_commitment_keys == at
        assert [info.off_ped[k] for k in range(nc)] == [at + 4 + 2 * g2 * k for k in range(nc)] and at + 4 + 2 * g2 * nc == len(blob)
        assert blob[info.off_k + g1 * (info.n_k - 1):info.off_lists] == VK.K.g1_enc(case["vk"]["k"][-1], encoding)
        assert blob[info.off_gamma2:info.off_delta1] == VK.K.g2_enc(case["vk"]["gamma2"], encoding)
        if nc:
            assert blob[info.off_ped[nc - 1] + g2:] == VK.K.g2_enc(case["vk"]["ped"][nc - 1][1], encoding)
        n_idx = sum(map(len, lists))
        assert B.vk_stream_size(nb_public + nc, nc, n_idx, encoding) == len(blob) == VK.vk_stream_len(nb_public + nc, nc, n_idx, encoding)


def test_stated_sizes():
    """the two sizes include/mi355x_groth16_vkfile.h states, by the library and by the Python helper"""
    B = load_binding()
    assert B.vk_stream_size(4, 1, 0, VK.COMPRESSED) == VK.vk_stream_len(4, 1, 0, VK.COMPRESSED) == 560
    assert B.vk_stream_size(4, 1, 0, VK.RAW) == VK.vk_stream_len(4, 1, 0, VK.RAW) == 1104


@pytest.mark.parametrize("encoding", [VK.RAW, VK.COMPRESSED])
def test_inspect_refusals(streams, encoding):
    B = load_binding()

    def refused(blob, *words):
        with pytest.raises(B.MiError) as e:
            B.vk_stream_inspect(bytes(blob))
        for w in words:
            assert w in str(e.value), (w, str(e.value))

    for shape in ((3, 2), (1, 0)):
        case, lists, blob = streams[shape, encoding, True]
        info, _ = B.vk_stream_inspect(blob)
        for cut in range(len(blob)):                                           # every strict prefix
            refused(blob[:cut])
        refused(blob + b"\x00")                                                # one byte appended
        offs = [info.off_k - 1, info.off_lists + 3, info.off_commitment_keys + 3] + [info.off_list[k] - 1 for k in range(shape[1])]
        for off in offs:                                                       # each count off by one, either way
            for d in (1, -1):
                broken = bytearray(blob); broken[off] = (broken[off] + d) % 256
                refused(broken)
        # the flag bits of G1.Alpha say the other encoding
        broken = bytearray(blob); broken[0] = (broken[0] & 0x3F) | (0x80 if encoding == VK.RAW else 0x00)
        refused(broken, "G1.Alpha")
    case, lists, blob = streams[(3, 2), encoding, True]
    info, _ = B.vk_stream_inspect(blob)
    vk, ped = case["vk"], case["vk"]["ped"]
    refused(VK.write_vk_stream(vk, ped, lists[:1], encoding), "n_lists")      # n_lists != n_commitment_keys
    refused(VK.write_vk_stream(vk, ped, lists + [[]], encoding), "n_lists")
    refused(VK.write_vk_stream(dict(vk, k=vk["k"][:2]), ped, [[], []], encoding), "n_k")   # n_k < 1 + n_commitment_keys
    refused(VK.write_vk_stream(dict(vk, k=vk["k"] * 4), [ped[0]] * 17, [[]] * 17, encoding), "MI_PK_RAW_MAX_COMMITMENTS")
    for bad, k in ((0, 0), (3, 0), (4, 1), (1 << 32, 1), ((1 << 32) + 1, 0), (1 << 63, 1)):   # 0, above the range, not below 2^32
        ls = [list(l) for l in lists]; ls[k][0] = bad
        refused(VK.write_vk_stream(vk, ped, ls, encoding), f"PublicAndCommitmentCommitted[{k}][0]")
    ls = [[1, 2], [3]]                                                          # the highest index of each list is taken
    assert B.vk_stream_inspect(VK.write_vk_stream(vk, ped, ls, encoding))[1] == encoding


# ---------------------------------------------------------------------------------------------------- the witness on the host
@pytest.mark.parametrize("n", [0, 1, 4, 65])
def test_witness_write_and_read_against_python(n):
    B = load_binding()
    rnd = random.Random(n)
    vals = ([0, 1, r - 1] + [rnd.randrange(r) for _ in range(n)])[:n]
    want = VK.write_witness(vals)
    assert len(want) == 12 + 32 * n
    assert B.public_witness_write(fr_arr(vals) if n else np.zeros((0, 4), np.uint64)) == want
    got = B.public_witness_read(want)
    assert got.shape == (n, 4) and (not n or np.array_equal(got, fr_arr(vals)))
    # a full witness: the public part is its first nbPublic values
    full = VK.write_witness(vals, n_secret=3)
    assert len(full) == 12 + 32 * (n + 3)
    got = B.public_witness_read(full)
    assert got.shape == (n, 4) and (not n or np.array_equal(got, fr_arr(vals)))
    # too small a buffer: the size comes back, nothing is written
    with pytest.raises(B.MiError, match=str(12 + 32 * n)):
        B.public_witness_write(fr_arr(vals) if n else np.zeros((0, 4), np.uint64), cap=11 + 32 * n)


def test_witness_read_refusals():
    B = load_binding()
    vals = [5, 6, 7]
    good = VK.write_witness(vals)
    for bad in (good[:-1], good + b"\0", good[:11], b"", good[:12], good + bytes(32),
                struct.pack(">III", 3, 0, 4) + good[12:], struct.pack(">III", 2, 0, 3) + good[12:], struct.pack(">III", 3, 1, 3) + good[12:],
                struct.pack(">III", 0xffffffff, 1, 0) + good[12:]):
        with pytest.raises(B.MiError):
            B.public_witness_read(bad)
    for v in (r, r + 1, (1 << 256) - 1):
        with pytest.raises(B.MiError):
            B.public_witness_read(good[:12 + 32] + v.to_bytes(32, "big") + good[12 + 64:])
        # in the secret part it is not read
        assert B.public_witness_read(struct.pack(">III", 1, 2, 3) + good[12:12 + 32] + v.to_bytes(32, "big") + good[12 + 64:]).shape == (1, 4)
    assert np.array_equal(B.public_witness_read(good[:12 + 32] + (r - 1).to_bytes(32, "big") + good[12 + 64:]), fr_arr([5, r - 1, 7]))
    with pytest.raises(B.MiError):
        B.public_witness_read(good, cap=2)


# ---------------------------------------------------------------------------------------------------- the sanitizer build
def test_mutated_streams_never_trip_a_sanitizer(streams, tmp_path):
    """tests/cpp/vkfile_fuzz.cpp, its own main, -fsanitize=address,undefined on the host: mi_vk_stream_inspect and mi_public_witness_read
    over every truncation and seeded mutants, each in a heap block of exactly its size; its contract checks run inside the program"""
    subprocess.check_call(["make", "-C", PKG, "-s", "sanitize-vkfile"])
    paths = []
    for e in (VK.RAW, VK.COMPRESSED):
        paths.append(str(tmp_path / f"vk_{e}.bin"))
        open(paths[-1], "wb").write(streams[(3, 2), e, True][2])
    paths.append(str(tmp_path / "witness.bin"))
    wit = VK.write_witness([1, r - 1, 12345], n_secret=2)
    open(paths[-1], "wb").write(wit)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:allocator_may_return_null=1", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([os.path.join(PKG, "build", "vkfile_fuzz_asan"), *paths, "40000", "3"], capture_output=True, text=True, env=env, timeout=600)
    assert res.returncode == 0 and not res.stderr.strip(), f"rc {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-6000:]}"
    accepted, refused = (int(x) for x in res.stdout.split()[-2:])
    assert accepted >= 3 and refused >= sum(len(streams[(3, 2), e, True][2]) for e in (VK.RAW, VK.COMPRESSED)) + len(wit)


# ---------------------------------------------------------------------------------------------------- the per-value text
def test_witness_decoder_against_python(tmp_path_factory):
    """0, 1, r - 1, r, r + 1, 2^256 - 1 and 60 seeded values at odd addresses: the words are v 2^256 mod r, zero where v is not below r"""
    emu = C.CDLL(VK.build_emu(str(tmp_path_factory.mktemp("emu") / "libemu_witness.so")))
    rnd = random.Random(8)
    vals = list(VK.WITNESS_EDGES) + [rnd.randrange(1 << 256) for _ in range(30)] + [rnd.randrange(r) for _ in range(30)]
    for shift in (1, 3, 0, 7):
        buf = np.frombuffer(bytes(shift) + b"".join(v.to_bytes(32, "big") for v in vals), np.uint8).copy()
        base = buf.ctypes.data + shift
        out = np.zeros((len(vals), 4), np.uint64); below = np.zeros(len(vals), np.uint8)
        assert emu.emu_witness_decode(C.c_void_p(base), C.c_size_t(len(vals)), V.p_(out), V.p_(below)) == 0
        assert list(below) == [int(v < r) for v in vals]
        assert list(below[:6]) == [1, 1, 1, 0, 0, 0] and 6 < int(below.sum()) < len(vals)
        for v, row in zip(vals, out):
            assert sum(int(w) << (64 * i) for i, w in enumerate(row)) == (VK.mont(v) if v < r else 0), hex(v)


# ---------------------------------------------------------------------------------------------------- the fixture pair
def test_python_writer_reproduces_the_committed_fixtures():
    """tests/golden/vk_toy_c1.*: V.toy_case(1, nb_public=3) as this library's layout has it -- something to diff against gnark's files"""
    B = load_binding()
    case = V.toy_case(1, nb_public=3)
    one, lists = VK.toy_key(3, 1)
    assert one["vk"]["k"] == case["vk"]["k"] and one["public_inputs"] == case["public_inputs"]
    vk_bytes, wit = open(VK.GOLDEN_VK, "rb").read(), open(VK.GOLDEN_WITNESS, "rb").read()
    assert (len(vk_bytes), len(wit)) == (560, 76)
    assert VK.write_vk_stream(one["vk"], one["vk"]["ped"], [[]], VK.COMPRESSED) == vk_bytes
    assert VK.write_witness(case["public_inputs"]) == wit
    info, enc = B.vk_stream_inspect(vk_bytes)
    assert enc == VK.COMPRESSED and (info.n_k, info.nb_public, info.n_commitment_keys, info.list_len[0]) == (4, 3, 1, 0)
    assert np.array_equal(B.public_witness_read(wit), fr_arr(case["public_inputs"]))

"""CPU suite: the library exports every symbol include/mi355x_groth16_phase1.h declares (phase 1 on the device), the binding's list
matches the header, the binding's structures have the sizes the header's have, the header says what it leaves out, and
mi_phase1_records_verify -- host only -- refuses null arguments."""
import ctypes as C
import os
import re
import numpy as np
import pyref as P
from helpers import g1_arr
from gpu_common import load_binding, ROOT

HEADER = os.path.join(ROOT, "include", "mi355x_groth16_phase1.h")


def _declared(path=HEADER):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_phase1_symbol():
    B = load_binding()
    lib = B.load()
    names = _declared()
    for n in ("mi_phase1_init", "mi_phase1_from_srs", "mi_phase1_set_transcript_id", "mi_phase1_contribute", "mi_phase1_contribute_proved",
              "mi_phase1_records_verify", "mi_phase1_verify_adopt", "mi_phase1_check", "mi_phase1_export", "mi_phase1_free", "mi_phase1_get_stats",
              "mi_phase2_init_from_phase1"):
        assert n in names, n
    for n in names:
        assert hasattr(lib, n), f"{n} declared in mi355x_groth16_phase1.h but not exported"
    assert sorted(B.PHASE1_EXPORTS) == names
    assert not set(B.PHASE1_EXPORTS) & (set(B.EXPORTS) | set(B.PHASE2_EXPORTS) | set(B.PHASE2_CHECK_EXPORTS))
    for n in B.PHASE1_EXPORTS:
        assert hasattr(lib, n), n


def test_debug_entry_lives_in_the_debug_header():
    B = load_binding()
    dbg = _declared(os.path.join(ROOT, "include", "mi355x_groth16_debug.h"))
    assert "mi_debug_scale_powers_dev" in dbg and "mi_debug_scale_powers_dev" in B.EXPORTS and hasattr(B.load(), "mi_debug_scale_powers_dev")
    src = open(HEADER).read()
    assert "mi355x_groth16_debug.h" not in src and not [n for n in _declared() if n.startswith(("mi_debug_", "mi_bench_", "mi_gen_"))]
    text = open(os.path.join(ROOT, "include", "mi355x_groth16_debug.h")).read()
    assert '"scale_powers_window"' in text and '"scale_powers_chunk"' in text


def test_phase1_header_and_binding_agree():
    B = load_binding()
    src = open(HEADER).read()
    assert B.PHASE1_RECORD_WORDS * 8 == 3 * 64 + 3 * 64 + 3 * 32 + 32
    assert C.sizeof(B.Phase1Stats) == 9 * 4 + 2 * 4 + 4 + 8 and C.sizeof(B.Phase1Info) == 8 + 8 + 32 + 3 * 64
    for name in ("RECORD", "LINK"):
        assert int(re.search(rf"#define MI_PHASE1_BAD_{name}\s+(\d+)u", src).group(1)) == getattr(B, "PHASE1_BAD_" + name)
    assert not (B.PHASE1_BAD_RECORD | B.PHASE1_BAD_LINK) & (B.SRS_BAD_GENERATORS | B.SRS_BAD_TAU_G1 | B.SRS_BAD_ALPHA_G1 | B.SRS_BAD_BETA_G1 | B.SRS_BAD_TAU_G2
                                                           | B.SRS_BAD_BETA_G2)
    flat = " ".join(src.split())
    for phrase in ("A SEED THE MAKER OF THE DATA CANNOT PREDICT", "THIS PROJECT'S OWN FORMAT", "mi355x-phase1-record", "mi355x-phase1-challenge",
                   "bit for bit as it was", "will not verify for anyone else"):
        assert phrase in flat, phrase


def test_not_done_lists_no_longer_name_phase_1():
    """the three lists of what is left out (README, the two phase-2 headers) do not ask for a phase-1 transcript any more;
    sigma and gnark's formats stay"""
    p2 = " ".join(open(os.path.join(ROOT, "include", "mi355x_groth16_phase2.h")).read().split())
    chk = " ".join(open(os.path.join(ROOT, "include", "mi355x_groth16_phase2_check.h")).read().split())
    not_covered = chk[chk.index("NOT COVERED"):chk.index("#ifndef")]
    assert "a phase-1 transcript:" not in not_covered and "mi355x_groth16_phase1.h" in chk
    assert "BasisExpSigma" in not_covered and "file formats" in not_covered
    assert "mi355x_groth16_phase1.h" in p2 and "mpcsetup file formats" in p2
    for doc in ("README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "mi355x_groth16_phase1.h" in text, doc


def test_records_verify_refuses_null_arguments():
    B = load_binding()
    lib = B.load()
    g = np.repeat(g1_arr([P.G1_GEN]), 3, axis=0)
    h = bytes(32)
    fb = C.c_uint64(77)
    rec = np.zeros((1, B.PHASE1_RECORD_WORDS), np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.mi_phase1_records_verify(None, h, C.c_uint64(0), p(rec), C.c_size_t(1), C.byref(fb)) == -1
    assert lib.mi_phase1_records_verify(p(g), None, C.c_uint64(0), p(rec), C.c_size_t(1), C.byref(fb)) == -1
    assert lib.mi_phase1_records_verify(p(g), h, C.c_uint64(0), None, C.c_size_t(1), C.byref(fb)) == -1
    assert lib.mi_phase1_records_verify(p(g), h, C.c_uint64(0), p(rec), C.c_size_t(1), None) == -1
    assert fb.value == 77
    # the generator three times is a start; no record: all of none hold; a record of zeros holds nothing
    assert B.phase1_records_verify(g, h, 0, rec[:0]) == 0
    assert B.phase1_records_verify(g, h, 0, rec) == 0
    z = g.copy(); z[1] = 0
    assert lib.mi_phase1_records_verify(p(z), h, C.c_uint64(0), None, C.c_size_t(0), C.byref(fb)) == -1   # a start at infinity

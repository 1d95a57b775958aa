"""CPU suite: the library exports every symbol include/mi355x_groth16_keyaudit.h declares (a key audited against its circuit and an SRS),
the binding's list matches the header and overlaps no other list, the mask bits and the structures agree, the header says what the
audit presumes and leaves out, and the entry that exposes the sums lives in the debug header alone."""
import ctypes as C
import os
import re
from gpu_common import load_binding, ROOT

HEADER = os.path.join(ROOT, "include", "mi355x_groth16_keyaudit.h")
DEBUG = os.path.join(ROOT, "include", "mi355x_groth16_debug.h")
BITS = ("SMALL", "A", "B1", "B2", "K_PRIVATE", "K_PUBLIC", "BASIS", "SIGMA", "Z")


def _declared(path=HEADER):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_keyaudit_symbol():
    B = load_binding()
    lib = B.load()
    names = _declared()
    for n in ("mi_key_claim_from_streams", "mi_key_claim_from_phase2", "mi_key_claim_from_arrays", "mi_key_claim_free", "mi_key_audit", "mi_key_audit_get_stats"):
        assert n in names
    for n in names:
        assert hasattr(lib, n), f"{n} declared in mi355x_groth16_keyaudit.h but not exported"
    assert sorted(B.KEYAUDIT_EXPORTS) == names
    others = [getattr(B, n) for n in dir(B) if n.endswith("EXPORTS") and n != "KEYAUDIT_EXPORTS"]
    assert len(others) >= 12
    for lst in others:
        assert not set(B.KEYAUDIT_EXPORTS) & set(lst)


def test_mask_bits_are_distinct_single_bits_and_the_binding_s():
    B = load_binding()
    src = open(HEADER).read()
    seen = 0
    for name in BITS:
        v = int(re.search(rf"#define MI_KEY_BAD_{name}\s+(\d+)u", src).group(1))
        assert v and not v & (v - 1) and not v & seen, name
        seen |= v
        assert v == getattr(B, "KEY_BAD_" + name)
    assert seen == (1 << len(BITS)) - 1


def test_binding_structures_match_the_header_layout():
    B = load_binding()
    assert C.sizeof(B.KeyAuditStats) == 11 * 4 + 4 + 8
    assert C.sizeof(B.KeyAuditSums) == 6 * 2 * 64 + 2 * 128 + 16 * 2 * 64 + 8
    src = open(HEADER).read()
    fields = re.search(r"typedef struct mi_key_audit_stats \{(.*?)\} mi_key_audit_stats;", src, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = re.findall(r"\b([a-z0-9_]+)\s*[,;]", fields)
    assert names == [n for n, _ in B.KeyAuditStats._fields_]


def test_header_says_what_the_audit_presumes_and_leaves_out():
    src = open(HEADER).read()
    assert not [n for n in _declared() if n.startswith(("mi_debug_", "mi_bench_", "mi_gen_"))]
    assert "mi355x_groth16_debug.h" not in src and '#include "mi355x_groth16_phase2_check.h"' in src
    flat = " ".join(src.replace(" * ", " ").split())
    for phrase in ("A SEED THE MAKER OF THE DATA CANNOT PREDICT", "presumes the rows are consistent powers", "NOT COVERED", "who knows delta or sigma",
                   "encodings and mask canonicity", "recalled, not pinned to gnark", "2^-128 per relation", "mi_srs_check_powers or mi_phase1_check",
                   "Every relation is evaluated whatever the others say"):
        assert phrase in flat, phrase


def test_the_sums_are_declared_in_the_debug_header_alone():
    B = load_binding()
    assert "mi_debug_key_audit_sums" in _declared(DEBUG) and hasattr(B.load(), "mi_debug_key_audit_sums")
    inc = os.path.join(ROOT, "include")
    for h in os.listdir(inc):
        if h != "mi355x_groth16_debug.h":
            assert "mi_debug_key_audit_sums" not in _declared(os.path.join(inc, h)), h
    assert "mi_debug_key_audit_sums" not in B.KEYAUDIT_EXPORTS


def test_the_ceremony_headers_point_to_the_audit():
    for h in ("mi355x_groth16_phase2.h", "mi355x_groth16_phase2_check.h"):
        assert "mi355x_groth16_keyaudit.h" in open(os.path.join(ROOT, "include", h)).read(), h

"""ctypes binding of libmi355x_groth16.so (the C-ABI of include/mi355x_groth16.h).

This is plumbing for tests/ and bench.py: it mirrors the C entry points one to one and adds no
compute.  There is NO fallback: if the HIP library is missing or no gfx950 device is present,
load()/Context() raise.  numpy layouts: Fr/Fp (n,4) uint64; G1 affine (n,8); G1 jac (12,);
G2 affine (n,16); G2 jac (24,), all Montgomery little-endian limbs.
"""
from __future__ import annotations
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MI355X_GROTH16_LIB", os.path.join(_HERE, "libmi355x_groth16.so"))   # the override is for A/B runs of two builds
_LIB = None

EXPORTS = [
    "mi_init", "mi_init_prio", "mi_shutdown", "mi_last_error", "mi_set_stream", "mi_pk_load", "mi_pk_load_dev", "mi_pk_free",
    "mi_ntt", "mi_ntt_dev", "mi_compute_h", "mi_compute_h_dev", "mi_msm_g1", "mi_msm_g1_dev", "mi_msm_g2",
    "mi_msm_g2_dev", "mi_groth16_prove", "mi_groth16_prove_dev", "mi_get_stats", "mi_g1_compress",
    "mi_g2_compress", "mi_proof_write", "mi_g1_sum", "mi_g2_sum", "mi_gen_scalars_dev", "mi_gen_g1_dev",
    "mi_gen_g2_dev", "mi_field_op_dev", "mi_debug_limb29_op_dev", "mi_debug_lazy_op_dev", "mi_debug_field_shape_dev", "mi_debug_pairing_dev", "mi_debug_fp12_op_dev", "mi_debug_pairing_wave_dev", "mi_debug_fp12_op_wave_dev", "mi_debug_verify_wave_split", "mi_debug_verify_pairs_dev", "mi_debug_decode_g1_dev", "mi_debug_decode_g2_dev", "mi_debug_hash_to_field_dev", "mi_debug_witness_decode_dev", "mi_debug_fp12_product_dev", "mi_debug_g1_scale128_dev", "mi_debug_g1_sum_tree_dev", "mi_debug_locate_points_dev", "mi_debug_locate_colsums_dev", "mi_debug_set_locate_round_nodes", "mi_g1_add_dev", "mi_g2_add_dev", "mi_bench_modmul_dev", "mi_bench_valu_dev", "mi_bench_gather_dev",
    "mi_dev_alloc", "mi_dev_free", "mi_dev_upload", "mi_dev_download", "mi_dev_sync",
    "mi_msm_precompute_g1_dev", "mi_msm_precompute_g2_dev", "mi_msm_g1_fixed_dev", "mi_msm_g2_fixed_dev", "mi_msm_table_to_rprime_g1_dev", "mi_msm_table_to_rprime_g2_dev", "mi_pk_table_plan",
    "mi_batch_scalar_mul_g1", "mi_batch_scalar_mul_g1_dev", "mi_batch_scalar_mul_g2", "mi_batch_scalar_mul_g2_dev",
    "mi_pedersen_pk_load", "mi_pedersen_pk_free", "mi_pedersen_commit", "mi_pedersen_prove_knowledge", "mi_pedersen_fold",
    "mi_debug_set_prove_fixed_base", "mi_debug_set_prove_schedule", "mi_debug_set_msm_batch_affine", "mi_debug_set_msm_group_bits", "mi_debug_inject_hip_failure", "mi_debug_set_ntt_plan", "mi_debug_set_ntt_threads", "mi_debug_set_ntt_wave_stages",
    "mi_debug_set_msm_plan", "mi_debug_set_msm_chunk", "mi_debug_set_msm_one_pass_sort", "mi_debug_set_msm_bound_levels", "mi_debug_set_msm_limb29", "mi_debug_set_msm_l1_waves", "mi_debug_set_msm_precompute_batched", "mi_debug_set_ntt_fuse_pair", "mi_debug_set_knob", "mi_debug_get_counter", "mi_debug_scale_powers_dev", "mi_debug_set_stream_plan", "mi_debug_set_trace_ranges", "mi_set_trace_ranges",
    "mi_prover_create", "mi_prover_destroy", "mi_prover_in_flight", "mi_prover_ctx", "mi_prover_last_error",
    "mi_prover_submit", "mi_prover_submit_dev", "mi_prover_wait", "mi_prover_commit", "mi_prover_submit_bsb22", "mi_prover_trim", "mi_ctx_trim",
    "mi_group_create", "mi_group_unique_id", "mi_group_create_rank", "mi_group_create_rank_ex", "mi_group_rank", "mi_group_destroy", "mi_group_world", "mi_group_local", "mi_group_ctx",
    "mi_group_last_error", "mi_group_transport", "mi_group_comm_ranks", "mi_group_device_pci", "mi_group_set_lead_share", "mi_group_wire_range", "mi_group_set_sharded_compute_h", "mi_compute_h_sharded_dev", "mi_groth16_prove_sharded_slices_dev", "mi_group_exchange_selftest", "mi_pk_load_sharded", "mi_pk_sharded_free",
    "mi_groth16_prove_sharded", "mi_groth16_prove_sharded_dev", "mi_pk_load_sharded_dev", "mi_msm_g1_sharded", "mi_msm_g2_sharded",
    "mi_msm_g1_sharded_dev", "mi_msm_g2_sharded_dev",
    "mi_pk_raw_inspect", "mi_pk_load_raw",
    "mi_whir_proof_decode", "mi_whir_proof_free", "mi_whir_proof_elements", "mi_whir_proof_statement_values", "mi_whir_element_shape", "mi_whir_parse_paths",
    "mi_whir_reverse", "mi_whir_prefix_decode_path", "mi_whir_limbs_to_fr", "mi_whir_interner_decode", "mi_whir_matrix_cells", "mi_whir_config_parse", "mi_whir_config_free",
]

# include/mi355x_groth16_setup.h (groth16.Setup on the device); kept apart from EXPORTS, which lists the four older headers
SETUP_EXPORTS = ["mi_groth16_setup", "mi_groth16_setup_exponents", "mi_groth16_setup_get_stats"]
MAX_COMMITMENTS = 16   # MI_PK_RAW_MAX_COMMITMENTS
# include/mi355x_groth16_r1cs.h (the device-resident R1CS and the entry points that prove from W alone)
R1CS_EXPORTS = ["mi_r1cs_load", "mi_r1cs_free", "mi_r1cs_bytes", "mi_r1cs_eval", "mi_r1cs_eval_dev", "mi_r1cs_check_dev", "mi_r1cs_get_stats",
                "mi_groth16_prove_w", "mi_groth16_prove_w_dev", "mi_prover_submit_w", "mi_prover_submit_w_dev", "mi_prover_submit_w_bsb22"]
R1CS_A, R1CS_B, R1CS_C = 1, 2, 4
PROVE_W_EVAL_C = 1
# include/mi355x_groth16_verify.h (groth16.Verify on the device)
VERIFY_EXPORTS = ["mi_vk_load", "mi_vk_free", "mi_pedersen_vk_make", "mi_groth16_verify", "mi_groth16_verify_batch"]
VERIFY_OK, VERIFY_PAIRING, VERIFY_PEDERSEN, VERIFY_MALFORMED = 0, 1, 2, 3
PAIRING_FINAL_EXP = 1
# include/mi355x_groth16_verify_bytes.h (groth16.Verify from a proof's bytes: decode and hash on the device)
VERIFY_BYTES_EXPORTS = ["mi_vk_set_public_committed", "mi_groth16_verify_bytes", "mi_groth16_verify_bytes_batch", "mi_proof_read", "mi_hash_to_field"]
# include/mi355x_groth16_verify_combined.h (one verdict for a batch: the random linear combination of the proofs' equations)
VERIFY_COMBINED_EXPORTS = ["mi_groth16_verify_combined", "mi_groth16_verify_bytes_combined"]
# include/mi355x_groth16_verify_locate.h (one verdict per proof: the combined test on a tree of subsets, descending into the ones that fail)
VERIFY_LOCATE_EXPORTS = ["mi_groth16_verify_locate", "mi_groth16_verify_bytes_locate"]
# include/mi355x_groth16_verify_wave.h (one proof, or a few: one wave per pairing, the verdicts of the batch calls)
VERIFY_WAVE_EXPORTS = ["mi_groth16_verify_wave", "mi_groth16_verify_bytes_wave"]
# include/mi355x_groth16_verify_ksum.h (the public-input sums of a whole batch over a window table of the key's bases)
VERIFY_KSUM_EXPORTS = ["mi_vk_ksum_prepare", "mi_vk_ksum_get_info", "mi_vk_ksum_batch_dev", "mi_vk_ksum_batch"]
KSUM_NOT_BUILT, KSUM_READY, KSUM_OVER_BUDGET, KSUM_NO_MEMORY, KSUM_NO_BASES = 0, 1, 2, 3, 4
KSUM_DEFAULT_TABLE_BYTES = 64 << 20
VERIFY_WAVE_SPLIT_PHASES = ("host", "bs_check", "miller", "judge", "copy_back")   # mi_debug_verify_wave_split, ms
# include/mi355x_groth16_keyfile.h (proving keys as files: bulk point codecs, loading gnark's raw or compressed stream, writing both)
KEYFILE_EXPORTS = ["mi_g1_decompress_dev", "mi_g2_decompress_dev", "mi_g1_compress_dev", "mi_g2_compress_dev", "mi_pk_stream_inspect", "mi_pk_load_stream",
                   "mi_keyfile_get_stats", "mi_pk_stream_size", "mi_pk_write_dev", "mi_groth16_setup_to_stream"]
KEYFILE_RAW, KEYFILE_COMPRESSED = 0, 1
KEYFILE_NO_SUBGROUP_CHECK, KEYFILE_SUBGROUP_BY_R = 1, 2
NO_BAD_INDEX = (1 << 64) - 1
# include/mi355x_groth16_vkfile.h (verify from files: the verifying key's stream and the public witness's bytes, decoded on the device)
VKFILE_EXPORTS = ["mi_vk_stream_inspect", "mi_vk_stream_size", "mi_vk_write", "mi_vk_load_stream", "mi_groth16_setup_to_streams",
                  "mi_public_witness_write", "mi_public_witness_read", "mi_groth16_verify_files", "mi_groth16_verify_files_batch",
                  "mi_groth16_verify_files_combined", "mi_groth16_verify_files_locate"]
# include/mi355x_groth16_phase2.h (the keys from a powers-of-tau SRS: gnark's mpcsetup phase 2 on the device)
PHASE2_EXPORTS = ["mi_phase2_init", "mi_phase2_contribute", "mi_phase2_seal", "mi_phase2_to_streams", "mi_phase2_free", "mi_phase2_get_stats",
                  "mi_phase2_get_array"]
PHASE2_G1_A, PHASE2_G1_B, PHASE2_G2_B, PHASE2_G1_K, PHASE2_G1_Z, PHASE2_VK_K, PHASE2_BASIS = 0, 1, 2, 3, 4, 5, 6
# include/mi355x_groth16_phase2_check.h (the SRS rows are consistent powers, contributions with a proof of knowledge, a claimed state verified)
PHASE2_CHECK_EXPORTS = ["mi_srs_check_powers", "mi_srs_check_get_stats", "mi_phase2_set_transcript_id", "mi_phase2_contribute_proved",
                        "mi_phase2_records_verify", "mi_phase2_verify_adopt", "mi_phase2_verify_get_stats", "mi_phase2_get_pedersen_vk",
                        "mi_phase2_contribute_sigma_proved", "mi_phase2_sigma_records_verify", "mi_phase2_get_chain_info", "mi_phase2_verify_adopt_sigma"]
SRS_BAD_GENERATORS, SRS_BAD_TAU_G1, SRS_BAD_ALPHA_G1, SRS_BAD_BETA_G1, SRS_BAD_TAU_G2, SRS_BAD_BETA_G2 = 1, 2, 4, 8, 16, 32
PHASE2_BAD_RECORD, PHASE2_BAD_DELTA, PHASE2_BAD_Z, PHASE2_BAD_K = 1, 2, 4, 8
PHASE2_BAD_SIGMA_RECORD, PHASE2_BAD_SIGMA_LINK, PHASE2_BAD_BES = 16, 32, 64
# include/mi355x_groth16_phase1.h (the powers-of-tau SRS itself: a phase-1 ceremony on the device and its handover to phase 2)
PHASE1_EXPORTS = ["mi_phase1_init", "mi_phase1_from_srs", "mi_phase1_set_transcript_id", "mi_phase1_contribute", "mi_phase1_contribute_proved",
                  "mi_phase1_records_verify", "mi_phase1_verify_adopt", "mi_phase1_check", "mi_phase1_get_info", "mi_phase1_export", "mi_phase1_free",
                  "mi_phase1_get_stats", "mi_phase2_init_from_phase1"]
PHASE1_BAD_RECORD, PHASE1_BAD_LINK = 64, 128
# include/mi355x_groth16_keyaudit.h (a key audited against its circuit and an SRS without deriving it again)
KEYAUDIT_EXPORTS = ["mi_key_claim_from_streams", "mi_key_claim_from_phase2", "mi_key_claim_from_arrays", "mi_key_claim_free", "mi_key_audit",
                    "mi_key_audit_get_stats"]
(KEY_BAD_SMALL, KEY_BAD_A, KEY_BAD_B1, KEY_BAD_B2, KEY_BAD_K_PRIVATE, KEY_BAD_K_PUBLIC, KEY_BAD_BASIS, KEY_BAD_SIGMA,
 KEY_BAD_Z) = 1, 2, 4, 8, 16, 32, 64, 128, 256
PHASE1_RECORD_WORDS = 64   # a mi_phase1_record as uint64 words: tau1, alpha1, beta1 (8 each), commit[3] (24), response[3] (12), hash (4)
PHASE2_SIGMA_PROOF_WORDS = 36   # a mi_phase2_sigma_proof as uint64 words: g_sigma_neg (16), commit (16), response (4)
PHASE2_RECORD_WORDS = 24   # a mi_phase2_record as uint64 words: delta1 (8), commit (8), response (4), hash (4 words = 32 bytes)


class PkDesc(C.Structure):
    _fields_ = [
        ("log_n", C.c_uint32), ("nb_public", C.c_uint32), ("nb_wires", C.c_uint64),
        ("g1_a", C.c_void_p), ("n_g1_a", C.c_uint64), ("g1_b", C.c_void_p), ("n_g1_b", C.c_uint64),
        ("g1_k", C.c_void_p), ("n_g1_k", C.c_uint64), ("g1_z", C.c_void_p), ("n_g1_z", C.c_uint64),
        ("g2_b", C.c_void_p), ("n_g2_b", C.c_uint64),
        ("alpha1", C.c_uint64 * 8), ("beta1", C.c_uint64 * 8), ("delta1", C.c_uint64 * 8),
        ("beta2", C.c_uint64 * 16), ("delta2", C.c_uint64 * 16),
        ("infinity_a", C.c_void_p), ("infinity_b", C.c_void_p),
        ("committed_wires", C.c_void_p), ("n_committed", C.c_uint64),
    ]


class MemLedger(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("key_bases", "key_tables", "key_indices", "ctx_ntt_tables", "ctx_ntt_vectors", "ctx_msm", "ctx_other")]


class PkRawInfo(C.Structure):
    _fields_ = [("log_n", C.c_uint32), ("n_commitment_keys", C.c_uint32)] + [(n, C.c_uint64) for n in (
        "nb_wires", "n_g1_a", "n_g1_b", "n_g1_z", "n_g1_k", "n_g2_b", "off_alpha1", "off_g1_a", "off_g1_b", "off_g1_z", "off_g1_k",
        "off_beta2", "off_g2_b", "off_infinity_a", "off_infinity_b")] + [
        ("n_basis", C.c_uint64 * 16), ("off_basis", C.c_uint64 * 16), ("off_basis_exp_sigma", C.c_uint64 * 16)]


def pk_raw_inspect(blob: bytes):
    """section offsets / counts of a gnark ProvingKey.WriteRawTo stream (host only); raises MiError if the layout does not parse"""
    info = PkRawInfo(); buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
    if load().mi_pk_raw_inspect(buf, C.c_size_t(len(blob)), C.byref(info)) != 0:
        raise MiError("mi_pk_raw_inspect: not a gnark v0.11.0 ProvingKey.WriteRawTo stream (as recalled)")
    return info


class PedersenArrays(C.Structure):
    _fields_ = [("basis_dev", C.c_void_p), ("basis_exp_sigma_dev", C.c_void_p), ("n", C.c_uint64)]


class KeyfileStats(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("upload_ms", "decode_ms", "subgroup_ms", "build_ms", "total_ms")]


def pk_stream_inspect(blob: bytes):
    """(section offsets / counts, KEYFILE_RAW or KEYFILE_COMPRESSED) of a proving key's stream (host only); raises MiError if neither layout parses"""
    info = PkRawInfo(); enc = C.c_uint32(); buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
    if load().mi_pk_stream_inspect(buf, C.c_size_t(len(blob)), C.byref(info), C.byref(enc)) != 0:
        raise MiError("mi_pk_stream_inspect: neither a ProvingKey.WriteRawTo nor a ProvingKey.WriteTo stream (as recalled)")
    return info, int(enc.value)


def _pedersen_arrays(ped):
    """[(basis device pointer, basis_exp_sigma device pointer, n)] -> the C array"""
    arr = (PedersenArrays * max(len(ped), 1))()
    for k, (b, s, n) in enumerate(ped):
        arr[k].basis_dev, arr[k].basis_exp_sigma_dev, arr[k].n = (int(b) if b else None), (int(s) if s else None), int(n)
    return arr


def pk_stream_size(counts: dict, ped_ns=(), encoding=KEYFILE_COMPRESSED):
    """mi_pk_stream_size: counts = nb_wires and n_g1_a, n_g1_b, n_g1_k, n_g1_z, n_g2_b"""
    d = PkDesc()
    for k, v in counts.items():
        setattr(d, k, int(v))
    n = C.c_size_t()
    if load().mi_pk_stream_size(C.byref(d), _pedersen_arrays([(None, None, m) for m in ped_ns]), C.c_uint32(len(ped_ns)), C.c_uint32(encoding), C.byref(n)) != 0:
        raise MiError("mi_pk_stream_size refused its arguments")
    return int(n.value)


class R1csMatrix(C.Structure):
    _fields_ = [("row_ptr", C.c_void_p), ("col", C.c_void_p), ("coeff", C.c_void_p)]


class R1csDesc(C.Structure):
    _fields_ = [("n_constraints", C.c_uint64), ("nb_wires", C.c_uint64), ("nb_public", C.c_uint32),
                ("A", R1csMatrix), ("B", R1csMatrix), ("C", R1csMatrix), ("coeffs", C.c_void_p), ("n_coeffs", C.c_uint64),
                ("n_commitments", C.c_uint32), ("committed", C.POINTER(C.c_void_p)), ("n_committed", C.POINTER(C.c_uint64)),
                ("commitment_wire", C.c_void_p)]


class Trapdoor(C.Structure):
    _fields_ = [(n, C.c_uint64 * 4) for n in ("tau", "alpha", "beta", "gamma", "delta")] + [("sigma", (C.c_uint64 * 4) * MAX_COMMITMENTS)]


class VkOut(C.Structure):
    _fields_ = [("alpha1", C.c_uint64 * 8), ("beta2", C.c_uint64 * 16), ("gamma2", C.c_uint64 * 16), ("delta2", C.c_uint64 * 16),
                ("k", C.c_void_p), ("k_cap", C.c_uint64), ("n_k", C.c_uint64)]


class SetupExponents(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("a", "b", "c", "k", "k_gamma", "z", "infinity_a", "infinity_b")]


class SetupStats(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("upload_ms", "lagrange_ms", "sparse_ms", "elementwise_ms", "points_ms", "handover_ms", "total_ms",
                                         "sparse_sort_ms", "sparse_sum_ms")] + [(n, C.c_uint64) for n in ("entries", "long_columns", "chunks")]


class SrsDesc(C.Structure):
    _fields_ = [("tau_g1", C.c_void_p), ("alpha_tau_g1", C.c_void_p), ("beta_tau_g1", C.c_void_p), ("tau_g2", C.c_void_p), ("beta_g2", C.c_uint64 * 16)] + [
        (n, C.c_uint64) for n in ("n_tau_g1", "n_alpha_tau_g1", "n_beta_tau_g1", "n_tau_g2")]


class Phase2Stats(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("upload_ms", "check_ms", "point_ntt_g1_ms", "point_ntt_g2_ms", "sparse_g1_ms", "sparse_g2_ms", "z_ms",
                                         "affine_ms", "total_ms")] + [("pad_", C.c_uint32)] + [(n, C.c_uint64) for n in ("entries", "long_columns", "chunks", "peak_bytes")]


class SrsCheckStats(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("upload_ms", "point_check_ms", "coeff_ms", "msm_g1_ms", "msm_g2_ms", "pairing_ms", "total_ms")] + [
        ("pad_", C.c_uint32), ("peak_bytes", C.c_uint64)]


class KeyAuditStats(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("upload_ms", "point_check_ms", "coeff_ms", "sparse_ms", "transform_ms", "srs_msm_g1_ms", "srs_msm_g2_ms",
                                         "key_msm_g1_ms", "key_msm_g2_ms", "pairing_ms", "total_ms")] + [("relations", C.c_uint32), ("peak_bytes", C.c_uint64)]


class KeyAuditSums(C.Structure):
    _fields_ = [(n, (C.c_uint64 * 8) * 2) for n in ("a", "b1", "k_private", "k_public", "basis", "z")] + [
        ("b2", (C.c_uint64 * 16) * 2), ("sigma", ((C.c_uint64 * 8) * 2) * 16), ("n_sigma", C.c_uint32), ("valid", C.c_uint32)]


class Phase1Stats(C.Structure):
    _fields_ = [("scalar_mul_ms", C.c_float * 4), ("affine_ms", C.c_float * 4), ("total_ms", C.c_float), ("window", C.c_uint32), ("chunk", C.c_uint32),
                ("pad_", C.c_uint32), ("peak_bytes", C.c_uint64)]


class Phase1Info(C.Structure):
    _fields_ = [("log_n", C.c_uint32), ("pad_", C.c_uint32), ("n_records", C.c_uint64), ("chain", C.c_uint8 * 32), ("tau1", C.c_uint64 * 8),
                ("alpha1", C.c_uint64 * 8), ("beta1", C.c_uint64 * 8)]


class Phase2Claim(C.Structure):
    _fields_ = [("g1_z", C.c_void_p), ("n_z", C.c_uint64), ("g1_k", C.c_void_p), ("n_k", C.c_uint64), ("delta1", C.c_uint64 * 8), ("delta2", C.c_uint64 * 16)]


class Phase2SigmaClaim(C.Structure):
    _fields_ = [("basis_exp_sigma", C.c_void_p), ("n", C.c_void_p), ("g_sigma_neg", C.c_void_p)]


class Phase2ChainInfo(C.Structure):
    _fields_ = [("n_commitments", C.c_uint32), ("pad_", C.c_uint32), ("n_records", C.c_uint64), ("chain", C.c_uint8 * 32), ("n_sigma_records", C.c_uint64),
                ("sigma_chain", C.c_uint8 * 32)]


def _sigma_steps(proofs, hashes, nc):
    """proofs: (m, nc, PHASE2_SIGMA_PROOF_WORDS) uint64; hashes: m values of 32 bytes -> (the array, the hashes as one buffer, m)"""
    pr = _u64(proofs).reshape(-1, nc, PHASE2_SIGMA_PROOF_WORDS)
    hs = b"".join(bytes(h) for h in hashes)
    if len(hs) != 32 * pr.shape[0]:
        raise ValueError("one 32-byte chain value per step")
    return pr, (C.c_uint8 * max(len(hs), 1)).from_buffer_copy(hs or b"\0"), pr.shape[0]


def _srs_desc(srs: dict):
    """srs: tau_g1 (n, 8), alpha_tau_g1, beta_tau_g1 (n, 8), tau_g2 (n, 16), beta_g2 (16,) uint64 Montgomery; a row may be None, and
    n_<row> overrides the count the array has -> (SrsDesc, the arrays it points into)"""
    d = SrsDesc(); keep = []
    for name in ("tau_g1", "alpha_tau_g1", "beta_tau_g1", "tau_g2"):
        a = srs.get(name)
        if a is not None:
            a = _u64(a); keep.append(a)
            setattr(d, name, a.ctypes.data)
        setattr(d, "n_" + name, int(srs.get("n_" + name, 0 if a is None else a.shape[0])))
    d.beta_g2 = (C.c_uint64 * 16)(*[int(v) for v in _u64(srs["beta_g2"]).reshape(16)])
    return d, keep


class R1csStats(C.Structure):
    _fields_ = [("eval_ms", C.c_float), ("matrices", C.c_uint32)] + [(n, C.c_uint64) for n in ("entries", "long_rows", "pieces")]


def _r1cs_desc(r1cs: dict):
    """r1cs: n_constraints, nb_wires, nb_public, A / B / C = (row_ptr uint64, col uint32, coeff uint32), coeffs (n, 4) uint64 Montgomery,
    commitments = [(committed private wires uint32, commitment wire)] -> (R1csDesc, the arrays it points into)"""
    d = R1csDesc(); keep = []
    d.n_constraints, d.nb_wires, d.nb_public = int(r1cs["n_constraints"]), int(r1cs["nb_wires"]), int(r1cs["nb_public"])
    for name in "ABC":
        rp, col, cf = r1cs[name]
        rp = None if rp is None else np.ascontiguousarray(rp, dtype=np.uint64)
        col = None if col is None else np.ascontiguousarray(col, dtype=np.uint32)
        cf = None if cf is None else np.ascontiguousarray(cf, dtype=np.uint32)
        keep += [rp, col, cf]
        m = getattr(d, name)
        m.row_ptr, m.col, m.coeff = (None if x is None else x.ctypes.data for x in (rp, col, cf))
    co = r1cs["coeffs"]
    if co is not None:
        co = _u64(co); keep.append(co)
        d.coeffs = co.ctypes.data
    d.n_coeffs = int(r1cs.get("n_coeffs", 0 if co is None else co.shape[0]))
    com = r1cs.get("commitments") or []
    d.n_commitments = int(r1cs.get("n_commitments", len(com)))
    if com:
        wires = [np.ascontiguousarray(w, dtype=np.uint32) for w, _ in com]
        ptrs = (C.c_void_p * len(com))(*[w.ctypes.data for w in wires])
        cnts = (C.c_uint64 * len(com))(*[w.shape[0] for w in wires])
        cw = np.array([int(c) for _, c in com], dtype=np.uint32)
        keep += [wires, ptrs, cnts, cw]
        d.committed, d.n_committed, d.commitment_wire = C.cast(ptrs, C.POINTER(C.c_void_p)), C.cast(cnts, C.POINTER(C.c_uint64)), cw.ctypes.data
    return d, keep


def _trapdoor(td: dict):
    """td: tau, alpha, beta, gamma, delta as (4,) uint64 Montgomery rows, sigma = list of such rows"""
    t = Trapdoor()
    for n in ("tau", "alpha", "beta", "gamma", "delta"):
        setattr(t, n, (C.c_uint64 * 4)(*[int(v) for v in _u64(td[n]).reshape(4)]))
    for k, sg in enumerate(td.get("sigma", [])):
        t.sigma[k] = (C.c_uint64 * 4)(*[int(v) for v in _u64(sg).reshape(4)])
    return t


class PedersenVk(C.Structure):
    _fields_ = [("g", C.c_uint64 * 16), ("g_sigma_neg", C.c_uint64 * 16)]


class VkDesc(C.Structure):
    _fields_ = [("alpha1", C.c_uint64 * 8), ("beta2", C.c_uint64 * 16), ("gamma2", C.c_uint64 * 16), ("delta2", C.c_uint64 * 16),
                ("k", C.c_void_p), ("n_k", C.c_uint64), ("nb_public", C.c_uint32), ("n_commitments", C.c_uint32), ("ped", C.c_void_p)]


class VerifyInput(C.Structure):
    _fields_ = [("proof", C.c_uint64 * 32), ("commitments", C.c_void_p), ("pok", C.c_void_p), ("public_inputs", C.c_void_p),
                ("commitment_values", C.c_void_p), ("fold_challenge", C.c_void_p)]


class VerifyBytesInput(C.Structure):
    _fields_ = [("proof", C.c_void_p), ("proof_len", C.c_size_t), ("public_inputs", C.c_void_p)]


class VerifyFilesInput(C.Structure):
    _fields_ = [("proof", C.c_void_p), ("proof_len", C.c_size_t), ("witness", C.c_void_p), ("witness_len", C.c_size_t)]


class VkStreamInfo(C.Structure):
    _fields_ = [("n_k", C.c_uint64), ("nb_public", C.c_uint32), ("n_commitment_keys", C.c_uint32)] + [(n, C.c_uint64) for n in (
        "off_alpha1", "off_beta1", "off_beta2", "off_gamma2", "off_delta1", "off_delta2", "off_k", "off_lists")] + [
        ("list_len", C.c_uint64 * 16), ("off_list", C.c_uint64 * 16), ("off_commitment_keys", C.c_uint64), ("off_ped", C.c_uint64 * 16),
        ("refused", C.c_char * 96)]


class VkFileDesc(C.Structure):
    _fields_ = [("alpha1", C.c_uint64 * 8), ("beta1", C.c_uint64 * 8), ("delta1", C.c_uint64 * 8), ("beta2", C.c_uint64 * 16),
                ("gamma2", C.c_uint64 * 16), ("delta2", C.c_uint64 * 16), ("k", C.c_void_p), ("n_k", C.c_uint64), ("nb_public", C.c_uint32),
                ("n_commitments", C.c_uint32), ("ped", C.c_void_p), ("pc_offsets", C.c_void_p), ("pc_indices", C.c_void_p)]


def vk_stream_inspect(blob: bytes):
    """(field offsets / counts, KEYFILE_RAW or KEYFILE_COMPRESSED) of a verifying key's stream (host only); raises MiError naming the
    field if neither layout parses"""
    info = VkStreamInfo(); enc = C.c_uint32(); buf = (C.c_uint8 * max(len(blob), 1)).from_buffer_copy(blob or b"\0")
    if load().mi_vk_stream_inspect(buf, C.c_size_t(len(blob)), C.byref(info), C.byref(enc)) != 0:
        raise MiError("mi_vk_stream_inspect: neither a VerifyingKey.WriteRawTo nor a VerifyingKey.WriteTo stream (as recalled): " + info.refused.decode())
    return info, int(enc.value)


def _vk_file_desc(vk: dict, nb_public, ped=None, lists=None):
    """the vk dict of setup() plus beta1 and delta1, the Pedersen verifying keys and the committed lists -> (VkFileDesc, what it points to)"""
    d = VkFileDesc()
    for n, w in (("alpha1", 8), ("beta1", 8), ("delta1", 8), ("beta2", 16), ("gamma2", 16), ("delta2", 16)):
        if vk.get(n) is not None:
            setattr(d, n, (C.c_uint64 * w)(*[int(v) for v in _u64(vk[n]).reshape(w)]))
    k = _u64(vk["k"]).reshape(-1, 8)
    ped = None if ped is None else _u64(ped).reshape(-1, 2, 16)
    d.k, d.n_k, d.nb_public = k.ctypes.data, int(k.shape[0]), int(nb_public)
    d.n_commitments = 0 if ped is None else int(ped.shape[0])
    d.ped = None if ped is None else ped.ctypes.data
    off = idx = None
    if lists is not None:
        off = np.cumsum([0] + [len(l) for l in lists]).astype(np.uint32)
        idx = np.array([j for l in lists for j in l], np.uint32)
        d.pc_offsets = off.ctypes.data
        d.pc_indices = idx.ctypes.data if len(idx) else None
    return d, (k, ped, off, idx)


def vk_stream_size(n_k, n_commitments=0, n_indices=0, encoding=KEYFILE_COMPRESSED):
    d = VkFileDesc(); d.n_k, d.n_commitments = int(n_k), int(n_commitments)
    off = np.array([0] * int(n_commitments) + [int(n_indices)], np.uint32); d.pc_offsets = off.ctypes.data
    n = C.c_size_t()
    if load().mi_vk_stream_size(C.byref(d), C.c_uint32(encoding), C.byref(n)) != 0:
        raise MiError("mi_vk_stream_size refused its arguments")
    return int(n.value)


def public_witness_write(values, cap=None) -> bytes:
    """mi_public_witness_write: (n, 4) Montgomery values -> witness.WriteTo's bytes of a public witness"""
    v = _u64(values).reshape(-1, 4); n = v.shape[0]
    cap = 12 + 32 * n if cap is None else cap
    out = (C.c_uint8 * max(cap, 1))(); need = C.c_size_t()
    if load().mi_public_witness_write(_p(v) if n else None, C.c_size_t(n), out, C.c_size_t(cap), C.byref(need)) != 0:
        raise MiError(f"mi_public_witness_write: MI_EINVAL ({need.value} bytes needed)")
    return C.string_at(out, need.value)


def public_witness_read(data: bytes, cap=None):
    """mi_public_witness_read: the public part of a witness's bytes -> (nbPublic, 4) uint64 Montgomery; MiError for a header that
    disagrees with the length or a value not below r"""
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    cap = max((len(data) - 12) // 32, 0) if cap is None else cap
    out = np.zeros((max(cap, 1), 4), np.uint64); n = C.c_size_t()
    if load().mi_public_witness_read(buf, C.c_size_t(len(data)), _p(out), C.c_size_t(cap), C.byref(n)) != 0:
        raise MiError("mi_public_witness_read: MI_EINVAL")
    return out[:int(n.value)].copy()


class VerifyLocateStats(C.Structure):
    _fields_ = [("rounds", C.c_uint32), ("nodes_tested", C.c_uint64), ("judged_alone", C.c_uint64), ("malformed", C.c_uint64), ("rejected", C.c_uint64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class VkKsumInfo(C.Structure):
    _fields_ = [("window_bits", C.c_uint32), ("windows", C.c_uint32), ("table_bytes", C.c_uint64), ("bases", C.c_uint64), ("budget_bytes", C.c_uint64),
                ("state", C.c_uint32), ("build_ms", C.c_float)]

    def as_dict(self):
        return {n: (float if n == "build_ms" else int)(getattr(self, n)) for n, _ in self._fields_}


class Bsb22Input(C.Structure):
    _fields_ = [("key", C.c_void_p), ("values", C.c_void_p), ("n", C.c_size_t)]


class Stats(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("h2d_ms", "compute_h_ms", "filter_ms", "msm_a_ms", "msm_b1_ms", "msm_k_ms",
                                         "msm_z_ms", "msm_b2_ms", "assemble_ms", "total_ms")] + [
        ("g1_accum_kernel_ms", C.c_float), ("g1_accum_pairs", C.c_uint64), ("g1_accum_launches", C.c_uint32),
        ("ntt_kernel_ms", C.c_float), ("ntt_elems", C.c_uint64), ("ntt_launches", C.c_uint32), ("g1_accum_entries", C.c_uint64), ("g1_level1_additions", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class MiError(RuntimeError):
    pass


def load():
    """dlopen the HIP library; raises if it has not been built (no CPU fallback exists)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise MiError(f"{LIB_PATH} missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        _LIB = C.CDLL(LIB_PATH)
        _LIB.mi_last_error.restype = C.c_char_p
        _LIB.mi_proof_write.restype = C.c_size_t
        _LIB.mi_prover_last_error.restype = C.c_char_p
        _LIB.mi_prover_ctx.restype = C.c_void_p
        _LIB.mi_prover_in_flight.restype = C.c_uint32
        _LIB.mi_group_ctx.restype = C.c_void_p
        _LIB.mi_group_last_error.restype = C.c_char_p
    return _LIB


DIST_UNIFORM, DIST_WHIR = 0, 1


def dist_mix(bit_pm, byte_pm, u64_pm=0):
    """MI_DIST_MIX(bit, byte, u64) of include/mi355x_groth16_debug.h: per-mille shares of {0,1} / bytes / 64-bit scalars, the rest uniform Fr"""
    assert 0 <= bit_pm and 0 <= byte_pm and 0 <= u64_pm and bit_pm + byte_pm + u64_pm <= 1000
    return 0x40000000 | (bit_pm << 20) | (byte_pm << 10) | u64_pm


def _p(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    return C.c_void_p(int(a))  # raw device pointer


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


class DevArray:
    """A hipMalloc'ed buffer owned through the C-ABI (mi_dev_alloc)."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, int(nbytes)
        ptr = C.c_void_p()
        ctx._ck(ctx.lib.mi_dev_alloc(ctx.h, C.c_size_t(self.nbytes), C.byref(ptr)))
        self.ptr = ptr.value

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        self.ctx._ck(self.ctx.lib.mi_dev_upload(self.ctx.h, C.c_void_p(self.ptr), _p(arr), C.c_size_t(arr.nbytes)))
        return self

    def download(self, shape, dtype=np.uint64):
        out = np.zeros(shape, dtype)
        assert out.nbytes <= self.nbytes
        self.ctx._ck(self.ctx.lib.mi_dev_download(self.ctx.h, _p(out), C.c_void_p(self.ptr), C.c_size_t(out.nbytes)))
        return out

    def free(self):
        if self.ptr:
            self.ctx.lib.mi_dev_free(self.ctx.h, C.c_void_p(self.ptr))
            self.ptr = None


class Context:
    def __init__(self, device_id=0, _borrowed=None):
        self.lib = load()
        self.owned = _borrowed is None
        if _borrowed is not None:      # a context owned by a Prover pool (mi_prover_ctx)
            self.h = C.c_void_p(_borrowed)
            return
        h = C.c_void_p()
        rc = self.lib.mi_init(C.c_int(device_id), C.byref(h))
        if rc != 0:
            raise MiError(f"mi_init failed: {rc} (no gfx950 device? the product has no CPU path)")
        self.h = h

    def _ck(self, rc):
        if rc != 0:
            raise MiError(f"rc={rc}: {self.lib.mi_last_error(self.h).decode()}")

    def close(self):
        if self.h and self.owned:
            self.lib.mi_shutdown(self.h)
        self.h = None

    def set_stream(self, stream_ptr):
        self._ck(self.lib.mi_set_stream(self.h, C.c_void_p(int(stream_ptr))))

    def sync(self):
        self._ck(self.lib.mi_dev_sync(self.h))

    def set_knob(self, name, value):
        """mi_debug_set_knob: a named measurement / test knob of this context (the header lists them)"""
        self._ck(self.lib.mi_debug_set_knob(self.h, C.c_char_p(name.encode()), C.c_int64(int(value))))

    def counter(self, name):
        """mi_debug_get_counter: how often an optional path ran on this context"""
        v = C.c_uint64()
        self._ck(self.lib.mi_debug_get_counter(self.h, C.c_char_p(name.encode()), C.byref(v)))
        return int(v.value)

    def alloc(self, nbytes):
        return DevArray(self, nbytes)

    def to_dev(self, arr):
        arr = np.ascontiguousarray(arr)
        return DevArray(self, max(arr.nbytes, 32)).upload(arr)

    # ---- utilities
    def gen_scalars(self, n, seed, dist):
        d = self.alloc(32 * n); self._ck(self.lib.mi_gen_scalars_dev(self.h, _p(d.ptr), C.c_size_t(n), C.c_uint64(seed), C.c_int(dist))); return d

    def gen_g1(self, n, seed):
        d = self.alloc(64 * n); self._ck(self.lib.mi_gen_g1_dev(self.h, _p(d.ptr), C.c_size_t(n), C.c_uint64(seed))); return d

    def gen_g2(self, n, seed):
        d = self.alloc(128 * n); self._ck(self.lib.mi_gen_g2_dev(self.h, _p(d.ptr), C.c_size_t(n), C.c_uint64(seed))); return d

    def field_op(self, field, op, x, y=None):
        x = _u64(x); n = x.shape[0]
        dx = self.to_dev(x); dy = self.to_dev(_u64(y)) if y is not None else None; dz = self.alloc(32 * n)
        self._ck(self.lib.mi_field_op_dev(self.h, field, op, _p(dz.ptr), _p(dx.ptr), _p(dy.ptr if dy else None), C.c_size_t(n)))
        out = dz.download((n, 4))
        for b in (dx, dy, dz):
            if b: b.free()
        return out

    def field_op_dev(self, field, op, z_ptr, x_ptr, y_ptr, n):
        self._ck(self.lib.mi_field_op_dev(self.h, C.c_int(field), C.c_int(op), _p(z_ptr), _p(x_ptr), _p(y_ptr), C.c_size_t(n)))

    def limb29_op(self, op, recs):
        """records of csrc/limb29_ops.cuh ((n, 144) uint32) through mi_debug_limb29_op_dev -> (n, 80) uint32"""
        recs = np.ascontiguousarray(recs, dtype=np.uint32).reshape(-1, 144); n = recs.shape[0]
        di = self.to_dev(recs); do = self.alloc(max(320 * n, 32))
        self._ck(self.lib.mi_debug_limb29_op_dev(self.h, C.c_int(op), _p(do.ptr), _p(di.ptr), C.c_size_t(n)))
        out = do.download((n, 80), np.uint32) if n else np.zeros((0, 80), np.uint32)
        di.free(); do.free()
        return out

    def lazy_op(self, op, recs):
        """records of csrc/lazy_ops.cuh ((n, 24) uint32) through mi_debug_lazy_op_dev -> (n, 16) uint32"""
        recs = np.ascontiguousarray(recs, dtype=np.uint32).reshape(-1, 24); n = recs.shape[0]
        di = self.to_dev(recs); do = self.alloc(max(64 * n, 32))
        self._ck(self.lib.mi_debug_lazy_op_dev(self.h, C.c_int(op), _p(do.ptr), _p(di.ptr), C.c_size_t(n)))
        out = do.download((n, 16), np.uint32) if n else np.zeros((0, 16), np.uint32)
        di.free(); do.free()
        return out

    def field_shape(self, shape, recs):
        """records of csrc/shape_ops.cuh ((n, 32) uint32) through mi_debug_field_shape_dev -> (n, 32) uint32"""
        recs = np.ascontiguousarray(recs, dtype=np.uint32).reshape(-1, 32); n = recs.shape[0]
        di = self.to_dev(recs); do = self.alloc(max(128 * n, 32))
        self._ck(self.lib.mi_debug_field_shape_dev(self.h, C.c_int(shape), _p(do.ptr), _p(di.ptr), C.c_size_t(n)))
        out = do.download((n, 32), np.uint32) if n else np.zeros((0, 32), np.uint32)
        di.free(); do.free()
        return out

    def ec_add(self, a, b, g2=False):
        a, b = _u64(a), _u64(b); n = a.shape[0]
        da, db = self.to_dev(a), self.to_dev(b); do = self.alloc(a.nbytes)
        f = self.lib.mi_g2_add_dev if g2 else self.lib.mi_g1_add_dev
        self._ck(f(self.h, _p(do.ptr), _p(da.ptr), _p(db.ptr), C.c_size_t(n)))
        out = do.download(a.shape)
        for x in (da, db, do): x.free()
        return out

    def bench_modmul(self, field, n_threads, iters):
        s = self.alloc(1024 * 32); ms = C.c_float()
        self._ck(self.lib.mi_bench_modmul_dev(self.h, field, C.c_size_t(n_threads), C.c_uint32(iters), _p(s.ptr), C.byref(ms)))
        s.free(); return ms.value

    def bench_gather(self, table_ptr, n_entries, n_threads, iters):
        s = self.alloc(1024); ms = C.c_float()
        self._ck(self.lib.mi_bench_gather_dev(self.h, _p(table_ptr), C.c_size_t(n_entries), C.c_size_t(n_threads), C.c_uint32(iters), _p(s.ptr), C.byref(ms)))
        s.free(); return ms.value

    def bench_valu(self, kind, n_threads, iters):
        s = self.alloc(1024); ms = C.c_float()
        self._ck(self.lib.mi_bench_valu_dev(self.h, kind, C.c_size_t(n_threads), C.c_uint32(iters), _p(s.ptr), C.byref(ms)))
        s.free(); return ms.value

    # ---- NTT / computeH
    def ntt(self, a, log_n, flags):
        a = _u64(a).copy(); self._ck(self.lib.mi_ntt(self.h, _p(a), C.c_uint32(log_n), C.c_uint32(flags))); return a

    def ntt_dev(self, dptr, log_n, flags):
        self._ck(self.lib.mi_ntt_dev(self.h, _p(dptr), C.c_uint32(log_n), C.c_uint32(flags)))

    def compute_h(self, log_n, a, b, c):
        h = np.zeros((1 << log_n, 4), np.uint64)
        a, b, c = _u64(a), _u64(b), (None if c is None else _u64(c))
        self._ck(self.lib.mi_compute_h(self.h, C.c_uint32(log_n), _p(a), _p(b), _p(c), C.c_size_t(a.shape[0]), _p(h)))
        return h

    def compute_h_dev(self, log_n, a, b, c, n_constraints, h):
        self._ck(self.lib.mi_compute_h_dev(self.h, C.c_uint32(log_n), _p(a), _p(b), _p(c), C.c_size_t(n_constraints), _p(h)))

    # ---- MSM
    def msm_g1(self, pts, sc, flags=0):
        out = np.zeros(12, np.uint64); pts, sc = _u64(pts), _u64(sc)
        self._ck(self.lib.mi_msm_g1(self.h, _p(pts), _p(sc), C.c_size_t(pts.shape[0]), C.c_uint32(flags), _p(out))); return out

    def msm_g2(self, pts, sc, flags=0):
        out = np.zeros(24, np.uint64); pts, sc = _u64(pts), _u64(sc)
        self._ck(self.lib.mi_msm_g2(self.h, _p(pts), _p(sc), C.c_size_t(pts.shape[0]), C.c_uint32(flags), _p(out))); return out

    def msm_g1_dev(self, pts_ptr, sc_ptr, n, flags=0):
        out = np.zeros(12, np.uint64)
        self._ck(self.lib.mi_msm_g1_dev(self.h, _p(pts_ptr), _p(sc_ptr), C.c_size_t(n), C.c_uint32(flags), _p(out))); return out

    def msm_g2_dev(self, pts_ptr, sc_ptr, n, flags=0):
        out = np.zeros(24, np.uint64)
        self._ck(self.lib.mi_msm_g2_dev(self.h, _p(pts_ptr), _p(sc_ptr), C.c_size_t(n), C.c_uint32(flags), _p(out))); return out

    # ---- fixed-base MSM (window copies of static bases)
    def msm_precompute(self, base_ptr, n, c, g2=False):
        nwin = (256 + c - 1) // c
        pre = self.alloc((128 if g2 else 64) * n * nwin)
        f = self.lib.mi_msm_precompute_g2_dev if g2 else self.lib.mi_msm_precompute_g1_dev
        self._ck(f(self.h, _p(base_ptr), C.c_size_t(n), C.c_uint32(c), _p(pre.ptr)))
        return pre

    def msm_table_to_rprime(self, pre_ptr, n_points, g2=False):
        f = self.lib.mi_msm_table_to_rprime_g2_dev if g2 else self.lib.mi_msm_table_to_rprime_g1_dev
        self._ck(f(self.h, _p(pre_ptr), C.c_size_t(n_points)))

    def pk_table_plan(self, pkh):
        c = (C.c_uint32 * 3)()
        self._ck(self.lib.mi_pk_table_plan(pkh, c))
        return tuple(int(x) for x in c)

    def msm_fixed_dev(self, pre_ptr, sc_ptr, n, c, flags=0, g2=False):
        out = np.zeros(24 if g2 else 12, np.uint64)
        f = self.lib.mi_msm_g2_fixed_dev if g2 else self.lib.mi_msm_g1_fixed_dev
        self._ck(f(self.h, _p(pre_ptr), _p(sc_ptr), C.c_size_t(n), C.c_uint32(c), C.c_uint32(flags), _p(out)))
        return out

    # ---- proving key + prove
    def pk_load(self, pk: dict, device_points=False):
        """pk arrays: numpy (host) or raw device pointers with explicit counts when device_points."""
        d = PkDesc(); keep = []
        d.log_n, d.nb_public, d.nb_wires = pk["log_n"], pk["nb_public"], pk["nb_wires"]
        for name in ("g1_a", "g1_b", "g1_k", "g1_z", "g2_b"):
            if device_points:
                ptr, cnt = pk[name]
                setattr(d, name, int(ptr)); setattr(d, "n_" + name, int(cnt))
            else:
                arr = _u64(pk[name]); keep.append(arr)
                setattr(d, name, arr.ctypes.data); setattr(d, "n_" + name, arr.shape[0])
        for name, k in (("alpha1", 8), ("beta1", 8), ("delta1", 8), ("beta2", 16), ("delta2", 16)):
            setattr(d, name, (C.c_uint64 * k)(*[int(v) for v in _u64(pk[name]).reshape(-1)]))
        ia = np.ascontiguousarray(pk["infinity_a"], dtype=np.uint8); ib = np.ascontiguousarray(pk["infinity_b"], dtype=np.uint8)
        keep += [ia, ib]
        d.infinity_a, d.infinity_b = ia.ctypes.data, ib.ctypes.data
        cw = pk.get("committed_wires")
        if cw is not None and len(cw):
            cw = np.ascontiguousarray(cw, dtype=np.uint32); keep.append(cw)
            d.committed_wires, d.n_committed = cw.ctypes.data, cw.shape[0]
        h = C.c_void_p()
        f = self.lib.mi_pk_load_dev if device_points else self.lib.mi_pk_load
        self._ck(f(self.h, C.byref(d), C.byref(h)))
        return h

    def pk_load_raw(self, blob: bytes, nb_public, committed_wires=None):
        """gnark ProvingKey.WriteRawTo stream -> (device-resident key, [Pedersen key handles])"""
        buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob); h = C.c_void_p()
        ped = (C.c_void_p * 16)(); nped = C.c_uint32()
        cw = None if committed_wires is None or not len(committed_wires) else np.ascontiguousarray(committed_wires, dtype=np.uint32)
        self._ck(self.lib.mi_pk_load_raw(self.h, buf, C.c_size_t(len(blob)), C.c_uint32(nb_public), _p(cw), C.c_size_t(0 if cw is None else cw.shape[0]),
                                         C.byref(h), ped, C.byref(nped)))
        return h, [C.c_void_p(ped[i]) for i in range(nped.value)]

    def pk_free(self, pkh):
        self._ck(self.lib.mi_pk_free(self.h, pkh))

    def prove(self, pkh, W, a, b, c, r, s, device=False, n_wires=None, n_constraints=None):
        out = np.zeros(32, np.uint64); st = Stats()
        r, s = _u64(r), _u64(s)
        if device:
            self._ck(self.lib.mi_groth16_prove_dev(self.h, pkh, _p(W), C.c_size_t(n_wires), _p(a), _p(b), _p(c),
                                                   C.c_size_t(n_constraints), _p(r), _p(s), _p(out), C.byref(st)))
        else:
            W, a, b, c = _u64(W), _u64(a), _u64(b), (None if c is None else _u64(c))   # c = None: formed on the device as a o b
            self._ck(self.lib.mi_groth16_prove(self.h, pkh, _p(W), C.c_size_t(W.shape[0]), _p(a), _p(b), _p(c),
                                               C.c_size_t(a.shape[0]), _p(r), _p(s), _p(out), C.byref(st)))
        return {"ar": out[:8].copy(), "bs": out[8:24].copy(), "krs": out[24:].copy(), "raw": out}, st.as_dict()

    # ---- fixed-base batch scalar multiplication
    def batch_scalar_mul(self, base, scalars, g2=False):
        base, scalars = _u64(base), _u64(scalars); out = np.zeros((scalars.shape[0], 16 if g2 else 8), np.uint64)
        f = self.lib.mi_batch_scalar_mul_g2 if g2 else self.lib.mi_batch_scalar_mul_g1
        self._ck(f(self.h, _p(base), _p(scalars), C.c_size_t(scalars.shape[0]), _p(out)))
        return out

    def batch_scalar_mul_dev(self, base, scalars_ptr, n, out_ptr, g2=False):
        f = self.lib.mi_batch_scalar_mul_g2_dev if g2 else self.lib.mi_batch_scalar_mul_g1_dev
        self._ck(f(self.h, _p(_u64(base)), _p(scalars_ptr), C.c_size_t(n), _p(out_ptr)))

    # ---- BSB22 Pedersen key
    def pedersen_pk_load(self, basis, basis_exp_sigma):
        basis, bes = _u64(basis), _u64(basis_exp_sigma); h = C.c_void_p()
        self._ck(self.lib.mi_pedersen_pk_load(self.h, _p(basis), _p(bes), C.c_size_t(basis.shape[0]), C.byref(h)))
        return h

    def pedersen_pk_free(self, pk):
        self._ck(self.lib.mi_pedersen_pk_free(self.h, pk))

    def pedersen_commit(self, pk, values, knowledge=False):
        values = _u64(values); out = np.zeros(8, np.uint64)
        f = self.lib.mi_pedersen_prove_knowledge if knowledge else self.lib.mi_pedersen_commit
        self._ck(f(self.h, pk, _p(values), C.c_size_t(values.shape[0]), _p(out)))
        return out

    # ---- groth16.Setup on the device (include/mi355x_groth16_setup.h)
    def setup_exponents(self, r1cs: dict, td: dict, want=("a", "b", "c", "k", "k_gamma", "z", "infinity_a", "infinity_b")):
        """mi_groth16_setup_exponents: the Fr half of Setup -> dict of host arrays ((n, 4) uint64 Montgomery; the masks uint8)"""
        d, keep = _r1cs_desc(r1cs); t = _trapdoor(td)
        nw = d.nb_wires; N = 1 << max(int(d.n_constraints) - 1, 0).bit_length()
        out = {n: (np.zeros(nw, np.uint8) if n.startswith("inf") else np.zeros((N if n == "z" else nw, 4), np.uint64)) for n in want}
        e = SetupExponents()
        for n, arr in out.items():
            setattr(e, n, arr.ctypes.data)
        self._ck(self.lib.mi_groth16_setup_exponents(self.h, C.byref(d), C.byref(t), C.byref(e)))
        return out

    def setup(self, r1cs: dict, td: dict):
        """mi_groth16_setup -> (key handle, [Pedersen key handles], vk dict: alpha1, beta2, gamma2, delta2, k (n, 8))"""
        d, keep = _r1cs_desc(r1cs); t = _trapdoor(td)
        cap = int(d.nb_public) + int(d.n_commitments)
        vk_k = np.zeros((max(cap, 1), 8), np.uint64)
        vk = VkOut(); vk.k = vk_k.ctypes.data; vk.k_cap = cap
        h = C.c_void_p(); ped = (C.c_void_p * MAX_COMMITMENTS)()
        self._ck(self.lib.mi_groth16_setup(self.h, C.byref(d), C.byref(t), C.byref(h), ped, C.byref(vk)))
        vkd = {n: np.array(getattr(vk, n), dtype=np.uint64) for n in ("alpha1", "beta2", "gamma2", "delta2")}
        vkd["k"] = vk_k[:int(vk.n_k)].copy()
        return h, [C.c_void_p(ped[i]) for i in range(int(d.n_commitments))], vkd

    # ---- proving keys as files (include/mi355x_groth16_keyfile.h)
    def decompress_dev(self, bytes_ptr, n, out_ptr, g2=False, flags=0):
        """mi_g1_decompress_dev / mi_g2_decompress_dev over device pointers -> (rc, lowest bad index or NO_BAD_INDEX)"""
        first = C.c_uint64()
        if g2:
            rc = self.lib.mi_g2_decompress_dev(self.h, _p(bytes_ptr), C.c_size_t(n), C.c_uint32(flags), _p(out_ptr), C.byref(first))
        else:
            rc = self.lib.mi_g1_decompress_dev(self.h, _p(bytes_ptr), C.c_size_t(n), _p(out_ptr), C.byref(first))
        return rc, int(first.value)

    def compress_dev(self, pts_ptr, n, bytes_ptr, g2=False, encoding=KEYFILE_COMPRESSED):
        f = self.lib.mi_g2_compress_dev if g2 else self.lib.mi_g1_compress_dev
        self._ck(f(self.h, _p(pts_ptr), C.c_size_t(n), C.c_uint32(encoding), _p(bytes_ptr)))

    def pk_load_stream(self, blob: bytes, nb_public, committed_wires=None, flags=0):
        """a ProvingKey.WriteRawTo or ProvingKey.WriteTo stream -> (device-resident key, [Pedersen key handles]), every point checked"""
        buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob); h = C.c_void_p()
        ped = (C.c_void_p * MAX_COMMITMENTS)(); nped = C.c_uint32()
        cw = None if committed_wires is None or not len(committed_wires) else np.ascontiguousarray(committed_wires, dtype=np.uint32)
        self._ck(self.lib.mi_pk_load_stream(self.h, buf, C.c_size_t(len(blob)), C.c_uint32(flags), C.c_uint32(nb_public), _p(cw),
                                            C.c_size_t(0 if cw is None else cw.shape[0]), C.byref(h), ped, C.byref(nped)))
        return h, [C.c_void_p(ped[i]) for i in range(nped.value)]

    def pk_write_dev(self, pk: dict, ped=(), encoding=KEYFILE_COMPRESSED, cap=None):
        """mi_pk_write_dev: pk as pk_load takes it with device_points (arrays = (device pointer, count)), ped = [(basis pointer,
        basis_exp_sigma pointer, n)] -> the stream's bytes.  cap: the room offered (default: what mi_pk_stream_size asks for)"""
        d = PkDesc(); d.log_n, d.nb_wires = pk["log_n"], pk["nb_wires"]
        for name in ("g1_a", "g1_b", "g1_k", "g1_z", "g2_b"):
            ptr, cnt = pk[name]
            setattr(d, name, int(ptr)); setattr(d, "n_" + name, int(cnt))
        for name, k in (("alpha1", 8), ("beta1", 8), ("delta1", 8), ("beta2", 16), ("delta2", 16)):
            setattr(d, name, (C.c_uint64 * k)(*[int(v) for v in _u64(pk[name]).reshape(-1)]))
        ia = np.ascontiguousarray(pk["infinity_a"], dtype=np.uint8); ib = np.ascontiguousarray(pk["infinity_b"], dtype=np.uint8)
        d.infinity_a, d.infinity_b = ia.ctypes.data, ib.ctypes.data
        pa = _pedersen_arrays(list(ped)); need = C.c_size_t()
        if cap is None:
            if self.lib.mi_pk_stream_size(C.byref(d), pa, C.c_uint32(len(ped)), C.c_uint32(encoding), C.byref(need)) != 0:
                raise MiError("mi_pk_stream_size refused its arguments")
            cap = need.value
        out = (C.c_uint8 * max(cap, 1))()
        self.keyfile_len = None
        rc = self.lib.mi_pk_write_dev(self.h, C.byref(d), pa, C.c_uint32(len(ped)), C.c_uint32(encoding), out, C.c_size_t(cap), C.byref(need))
        self.keyfile_len = int(need.value)   # the size asked for, also after a refusal for want of room
        self._ck(rc)
        return C.string_at(out, need.value)

    def setup_to_stream(self, r1cs: dict, td: dict, encoding=KEYFILE_COMPRESSED, cap=1 << 24, build=True):
        """mi_groth16_setup_to_stream -> (the key's stream, key handle or None, [Pedersen key handles], vk dict as setup())"""
        d, keep = _r1cs_desc(r1cs); t = _trapdoor(td)
        n_k = int(d.nb_public) + int(d.n_commitments)
        vk_k = np.zeros((max(n_k, 1), 8), np.uint64)
        vk = VkOut(); vk.k = vk_k.ctypes.data; vk.k_cap = n_k
        h = C.c_void_p(); ped = (C.c_void_p * MAX_COMMITMENTS)(); need = C.c_size_t()
        out = (C.c_uint8 * max(cap, 1))()
        self.keyfile_len = None
        rc = self.lib.mi_groth16_setup_to_stream(self.h, C.byref(d), C.byref(t), C.c_uint32(encoding), out, C.c_size_t(cap), C.byref(need),
                                                 C.byref(h) if build else None, ped if build else None, C.byref(vk))
        self.keyfile_len = int(need.value)
        self._ck(rc)
        vkd = {n: np.array(getattr(vk, n), dtype=np.uint64) for n in ("alpha1", "beta2", "gamma2", "delta2")}
        vkd["k"] = vk_k[:int(vk.n_k)].copy()
        return C.string_at(out, need.value), (h if build else None), ([C.c_void_p(ped[i]) for i in range(int(d.n_commitments))] if build else []), vkd

    # ---- verifying keys as files (include/mi355x_groth16_vkfile.h)
    def vk_load_stream(self, blob: bytes, flags=0):
        """a VerifyingKey.WriteRawTo or VerifyingKey.WriteTo stream -> VerifyingKey, every point checked, the committed lists installed"""
        info, _ = vk_stream_inspect(blob) if len(blob) else (None, 0)
        buf = (C.c_uint8 * max(len(blob), 1)).from_buffer_copy(blob or b"\0"); h = C.c_void_p()
        self._ck(self.lib.mi_vk_load_stream(self.h, buf, C.c_size_t(len(blob)), C.c_uint32(flags), C.byref(h)))
        return VerifyingKey._adopt(self, h, int(info.nb_public), int(info.n_commitment_keys))

    def vk_write(self, vk: dict, nb_public, ped=None, lists=None, encoding=KEYFILE_COMPRESSED, cap=None):
        """mi_vk_write: the vk dict of setup() with beta1 and delta1 added -> the stream's bytes.  cap: the room offered (default: what
        mi_vk_stream_size asks for)"""
        d, keep = _vk_file_desc(vk, nb_public, ped, lists); need = C.c_size_t()
        if cap is None:
            if self.lib.mi_vk_stream_size(C.byref(d), C.c_uint32(encoding), C.byref(need)) != 0:
                raise MiError("mi_vk_stream_size refused its arguments")
            cap = need.value
        out = (C.c_uint8 * max(cap, 1))()
        self.keyfile_len = None
        rc = self.lib.mi_vk_write(self.h, C.byref(d), C.c_uint32(encoding), out, C.c_size_t(cap), C.byref(need))
        self.keyfile_len = int(need.value)   # the size asked for, also after a refusal for want of room
        self.keyfile_out = bytes(out)        # what the call left in the buffer
        self._ck(rc)
        return C.string_at(out, need.value)

    def setup_to_streams(self, r1cs: dict, td: dict, encoding=KEYFILE_COMPRESSED, cap=1 << 24, vk_cap=1 << 20, build=True):
        """mi_groth16_setup_to_streams -> (the proving key's stream, the verifying key's stream, key handle or None, [Pedersen key
        handles], vk dict as setup())"""
        d, keep = _r1cs_desc(r1cs); t = _trapdoor(td)
        n_k = int(d.nb_public) + int(d.n_commitments)
        vk_k = np.zeros((max(n_k, 1), 8), np.uint64)
        vk = VkOut(); vk.k = vk_k.ctypes.data; vk.k_cap = n_k
        h = C.c_void_p(); ped = (C.c_void_p * MAX_COMMITMENTS)(); need = C.c_size_t(); vk_need = C.c_size_t()
        out = (C.c_uint8 * max(cap, 1))(); vk_out = (C.c_uint8 * max(vk_cap, 1))()
        self.keyfile_len = self.vkfile_len = None
        rc = self.lib.mi_groth16_setup_to_streams(self.h, C.byref(d), C.byref(t), C.c_uint32(encoding), out, C.c_size_t(cap), C.byref(need),
                                                  vk_out, C.c_size_t(vk_cap), C.byref(vk_need), C.byref(h) if build else None, ped if build else None, C.byref(vk))
        self.keyfile_len, self.vkfile_len = int(need.value), int(vk_need.value)
        self._ck(rc)
        vkd = {n: np.array(getattr(vk, n), dtype=np.uint64) for n in ("alpha1", "beta2", "gamma2", "delta2")}
        vkd["k"] = vk_k[:int(vk.n_k)].copy()
        return (C.string_at(out, need.value), C.string_at(vk_out, vk_need.value), (h if build else None),
                ([C.c_void_p(ped[i]) for i in range(int(d.n_commitments))] if build else []), vkd)

    def witness_decode_dev(self, values: bytes, n, n_pub, odd=True):
        """mi_debug_witness_decode_dev over host bytes (n * n_pub values of 32 bytes, placed at an odd device address) ->
        ((n, n_pub, 4) uint64 Montgomery, (n,) uint8 bad)"""
        assert len(values) == 32 * n * n_pub
        shift = 1 if odd else 0
        de = self.to_dev(np.frombuffer(b"\0" * shift + values + b"\0" * 32, np.uint8)); do = self.alloc(max(32 * n * n_pub, 32)); db = self.to_dev(np.zeros(max(n, 32), np.uint8))
        try:
            self._ck(self.lib.mi_debug_witness_decode_dev(self.h, C.c_void_p(int(de.ptr) + shift), C.c_size_t(n), C.c_uint32(n_pub), _p(do.ptr), _p(db.ptr)))
            self.sync()
            return do.download((n, n_pub, 4)) if n * n_pub else np.zeros((n, n_pub, 4), np.uint64), db.download((max(n, 32),), np.uint8)[:n]
        finally:
            for b in (de, do, db): b.free()

    # ---- the keys from a powers-of-tau SRS (include/mi355x_groth16_phase2.h)
    def phase2_init(self, r1cs: dict, srs: dict, sigma=(), flags=0):
        """mi_phase2_init: the dict setup() takes, the SRS rows (_srs_desc), one sigma per commitment -> the ceremony state's handle"""
        d, keep = _r1cs_desc(r1cs); sd, keep2 = _srs_desc(srs); h = C.c_void_p()
        sg = _u64(np.array(sigma, np.uint64).reshape(-1, 4)) if len(sigma) else None
        self._ck(self.lib.mi_phase2_init(self.h, C.byref(d), C.byref(sd), _p(sg), C.c_uint32(flags), C.byref(h)))
        return h

    def phase2_contribute(self, st, delta, sigma_factor=None):
        sf = None if sigma_factor is None else _u64(np.array(sigma_factor, np.uint64).reshape(-1, 4))
        self._ck(self.lib.mi_phase2_contribute(self.h, st, _p(_u64(delta)), _p(sf)))

    def phase2_seal(self, st, n_k, n_commitments=0):
        """mi_phase2_seal -> (key handle, [Pedersen key handles], vk dict as setup()); n_k = nb_public + n_commitments"""
        vk_k = np.zeros((max(n_k, 1), 8), np.uint64)
        vk = VkOut(); vk.k = vk_k.ctypes.data; vk.k_cap = n_k
        h = C.c_void_p(); ped = (C.c_void_p * MAX_COMMITMENTS)()
        self._ck(self.lib.mi_phase2_seal(self.h, st, C.byref(h), ped, C.byref(vk)))
        vkd = {n: np.array(getattr(vk, n), dtype=np.uint64) for n in ("alpha1", "beta2", "gamma2", "delta2")}
        vkd["k"] = vk_k[:int(vk.n_k)].copy()
        return h, [C.c_void_p(ped[i]) for i in range(n_commitments)], vkd

    def phase2_to_streams(self, st, encoding=KEYFILE_COMPRESSED, cap=1 << 24, vk_cap=1 << 20):
        """mi_phase2_to_streams -> (the proving key's stream, the verifying key's stream)"""
        need = C.c_size_t(); vk_need = C.c_size_t()
        out = (C.c_uint8 * max(cap, 1))(); vk_out = (C.c_uint8 * max(vk_cap, 1))()
        self.keyfile_len = self.vkfile_len = None
        rc = self.lib.mi_phase2_to_streams(self.h, st, C.c_uint32(encoding), out, C.c_size_t(cap), C.byref(need), vk_out, C.c_size_t(vk_cap), C.byref(vk_need))
        self.keyfile_len, self.vkfile_len = int(need.value), int(vk_need.value)
        self._ck(rc)
        return C.string_at(out, need.value), C.string_at(vk_out, vk_need.value)

    def phase2_array(self, st, which):
        """mi_phase2_get_array: one array of the state -> (n, 8) or (n, 16) uint64"""
        n = C.c_uint64()
        self._ck(self.lib.mi_phase2_get_array(self.h, st, C.c_uint32(which), None, C.c_uint64(0), C.byref(n)))
        out = np.zeros((int(n.value), 16 if which == PHASE2_G2_B else 8), np.uint64)
        self._ck(self.lib.mi_phase2_get_array(self.h, st, C.c_uint32(which), _p(out) if n.value else None, n, C.byref(n)))
        return out

    def phase2_free(self, st):
        self._ck(self.lib.mi_phase2_free(self.h, st))

    def phase2_stats(self):
        st = Phase2Stats(); self._ck(self.lib.mi_phase2_get_stats(self.h, C.byref(st)))
        return {n: getattr(st, n) for n, _ in Phase2Stats._fields_ if n != "pad_"}

    # ---- the checks of a ceremony (include/mi355x_groth16_phase2_check.h)
    def srs_check_powers(self, srs: dict, n_domain, seed=None, flags=0):
        """mi_srs_check_powers -> the mask of relations that do not hold; seed: 32 bytes, or None for the operating system's"""
        sd, keep = _srs_desc(srs); failed = C.c_uint32(0xFFFFFFFF)
        self._ck(self.lib.mi_srs_check_powers(self.h, C.byref(sd), C.c_uint64(n_domain), seed, C.c_uint32(flags), C.byref(failed)))
        return int(failed.value)

    def srs_check_stats(self, verify=False):
        """mi_srs_check_get_stats, or with verify mi_phase2_verify_get_stats"""
        st = SrsCheckStats(); self._ck((self.lib.mi_phase2_verify_get_stats if verify else self.lib.mi_srs_check_get_stats)(self.h, C.byref(st)))
        return {n: getattr(st, n) for n, _ in SrsCheckStats._fields_ if n != "pad_"}

    def ceremony_coeffs(self, seed, n):
        """mi_debug_ceremony_coeffs_dev -> (n, 4) uint64, Montgomery"""
        out = self.alloc(max(n, 1) * 32)
        try:
            self._ck(self.lib.mi_debug_ceremony_coeffs_dev(self.h, seed, C.c_size_t(n), C.c_void_p(out.ptr)))
            return out.download((n, 4), np.uint64)
        finally:
            out.free()

    def phase2_set_transcript_id(self, st, ident):
        self._ck(self.lib.mi_phase2_set_transcript_id(self.h, st, ident))

    def phase2_contribute_proved(self, st, delta, nonce=None):
        """mi_phase2_contribute_proved -> the record, PHASE2_RECORD_WORDS uint64"""
        rec = np.zeros(PHASE2_RECORD_WORDS, np.uint64)
        self._ck(self.lib.mi_phase2_contribute_proved(self.h, st, _p(_u64(delta)), None if nonce is None else _p(_u64(nonce)), _p(rec)))
        return rec

    def phase2_verify_adopt(self, st, g1_z, g1_k, delta1, delta2, records, seed=None):
        """mi_phase2_verify_adopt -> (mask, first_bad_record); records: (m, PHASE2_RECORD_WORDS) uint64"""
        z, k, rec = _u64(g1_z), _u64(g1_k), _u64(records).reshape(-1, PHASE2_RECORD_WORDS)
        cl = Phase2Claim(z.ctypes.data, z.shape[0], k.ctypes.data if k.shape[0] else None, k.shape[0], (C.c_uint64 * 8)(*[int(v) for v in _u64(delta1).reshape(8)]),
                         (C.c_uint64 * 16)(*[int(v) for v in _u64(delta2).reshape(16)]))
        failed = C.c_uint32(0xFFFFFFFF); fb = C.c_uint64(0)
        self._ck(self.lib.mi_phase2_verify_adopt(self.h, st, C.byref(cl), _p(rec), C.c_size_t(rec.shape[0]), seed, C.byref(failed), C.byref(fb)))
        return int(failed.value), int(fb.value)

    def phase2_get_pedersen_vk(self, st, n_commitments):
        """mi_phase2_get_pedersen_vk -> (n_commitments, 2, 16) uint64 as pedersen_vk_make: {g2, [-sigma_k]2} of the state's points"""
        out = np.zeros((n_commitments, 2, 16), np.uint64)
        self._ck(self.lib.mi_phase2_get_pedersen_vk(self.h, st, _p(out) if n_commitments else None))
        return out

    def phase2_contribute_sigma_proved(self, st, sigma_factor, nonce=None):
        """mi_phase2_contribute_sigma_proved -> (the step: (n_commitments, PHASE2_SIGMA_PROOF_WORDS) uint64, the chain value after it)"""
        sf = _u64(sigma_factor).reshape(-1, 4); out = np.zeros((sf.shape[0], PHASE2_SIGMA_PROOF_WORDS), np.uint64); h = (C.c_uint8 * 32)()
        self._ck(self.lib.mi_phase2_contribute_sigma_proved(self.h, st, _p(sf), None if nonce is None else _p(_u64(nonce).reshape(-1, 4)), _p(out), h))
        return out, bytes(h)

    def phase2_chain_info(self, st):
        """mi_phase2_get_chain_info -> {n_commitments, n_records, chain, n_sigma_records, sigma_chain}: where the delta and the sigma chain stand"""
        info = Phase2ChainInfo(); self._ck(self.lib.mi_phase2_get_chain_info(self.h, st, C.byref(info)))
        return {"n_commitments": int(info.n_commitments), "n_records": int(info.n_records), "chain": bytes(info.chain),
                "n_sigma_records": int(info.n_sigma_records), "sigma_chain": bytes(info.sigma_chain)}

    def phase2_verify_adopt_sigma(self, st, basis_exp_sigma, g_sigma_neg, proofs, hashes, seed=None):
        """mi_phase2_verify_adopt_sigma -> (mask, bad_commitments, first_bad_record); basis_exp_sigma: one (n_k, 8) array per commitment,
        g_sigma_neg: (n_commitments, 16), proofs: (m, n_commitments, PHASE2_SIGMA_PROOF_WORDS), hashes: m chain values"""
        bes = [_u64(a) for a in basis_exp_sigma]; nc = len(bes)
        ptrs = (C.c_void_p * max(nc, 1))(*[a.ctypes.data if a.shape[0] else None for a in bes])
        counts = (C.c_uint64 * max(nc, 1))(*[a.shape[0] for a in bes])
        gs = _u64(g_sigma_neg).reshape(-1, 16)
        pr, hs, m = _sigma_steps(proofs, hashes, max(nc, 1))
        cl = Phase2SigmaClaim(C.cast(ptrs, C.c_void_p), C.cast(counts, C.c_void_p), gs.ctypes.data)
        failed = C.c_uint32(0xFFFFFFFF); bad = C.c_uint64(0); fb = C.c_uint64(0)
        self._ck(self.lib.mi_phase2_verify_adopt_sigma(self.h, st, C.byref(cl), _p(pr), hs, C.c_size_t(m), seed, C.byref(failed), C.byref(bad), C.byref(fb)))
        return int(failed.value), int(bad.value), int(fb.value)

    # ---- phase 1: the SRS itself (include/mi355x_groth16_phase1.h)
    # ---- a key audited against its circuit and an SRS (include/mi355x_groth16_keyaudit.h)
    def key_claim_from_streams(self, pk_blob: bytes, vk_blob: bytes, flags=0):
        """mi_key_claim_from_streams: both of a key's streams, either encoding -> the claim's handle"""
        pb = (C.c_uint8 * max(len(pk_blob), 1)).from_buffer_copy(pk_blob or b"\0"); vb = (C.c_uint8 * max(len(vk_blob), 1)).from_buffer_copy(vk_blob or b"\0")
        h = C.c_void_p()
        self._ck(self.lib.mi_key_claim_from_streams(self.h, pb, C.c_size_t(len(pk_blob)), vb, C.c_size_t(len(vk_blob)), C.c_uint32(flags), C.byref(h)))
        return h

    def key_claim_from_phase2(self, st):
        """mi_key_claim_from_phase2: the claim borrows the state's arrays; free it before the state"""
        h = C.c_void_p()
        self._ck(self.lib.mi_key_claim_from_phase2(self.h, st, C.byref(h)))
        return h

    def key_claim_from_arrays(self, pk: dict, ped, vk: dict, vk_ped=None, n_vk=None):
        """mi_key_claim_from_arrays: pk as pk_write_dev takes it (arrays = (device pointer, count)), ped = [(basis pointer, basis_exp_sigma
        pointer, n)], vk = the dict setup() returns, vk_ped = (n_commitments, 2, 16) as pedersen_vk_make -> the claim's handle"""
        d = PkDesc(); d.log_n, d.nb_wires, d.nb_public = int(pk.get("log_n", 0)), int(pk["nb_wires"]), int(pk.get("nb_public", 0))
        for name in ("g1_a", "g1_b", "g1_k", "g1_z", "g2_b"):
            ptr, cnt = pk[name]
            setattr(d, name, int(ptr) if ptr else None); setattr(d, "n_" + name, int(cnt))
        for name, k in (("alpha1", 8), ("beta1", 8), ("delta1", 8), ("beta2", 16), ("delta2", 16)):
            setattr(d, name, (C.c_uint64 * k)(*[int(v) for v in _u64(pk[name]).reshape(-1)]))
        ia = np.ascontiguousarray(pk["infinity_a"], dtype=np.uint8); ib = np.ascontiguousarray(pk["infinity_b"], dtype=np.uint8)
        d.infinity_a, d.infinity_b = ia.ctypes.data, ib.ctypes.data
        vd = VkDesc()
        for n, w in (("alpha1", 8), ("beta2", 16), ("gamma2", 16), ("delta2", 16)):
            setattr(vd, n, (C.c_uint64 * w)(*[int(v) for v in _u64(vk[n]).reshape(w)]))
        k = _u64(vk["k"]).reshape(-1, 8)
        vp = None if vk_ped is None or not len(vk_ped) else _u64(vk_ped).reshape(-1, 2, 16)
        vd.k, vd.n_k = k.ctypes.data, int(k.shape[0] if n_vk is None else n_vk)
        vd.n_commitments = 0 if vp is None else int(vp.shape[0])
        vd.nb_public = max(int(vd.n_k) - int(vd.n_commitments), 0)
        vd.ped = None if vp is None else vp.ctypes.data
        h = C.c_void_p()
        self._ck(self.lib.mi_key_claim_from_arrays(self.h, C.byref(d), _pedersen_arrays(list(ped)), C.c_uint32(len(ped)), C.byref(vd), C.byref(h)))
        return h

    def key_claim_free(self, claim):
        self._ck(self.lib.mi_key_claim_free(self.h, claim))

    def key_audit(self, r1cs: dict, claim, srs=None, p1=None, seed=None, flags=0):
        """mi_key_audit -> the mask of relations that do not hold.  srs: the rows as a dict (_srs_desc), or p1: a phase-1 state's handle;
        seed: 32 bytes, or None for the operating system's"""
        d, keep = _r1cs_desc(r1cs); failed = C.c_uint32()
        sd, keep2 = _srs_desc(srs) if srs is not None else (None, None)
        self._ck(self.lib.mi_key_audit(self.h, C.byref(d), None if sd is None else C.byref(sd), p1, claim, seed, C.c_uint32(flags), C.byref(failed)))
        return int(failed.value)

    def key_audit_stats(self):
        st = KeyAuditStats(); self._ck(self.lib.mi_key_audit_get_stats(self.h, C.byref(st)))
        return {n: getattr(st, n) for n, _ in KeyAuditStats._fields_}

    def key_audit_sums(self):
        """mi_debug_key_audit_sums -> {relation: (2, 8) or (2, 16) uint64: the key's side, the SRS's side; "sigma": (n, 2, 8)}"""
        s = KeyAuditSums(); self._ck(self.lib.mi_debug_key_audit_sums(self.h, C.byref(s)))
        out = {n: np.array(getattr(s, n), dtype=np.uint64) for n in ("a", "b1", "k_private", "k_public", "basis", "z", "b2")}
        out["sigma"] = np.array(s.sigma, dtype=np.uint64)[:int(s.n_sigma)]
        return out

    def phase1_init(self, log_n):
        """mi_phase1_init -> the state's handle: every row the generator"""
        h = C.c_void_p()
        self._ck(self.lib.mi_phase1_init(self.h, C.c_uint32(log_n), C.byref(h)))
        return h

    def phase1_from_srs(self, srs: dict, n_domain, flags=0):
        """mi_phase1_from_srs: the SRS rows (_srs_desc) taken in -> the state's handle"""
        sd, keep = _srs_desc(srs); h = C.c_void_p()
        self._ck(self.lib.mi_phase1_from_srs(self.h, C.byref(sd), C.c_uint64(n_domain), C.c_uint32(flags), C.byref(h)))
        return h

    def phase1_set_transcript_id(self, st, ident):
        self._ck(self.lib.mi_phase1_set_transcript_id(self.h, st, ident))

    def phase1_contribute(self, st, tau, alpha, beta):
        """mi_phase1_contribute: tau, alpha, beta (4,) uint64 Montgomery (None passes a null pointer)"""
        self._ck(self.lib.mi_phase1_contribute(self.h, st, *(None if v is None else _p(_u64(v)) for v in (tau, alpha, beta))))

    def phase1_contribute_proved(self, st, tau, alpha, beta, nonce=None):
        """mi_phase1_contribute_proved -> the record, PHASE1_RECORD_WORDS uint64; nonce: (3, 4) uint64 Montgomery, or None for the operating system's"""
        rec = np.zeros(PHASE1_RECORD_WORDS, np.uint64)
        nn = None if nonce is None else _u64(np.array(nonce, np.uint64).reshape(3, 4))
        self._ck(self.lib.mi_phase1_contribute_proved(self.h, st, *(None if v is None else _p(_u64(v)) for v in (tau, alpha, beta)), _p(nn), _p(rec)))
        return rec

    def phase1_verify_adopt(self, st, claim: dict, records, seed=None):
        """mi_phase1_verify_adopt: claim as _srs_desc takes it -> (mask, first_bad_record); records: (m, PHASE1_RECORD_WORDS) uint64"""
        sd, keep = _srs_desc(claim); rec = _u64(records).reshape(-1, PHASE1_RECORD_WORDS)
        failed = C.c_uint32(0xFFFFFFFF); fb = C.c_uint64(0)
        self._ck(self.lib.mi_phase1_verify_adopt(self.h, st, C.byref(sd), _p(rec) if rec.shape[0] else None, C.c_size_t(rec.shape[0]), seed, C.byref(failed), C.byref(fb)))
        return int(failed.value), int(fb.value)

    def phase1_check(self, st, seed=None):
        """mi_phase1_check -> the SRS_BAD_* mask of the state's own rows"""
        failed = C.c_uint32(0xFFFFFFFF)
        self._ck(self.lib.mi_phase1_check(self.h, st, seed, C.byref(failed)))
        return int(failed.value)

    def phase1_info(self, st):
        """mi_phase1_get_info -> log_n, n_records, chain (32 bytes), tau1 / alpha1 / beta1 (8,) uint64"""
        i = Phase1Info(); self._ck(self.lib.mi_phase1_get_info(self.h, st, C.byref(i)))
        return {"log_n": int(i.log_n), "n_records": int(i.n_records), "chain": bytes(i.chain),
                **{n: np.array(getattr(i, n), dtype=np.uint64) for n in ("tau1", "alpha1", "beta1")}}

    def phase1_export(self, st, caps=None):
        """mi_phase1_export -> the rows as the dict _srs_desc takes; caps: four capacities in place of the rows' own sizes (for the refusals)"""
        n = (C.c_uint64 * 4)()
        self._ck(self.lib.mi_phase1_export(self.h, st, None, None, None, None, None, *(C.c_uint64(0),) * 4, n))
        cnt = [int(v) for v in n]
        rows = [np.zeros((c, w), np.uint64) for c, w in zip(cnt, (8, 8, 8, 16))]
        b2 = np.zeros(16, np.uint64)
        self._ck(self.lib.mi_phase1_export(self.h, st, *(_p(r) for r in rows), _p(b2), *(C.c_uint64(c) for c in (caps or cnt)), n))
        return {"tau_g1": rows[0], "alpha_tau_g1": rows[1], "beta_tau_g1": rows[2], "tau_g2": rows[3], "beta_g2": b2}

    def phase1_free(self, st):
        self._ck(self.lib.mi_phase1_free(self.h, st))

    def phase1_stats(self):
        st = Phase1Stats(); self._ck(self.lib.mi_phase1_get_stats(self.h, C.byref(st)))
        return {"scalar_mul_ms": list(st.scalar_mul_ms), "affine_ms": list(st.affine_ms), "total_ms": st.total_ms, "window": st.window, "chunk": st.chunk,
                "peak_bytes": st.peak_bytes}

    def phase2_init_from_phase1(self, r1cs: dict, p1, sigma=(), flags=0):
        """mi_phase2_init_from_phase1: phase2_init with the SRS rows read from a phase-1 state's device arrays"""
        d, keep = _r1cs_desc(r1cs); h = C.c_void_p()
        sg = _u64(np.array(sigma, np.uint64).reshape(-1, 4)) if len(sigma) else None
        self._ck(self.lib.mi_phase2_init_from_phase1(self.h, C.byref(d), p1, _p(sg), C.c_uint32(flags), C.byref(h)))
        return h

    def debug_scale_powers(self, pts, t, c, k0=0, g2=False):
        """mi_debug_scale_powers_dev: out[i] = [c t^(k0 + i)] pts[i] by the driver a phase-1 contribution runs -> (n, 8) or (n, 16) uint64"""
        p = _u64(pts).reshape(-1, 16 if g2 else 8); out = np.zeros_like(p)
        self._ck(self.lib.mi_debug_scale_powers_dev(self.h, C.c_int32(1 if g2 else 0), _p(p) if p.shape[0] else None, C.c_size_t(p.shape[0]), _p(_u64(t)), _p(_u64(c)),
                                                    C.c_uint64(k0), _p(out) if p.shape[0] else None))
        return out

    def keyfile_stats(self):
        st = KeyfileStats(); self._ck(self.lib.mi_keyfile_get_stats(self.h, C.byref(st)))
        return {n: getattr(st, n) for n, _ in KeyfileStats._fields_}

    def setup_stats(self):
        st = SetupStats(); self._ck(self.lib.mi_groth16_setup_get_stats(self.h, C.byref(st)))
        return {n: getattr(st, n) for n, _ in SetupStats._fields_}

    # ---- the device-resident R1CS (include/mi355x_groth16_r1cs.h)
    def r1cs_load(self, r1cs: dict):
        """mi_r1cs_load: the dict setup() takes -> handle of the resident R1CS (shared by every context of this device)"""
        d, keep = _r1cs_desc(r1cs); h = C.c_void_p()
        self._ck(self.lib.mi_r1cs_load(self.h, C.byref(d), C.byref(h)))
        return h

    def r1cs_free(self, rh):
        self._ck(self.lib.mi_r1cs_free(self.h, rh))

    def r1cs_bytes(self, rh):
        v = C.c_uint64(); self._ck(self.lib.mi_r1cs_bytes(rh, C.byref(v))); return int(v.value)

    def r1cs_eval(self, rh, W, n_constraints, which=R1CS_A | R1CS_B | R1CS_C, device=False):
        """(A W, B W, C W), None for a matrix not in `which`; W: (nb_wires, 4) host array, or a device pointer with device=True (the
        outputs then go through device buffers of the call's own: mi_r1cs_eval_dev)"""
        outs = [np.zeros((n_constraints, 4), np.uint64) if which & (1 << k) else None for k in range(3)]
        if not device:
            self._ck(self.lib.mi_r1cs_eval(self.h, rh, _p(_u64(W)), C.c_uint32(which), *[_p(o) for o in outs]))
            return tuple(outs)
        bufs = [self.alloc(32 * n_constraints + 32) if o is not None else None for o in outs]
        try:
            self._ck(self.lib.mi_r1cs_eval_dev(self.h, rh, _p(W), C.c_uint32(which), *[_p(b.ptr if b else None) for b in bufs]))
            self.sync()
            return tuple(None if b is None else b.download((n_constraints, 4)) for b in bufs)
        finally:
            for b in bufs:
                if b: b.free()

    def r1cs_check(self, rh, W, device=False):
        """mi_r1cs_check_dev -> (rows with (A W)(B W) != C W, the lowest of them or 2^64 - 1); W as in r1cs_eval"""
        n_bad, first = C.c_uint64(), C.c_uint64()
        d = None if device else self.to_dev(_u64(W))
        try:
            self._ck(self.lib.mi_r1cs_check_dev(self.h, rh, _p(W if device else d.ptr), C.byref(n_bad), C.byref(first)))
        finally:
            if d: d.free()
        return int(n_bad.value), int(first.value)

    def r1cs_stats(self):
        st = R1csStats(); self._ck(self.lib.mi_r1cs_get_stats(self.h, C.byref(st)))
        return {n: getattr(st, n) for n, _ in R1csStats._fields_}

    def prove_w(self, pkh, rh, W, r, s, flags=0, device=False, n_wires=None):
        """mi_groth16_prove_w[_dev]: the proof from the wire vector alone"""
        out = np.zeros(32, np.uint64); st = Stats()
        r, s = _u64(r), _u64(s)
        if device:
            self._ck(self.lib.mi_groth16_prove_w_dev(self.h, pkh, rh, _p(W), C.c_size_t(n_wires), C.c_uint32(flags), _p(r), _p(s), _p(out), C.byref(st)))
        else:
            W = _u64(W)
            self._ck(self.lib.mi_groth16_prove_w(self.h, pkh, rh, _p(W), C.c_size_t(W.shape[0] if n_wires is None else n_wires), C.c_uint32(flags),
                                                 _p(r), _p(s), _p(out), C.byref(st)))
        return {"ar": out[:8].copy(), "bs": out[8:24].copy(), "krs": out[24:].copy(), "raw": out}, st.as_dict()

    # ---- groth16.Verify on the device (include/mi355x_groth16_verify.h)
    def pedersen_vk_make(self, sigmas):
        """mi_pedersen_vk_make: (n, 4) Montgomery sigma rows -> (n, 2, 16) uint64: G and GSigmaNeg of each commitment"""
        sg = _u64(sigmas).reshape(-1, 4); n = sg.shape[0]
        out = np.zeros((n, 2, 16), np.uint64)
        self._ck(self.lib.mi_pedersen_vk_make(self.h, _p(sg), C.c_uint32(n), _p(out)))
        return out

    def vk_load(self, vk: dict, nb_public, ped=None, n_k=None):
        """mi_vk_load: the vk dict setup() returns (alpha1, beta2, gamma2, delta2, k), nb_public (with the ONE wire) and the Pedersen
        verifying keys ((n_commitments, 2, 16), as pedersen_vk_make) -> VerifyingKey"""
        return VerifyingKey(self, vk, nb_public, ped, n_k)

    def pairing(self, p, q, final_exp=True):
        """mi_debug_pairing_dev over host arrays: (n, 8) G1 and (n, 16) G2 points -> (n, 48) uint64, 12 x mi_fp per pair"""
        p, q = _u64(p).reshape(-1, 8), _u64(q).reshape(-1, 16); n = p.shape[0]
        dp, dq = self.to_dev(p), self.to_dev(q); do = self.alloc(max(384 * n, 32))
        try:
            self._ck(self.lib.mi_debug_pairing_dev(self.h, _p(dp.ptr), _p(dq.ptr), C.c_size_t(n), _p(do.ptr), C.c_uint32(PAIRING_FINAL_EXP if final_exp else 0)))
            self.sync()
            return do.download((n, 48)) if n else np.zeros((0, 48), np.uint64)
        finally:
            for b in (dp, dq, do): b.free()

    def fp12_op(self, op, x, y=None):
        """mi_debug_fp12_op_dev over host arrays of (n, 48) uint64 records (csrc/pairing_ops.cuh)"""
        x = _u64(x).reshape(-1, 48); n = x.shape[0]
        dx = self.to_dev(x); dy = self.to_dev(_u64(y).reshape(-1, 48)) if y is not None else None; dz = self.alloc(max(384 * n, 32))
        try:
            self._ck(self.lib.mi_debug_fp12_op_dev(self.h, C.c_int(op), _p(dz.ptr), _p(dx.ptr), _p(dy.ptr if dy else None), C.c_size_t(n)))
            self.sync()
            return dz.download((n, 48)) if n else np.zeros((0, 48), np.uint64)
        finally:
            for b in (dx, dy, dz):
                if b: b.free()

    def pairing_wave(self, p, q, final_exp=True):
        """mi_debug_pairing_wave_dev: pairing() with one wave per pair"""
        p, q = _u64(p).reshape(-1, 8), _u64(q).reshape(-1, 16); n = p.shape[0]
        dp, dq = self.to_dev(p), self.to_dev(q); do = self.alloc(max(384 * n, 32))
        try:
            self._ck(self.lib.mi_debug_pairing_wave_dev(self.h, _p(dp.ptr), _p(dq.ptr), C.c_size_t(n), _p(do.ptr), C.c_uint32(PAIRING_FINAL_EXP if final_exp else 0)))
            self.sync()
            return do.download((n, 48)) if n else np.zeros((0, 48), np.uint64)
        finally:
            for b in (dp, dq, do): b.free()

    def fp12_op_wave(self, op, x, y=None):
        """mi_debug_fp12_op_wave_dev: fp12_op() with one wave per record"""
        x = _u64(x).reshape(-1, 48); n = x.shape[0]
        dx = self.to_dev(x); dy = self.to_dev(_u64(y).reshape(-1, 48)) if y is not None else None; dz = self.alloc(max(384 * n, 32))
        try:
            self._ck(self.lib.mi_debug_fp12_op_wave_dev(self.h, C.c_int(op), _p(dz.ptr), _p(dx.ptr), _p(dy.ptr if dy else None), C.c_size_t(n)))
            self.sync()
            return dz.download((n, 48)) if n else np.zeros((0, 48), np.uint64)
        finally:
            for b in (dx, dy, dz):
                if b: b.free()

    def fp12_product(self, x):
        """mi_debug_fp12_product_dev over a host array of (n, 48) uint64 records -> (48,): their product"""
        x = _u64(x).reshape(-1, 48); n = x.shape[0]
        dx = self.to_dev(x); do = self.alloc(384)
        try:
            self._ck(self.lib.mi_debug_fp12_product_dev(self.h, _p(dx.ptr), C.c_size_t(n), _p(do.ptr)))
            self.sync()
            return do.download((48,))
        finally:
            for b in (dx, do): b.free()

    def g1_scale128(self, pts, ks):
        """mi_debug_g1_scale128_dev: (n, 8) G1 points and n plain integers below 2^128 -> (n, 8): ks[i] * pts[i], affine"""
        pts = _u64(pts).reshape(-1, 8); n = pts.shape[0]
        assert len(ks) == n and n and all(0 <= int(k) < 1 << 128 for k in ks)
        kk = np.array([[int(k) & (1 << 64) - 1, int(k) >> 64] for k in ks], np.uint64)
        dp, dk = self.to_dev(pts), self.to_dev(kk); do = self.alloc(64 * n)
        try:
            self._ck(self.lib.mi_debug_g1_scale128_dev(self.h, _p(dp.ptr), _p(dk.ptr), C.c_size_t(n), _p(do.ptr)))
            self.sync()
            return do.download((n, 8))
        finally:
            for b in (dp, dk, do): b.free()

    def g1_sum_tree(self, pts):
        """mi_debug_g1_sum_tree_dev: (n, 8) G1 points -> every level above them of the sum tree of fan-in 8, level 1 first"""
        pts = _u64(pts).reshape(-1, 8); n = pts.shape[0]
        m, total = n, 0
        while True:
            m = (m + 7) // 8; total += m
            if m <= 1:
                break
        dp = self.to_dev(pts); do = self.alloc(64 * total)
        try:
            self._ck(self.lib.mi_debug_g1_sum_tree_dev(self.h, _p(dp.ptr), C.c_size_t(n), _p(do.ptr)))
            self.sync()
            return do.download((total, 8))
        finally:
            for b in (dp, do): b.free()

    def locate_points(self, rs, krs, cm=None, pok=None, fold=None):
        """mi_debug_locate_points_dev: n plain integers below 2^128, (n, 8) Krs, (n, nc, 8) commitments, (n, 8) pok, (n, 4) fold challenges
        -> (arrays, n, 8): r Krs | r sum_k C_k | r pok | (r c^k) C_k per k (the last with nc > 1 only)"""
        krs = _u64(krs).reshape(-1, 8); n = krs.shape[0]
        nc = 0 if cm is None else _u64(cm).reshape(n, -1, 8).shape[1]
        na = 1 + (2 if nc else 0) + (nc if nc > 1 else 0)
        kk = np.array([[int(k) & (1 << 64) - 1, int(k) >> 64] for k in rs], np.uint64)
        bufs = [self.to_dev(kk), self.to_dev(krs), self.to_dev(_u64(cm)) if nc else None, self.to_dev(_u64(pok)) if nc else None,
                self.to_dev(_u64(fold)) if nc > 1 else None, self.alloc(64 * na * n)]
        try:
            ptr = [_p(b.ptr) if b else None for b in bufs]
            self._ck(self.lib.mi_debug_locate_points_dev(self.h, ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], C.c_uint32(nc), C.c_size_t(n), ptr[5]))
            self.sync()
            return bufs[5].download((na, n, 8))
        finally:
            for b in bufs:
                if b: b.free()

    def locate_colsums(self, scal, rs, level, nodes):
        """mi_debug_locate_colsums_dev: (n, ns, 4) Montgomery scalars, n plain integers below 2^128, the nodes of one level of the tree over
        n proofs -> (m, ns + 1, 4): per node the sums of r_i scal[i, j] over its proofs, the last column the sum of the r_i"""
        n = len(rs)
        scal = _u64(scal).reshape(n, -1, 4); ns = scal.shape[1]
        rr = np.zeros((n, 4), np.uint64)
        rr[:, 0] = [int(k) & (1 << 64) - 1 for k in rs]; rr[:, 1] = [int(k) >> 64 for k in rs]
        nd = np.ascontiguousarray(nodes, np.uint32); m = len(nd)
        bufs = [self.to_dev(scal) if ns else None, self.to_dev(rr), self.to_dev(nd), self.alloc(32 * m * (ns + 1))]
        try:
            self._ck(self.lib.mi_debug_locate_colsums_dev(self.h, _p(bufs[0].ptr) if ns else None, C.c_uint32(ns), _p(bufs[1].ptr), C.c_size_t(n),
                                                          C.c_uint32(level), _p(bufs[2].ptr), C.c_size_t(m), _p(bufs[3].ptr)))
            self.sync()
            return bufs[3].download((m, ns + 1, 4))
        finally:
            for b in bufs:
                if b: b.free()

    def set_locate_round_nodes(self, cap=0):
        """mi_debug_set_locate_round_nodes: the node budget of a round of verify_locate's descent; 0 = the default"""
        self._ck(self.lib.mi_debug_set_locate_round_nodes(self.h, C.c_uint32(cap)))

    def decode_points(self, enc: bytes, g2=False):
        """mi_debug_decode_g1_dev / _g2_dev over host bytes: n encodings of 32 (64) bytes -> ((n, 8) or (n, 16) uint64, (n,) uint8 malformed)"""
        w = 64 if g2 else 32
        assert len(enc) % w == 0
        n = len(enc) // w
        if not n:
            return np.zeros((0, w // 4), np.uint64), np.zeros(0, np.uint8)
        de = self.to_dev(np.frombuffer(enc, np.uint8)); do = self.alloc(n * w * 2); db = self.alloc(max(n, 32))
        try:
            fn = self.lib.mi_debug_decode_g2_dev if g2 else self.lib.mi_debug_decode_g1_dev
            self._ck(fn(self.h, _p(de.ptr), C.c_size_t(n), _p(do.ptr), _p(db.ptr)))
            self.sync()
            return do.download((n, w // 4)), db.download((n,), np.uint8)
        finally:
            for b in (de, do, db): b.free()

    def hash_to_field_dev(self, dst: bytes, msgs):
        """mi_debug_hash_to_field_dev: messages of one length and one dst -> (n, 4) uint64 Montgomery"""
        n = len(msgs); ln = len(msgs[0]) if n else 0
        assert all(len(m) == ln for m in msgs) and n
        dd = self.to_dev(np.frombuffer(dst, np.uint8)); dm = self.to_dev(np.frombuffer(b"".join(msgs) + b"\0", np.uint8)); do = self.alloc(32 * n)
        try:
            self._ck(self.lib.mi_debug_hash_to_field_dev(self.h, _p(dd.ptr), C.c_uint32(len(dst)), _p(dm.ptr), C.c_size_t(ln), C.c_size_t(n), _p(do.ptr)))
            self.sync()
            return do.download((n, 4))
        finally:
            for b in (dd, dm, do): b.free()

    def trim(self):
        """mi_ctx_trim: every grow-only workspace of this (idle) context goes back to the device"""
        self._ck(self.lib.mi_ctx_trim(self.h))

    def stats(self):
        st = Stats(); self._ck(self.lib.mi_get_stats(self.h, C.byref(st))); return st.as_dict()

    def mem_ledger(self, pkh=None):
        """device memory held by the key `pkh` and by this context, in GB (mi_get_mem_ledger)"""
        m = MemLedger(); self._ck(self.lib.mi_get_mem_ledger(self.h, pkh, C.byref(m)))
        return {n: getattr(m, n) / 1e9 for n, _ in MemLedger._fields_}


class VerifyingKey:
    """A device-resident verifying key (mi_vk).  verify / verify_batch take proofs as dicts: raw ((32,) uint64: Ar | Bs | Krs, as
    prove()'s "raw"), public_inputs ((nb_public - 1, 4) Montgomery), and with commitments: commitments (n, 8), pok (8,),
    commitment_values (n, 4), fold_challenge (4,) (optional with one commitment).  The verdict is one of VERIFY_*."""

    def __init__(self, ctx, vk, nb_public, ped=None, n_k=None):
        self.ctx = ctx
        d = VkDesc()
        for n, w in (("alpha1", 8), ("beta2", 16), ("gamma2", 16), ("delta2", 16)):
            setattr(d, n, (C.c_uint64 * w)(*[int(v) for v in _u64(vk[n]).reshape(w)]))
        k = _u64(vk["k"]).reshape(-1, 8)
        ped = None if ped is None else _u64(ped).reshape(-1, 2, 16)
        d.k, d.n_k, d.nb_public = k.ctypes.data, int(k.shape[0] if n_k is None else n_k), int(nb_public)
        d.n_commitments = 0 if ped is None else int(ped.shape[0])
        d.ped = None if ped is None else ped.ctypes.data
        self.nb_public, self.n_commitments = int(nb_public), int(d.n_commitments)
        h = C.c_void_p()
        ctx._ck(ctx.lib.mi_vk_load(ctx.h, C.byref(d), C.byref(h)))
        self.h = h

    @classmethod
    def _adopt(cls, ctx, h, nb_public, n_commitments):
        """a handle mi_vk_load_stream made"""
        self = cls.__new__(cls)
        self.ctx, self.h, self.nb_public, self.n_commitments = ctx, h, int(nb_public), int(n_commitments)
        return self

    def _inputs(self, proofs):
        arr = (VerifyInput * len(proofs))(); keep = []
        for i, pr in enumerate(proofs):
            arr[i].proof = (C.c_uint64 * 32)(*[int(v) for v in _u64(pr["raw"]).reshape(32)])
            for name in ("commitments", "pok", "public_inputs", "commitment_values", "fold_challenge"):
                v = pr.get(name)
                if v is not None:
                    v = _u64(v); keep.append(v)
                    setattr(arr[i], name, v.ctypes.data)
        return arr, keep

    def verify(self, proof: dict) -> int:
        arr, keep = self._inputs([proof]); v = C.c_uint8(255)
        self.ctx._ck(self.ctx.lib.mi_groth16_verify(self.ctx.h, self.h, C.byref(arr[0]), C.byref(v)))
        return int(v.value)

    def verify_batch(self, proofs):
        arr, keep = self._inputs(list(proofs)); out = np.full(len(arr), 255, np.uint8)
        self.ctx._ck(self.ctx.lib.mi_groth16_verify_batch(self.ctx.h, self.h, arr, C.c_size_t(len(arr)), _p(out)))
        return out

    # ---- one wave per pairing: one proof, or a few (include/mi355x_groth16_verify_wave.h)
    def verify_wave(self, proofs):
        """mi_groth16_verify_wave: proofs as verify_batch takes them -> verdicts (n,) uint8"""
        arr, keep = self._inputs(list(proofs)); out = np.full(len(arr), 255, np.uint8)
        self.ctx._ck(self.ctx.lib.mi_groth16_verify_wave(self.ctx.h, self.h, arr, C.c_size_t(len(arr)), _p(out)))
        return out

    def verify_bytes_wave(self, proofs):
        """mi_groth16_verify_bytes_wave: proofs as verify_bytes_batch takes them -> verdicts (n,) uint8"""
        arr, keep = self._bytes_inputs(proofs); out = np.full(len(arr), 255, np.uint8)
        self.ctx._ck(self.ctx.lib.mi_groth16_verify_bytes_wave(self.ctx.h, self.h, arr, C.c_size_t(len(arr)), _p(out)))
        return out

    def verify_wave_split(self, proofs):
        """mi_debug_verify_wave_split -> (verdicts, {phase: ms} over VERIFY_WAVE_SPLIT_PHASES)"""
        arr, keep = self._inputs(list(proofs)); out = np.full(len(arr), 255, np.uint8); ms = (C.c_float * len(VERIFY_WAVE_SPLIT_PHASES))()
        self.ctx._ck(self.ctx.lib.mi_debug_verify_wave_split(self.ctx.h, self.h, arr, C.c_size_t(len(arr)), _p(out), ms))
        return out, dict(zip(VERIFY_WAVE_SPLIT_PHASES, (float(v) for v in ms)))

    # ---- the sums of a whole batch over the key's window table (include/mi355x_groth16_verify_ksum.h)
    def ksum_prepare(self, max_table_bytes=0):
        """mi_vk_ksum_prepare: build (or build again) the table under a byte budget, 0 = the default -> ksum_info()"""
        self.ctx._ck(self.ctx.lib.mi_vk_ksum_prepare(self.ctx.h, self.h, C.c_uint64(int(max_table_bytes))))
        return self.ksum_info()

    def ksum_info(self):
        """mi_vk_ksum_get_info -> dict: window_bits (0 = no table), windows, table_bytes, bases, budget_bytes, state (KSUM_*), build_ms"""
        info = VkKsumInfo()
        self.ctx._ck(self.ctx.lib.mi_vk_ksum_get_info(self.ctx.h, self.h, C.byref(info)))
        return info.as_dict()

    def ksum_batch_dev(self, scalars_ptr, skip_ptr, n, out_ptr):
        """mi_vk_ksum_batch_dev over raw device pointers (skip_ptr may be None); mi_dev_sync before reading"""
        self.ctx._ck(self.ctx.lib.mi_vk_ksum_batch_dev(self.ctx.h, self.h, _p(scalars_ptr), _p(skip_ptr), C.c_size_t(n), _p(out_ptr)))

    def ksum_batch(self, scalars, skip=None):
        """mi_vk_ksum_batch: scalars (n, bases, 4) Montgomery, skip (n,) uint8 or None -> (n, 8) affine points, zeros = infinity"""
        scalars = _u64(scalars); n = int(scalars.shape[0])
        skip = None if skip is None else np.ascontiguousarray(skip, np.uint8)
        out = np.zeros((n, 8), np.uint64)
        self.ctx._ck(self.ctx.lib.mi_vk_ksum_batch(self.ctx.h, self.h, _p(scalars) if n else None, _p(skip), C.c_size_t(n), _p(out) if n else None))
        return out

    def verify_pairs(self, proofs):
        """mi_debug_verify_pairs_dev: the pairs the per-proof bodies hand to their Miller loops -> (P (n, np, 8), Q (n, np, 16))"""
        arr, keep = self._inputs(list(proofs)); n = len(arr)
        np_ = 3 + (self.n_commitments + 1 if self.n_commitments else 0)
        P_, Q_ = np.zeros((n, np_, 8), np.uint64), np.zeros((n, np_, 16), np.uint64)
        self.ctx._ck(self.ctx.lib.mi_debug_verify_pairs_dev(self.ctx.h, self.h, arr, C.c_size_t(n), _p(P_), _p(Q_)))
        return P_, Q_

    # ---- one verdict for the batch (include/mi355x_groth16_verify_combined.h)
    def verify_combined(self, proofs, seed=None):
        """mi_groth16_verify_combined: proofs as verify_batch takes them, seed = 32 bytes or None (the library draws it from the
        operating system) -> (verdict, first_malformed)"""
        assert seed is None or len(seed) == 32
        arr, keep = self._inputs(list(proofs)); v = C.c_uint8(255); first = C.c_uint64(1 << 63)
        self.ctx._ck(self.ctx.lib.mi_groth16_verify_combined(self.ctx.h, self.h, arr, C.c_size_t(len(arr)), seed, C.byref(v), C.byref(first)))
        return int(v.value), int(first.value)

    def verify_bytes_combined(self, proofs, seed=None):
        """mi_groth16_verify_bytes_combined: proofs as verify_bytes_batch takes them -> (verdict, first_malformed)"""
        assert seed is None or len(seed) == 32
        arr, keep = self._bytes_inputs(proofs); v = C.c_uint8(255); first = C.c_uint64(1 << 63)
        self.ctx._ck(self.ctx.lib.mi_groth16_verify_bytes_combined(self.ctx.h, self.h, arr, C.c_size_t(len(arr)), seed, C.byref(v), C.byref(first)))
        return int(v.value), int(first.value)

    # ---- one verdict per proof at the combined test's price (include/mi355x_groth16_verify_locate.h)
    def verify_locate(self, proofs, seed=None):
        """mi_groth16_verify_locate: proofs as verify_batch takes them, seed as verify_combined -> (verdicts (n,) uint8, stats dict)"""
        assert seed is None or len(seed) == 32
        arr, keep = self._inputs(list(proofs)); out = np.full(len(arr), 255, np.uint8); st = VerifyLocateStats()
        self.ctx._ck(self.ctx.lib.mi_groth16_verify_locate(self.ctx.h, self.h, arr, C.c_size_t(len(arr)), seed, _p(out), C.byref(st)))
        return out, st.as_dict()

    def verify_bytes_locate(self, proofs, seed=None):
        """mi_groth16_verify_bytes_locate: proofs as verify_bytes_batch takes them -> (verdicts, stats dict)"""
        assert seed is None or len(seed) == 32
        arr, keep = self._bytes_inputs(proofs); out = np.full(len(arr), 255, np.uint8); st = VerifyLocateStats()
        self.ctx._ck(self.ctx.lib.mi_groth16_verify_bytes_locate(self.ctx.h, self.h, arr, C.c_size_t(len(arr)), seed, _p(out), C.byref(st)))
        return out, st.as_dict()

    # ---- from a proof's bytes (include/mi355x_groth16_verify_bytes.h)
    def set_public_committed(self, lists):
        """mi_vk_set_public_committed: gnark's PublicAndCommitmentCommitted, one list of 1-based indices per commitment"""
        off = np.cumsum([0] + [len(l) for l in lists]).astype(np.uint32)
        idx = np.array([j for l in lists for j in l], np.uint32)
        assert len(lists) == self.n_commitments
        self.ctx._ck(self.ctx.lib.mi_vk_set_public_committed(self.ctx.h, self.h, _p(off), _p(idx) if len(idx) else None))

    def verify_bytes(self, proof: bytes, public_inputs=None) -> int:
        v = C.c_uint8(255); pub = None if public_inputs is None else _u64(public_inputs)
        self.ctx._ck(self.ctx.lib.mi_groth16_verify_bytes(self.ctx.h, self.h, proof, C.c_size_t(len(proof)), _p(pub), C.byref(v)))
        return int(v.value)

    def verify_bytes_batch(self, proofs):
        """proofs: [(bytes, public_inputs (nb_public - 1, 4) or None)]"""
        arr, keep = self._bytes_inputs(proofs)
        out = np.full(len(arr), 255, np.uint8)
        self.ctx._ck(self.ctx.lib.mi_groth16_verify_bytes_batch(self.ctx.h, self.h, arr, C.c_size_t(len(arr)), _p(out)))
        return out

    def _bytes_inputs(self, proofs):
        proofs = list(proofs); arr = (VerifyBytesInput * len(proofs))(); keep = []
        for i, (b, pub) in enumerate(proofs):
            buf = C.create_string_buffer(b, len(b)); keep.append(buf)
            arr[i].proof, arr[i].proof_len = C.addressof(buf), len(b)
            if pub is not None:
                pub = _u64(pub); keep.append(pub); arr[i].public_inputs = pub.ctypes.data
        return arr, keep

    # ---- from the bytes of proof and public witness (include/mi355x_groth16_vkfile.h); proofs: [(proof bytes, witness bytes)]
    def _files_inputs(self, proofs):
        proofs = list(proofs); arr = (VerifyFilesInput * len(proofs))(); keep = []
        for i, (b, w) in enumerate(proofs):
            pb = C.create_string_buffer(b, len(b)); wb = C.create_string_buffer(w, len(w)); keep += [pb, wb]
            arr[i].proof, arr[i].proof_len, arr[i].witness, arr[i].witness_len = C.addressof(pb), len(b), C.addressof(wb), len(w)
        return arr, keep

    def verify_files(self, proof: bytes, witness: bytes) -> int:
        v = C.c_uint8(255)
        self.ctx._ck(self.ctx.lib.mi_groth16_verify_files(self.ctx.h, self.h, proof, C.c_size_t(len(proof)), witness, C.c_size_t(len(witness)), C.byref(v)))
        return int(v.value)

    def verify_files_batch(self, proofs, out=None):
        arr, keep = self._files_inputs(proofs)
        out = np.full(len(arr), 255, np.uint8) if out is None else out
        self.ctx._ck(self.ctx.lib.mi_groth16_verify_files_batch(self.ctx.h, self.h, arr, C.c_size_t(len(arr)), _p(out)))
        return out

    def verify_files_combined(self, proofs, seed=None):
        assert seed is None or len(seed) == 32
        arr, keep = self._files_inputs(proofs); v = C.c_uint8(255); first = C.c_uint64(1 << 63)
        self.ctx._ck(self.ctx.lib.mi_groth16_verify_files_combined(self.ctx.h, self.h, arr, C.c_size_t(len(arr)), seed, C.byref(v), C.byref(first)))
        return int(v.value), int(first.value)

    def verify_files_locate(self, proofs, seed=None):
        assert seed is None or len(seed) == 32
        arr, keep = self._files_inputs(proofs); out = np.full(len(arr), 255, np.uint8); st = VerifyLocateStats()
        self.ctx._ck(self.ctx.lib.mi_groth16_verify_files_locate(self.ctx.h, self.h, arr, C.c_size_t(len(arr)), seed, _p(out), C.byref(st)))
        return out, st.as_dict()

    def free(self):
        if self.h:
            self.ctx._ck(self.ctx.lib.mi_vk_free(self.ctx.h, self.h))
            self.h = None


# ---- host-only helpers (no ctx)
class Prover:
    """Several proofs in flight on one device (mi_prover_*, include/mi355x_groth16.h).  Mirrors a prover service that
    calls groth16.Prove (reference mt.go:496) from many goroutines: submit() returns a ticket, wait() the proof."""

    def __init__(self, device_id=0, in_flight=2):
        self.lib = load()
        h = C.c_void_p()
        rc = self.lib.mi_prover_create(C.c_int(device_id), C.c_uint32(in_flight), C.byref(h))
        if rc != 0:
            raise MiError(f"mi_prover_create failed: {rc} (no gfx950 device? the product has no CPU path)")
        self.h = h
        self.in_flight = int(self.lib.mi_prover_in_flight(h))
        self._pending = {}

    def ctx(self, i=0) -> "Context":
        """context i of the pool, for mi_pk_load / device buffers (never prove on it directly)"""
        p = self.lib.mi_prover_ctx(self.h, C.c_uint32(i))
        if not p:
            raise MiError("mi_prover_ctx: index out of range")
        return Context(_borrowed=p)

    def set_knob(self, name, value):
        """the knob on every proving context of the pool (call while the pool is idle)"""
        for i in range(self.in_flight):
            self.ctx(i).set_knob(name, value)

    def submit(self, pkh, W, a, b, c, r, s, device=False, n_wires=None, n_constraints=None) -> int:
        out = np.zeros(32, np.uint64); st = Stats(); t = C.c_uint64()
        r, s = _u64(r), _u64(s)
        if device:
            keep = ()
            rc = self.lib.mi_prover_submit_dev(self.h, pkh, _p(W), C.c_size_t(n_wires), _p(a), _p(b), _p(c), C.c_size_t(n_constraints),
                                               _p(r), _p(s), _p(out), C.byref(st), C.byref(t))
        else:
            W, a, b, c = _u64(W), _u64(a), _u64(b), (None if c is None else _u64(c))   # c = None: formed on the device as a o b
            keep = (W, a, b, c)
            rc = self.lib.mi_prover_submit(self.h, pkh, _p(W), C.c_size_t(W.shape[0]), _p(a), _p(b), _p(c), C.c_size_t(a.shape[0]),
                                           _p(r), _p(s), _p(out), C.byref(st), C.byref(t))
        if rc != 0:
            raise MiError(f"mi_prover_submit: rc={rc}")
        self._pending[t.value] = (out, st, keep)   # the library writes into these until wait() returns
        return t.value

    def wait(self, ticket):
        out, st, keep = self._pending.pop(ticket)
        rc = self.lib.mi_prover_wait(self.h, C.c_uint64(ticket))
        if rc != 0:
            raise MiError(f"rc={rc}: {self.lib.mi_prover_last_error(self.h).decode()}")
        res = {"ar": out[:8].copy(), "bs": out[8:24].copy(), "krs": out[24:].copy(), "raw": out}
        if isinstance(keep, dict) and "pok" in keep:
            res["pok"] = keep["pok"]
        return res, st.as_dict()

    # ---- BSB22 through the pool (mi_prover_commit / mi_prover_submit_bsb22)
    def commit(self, ped_pk, values):
        """pedersen Commit inside the solve: synchronous, thread-safe"""
        values = _u64(values); out = np.zeros(8, np.uint64)
        rc = self.lib.mi_prover_commit(self.h, ped_pk, _p(values), C.c_size_t(values.shape[0]), _p(out))
        if rc != 0:
            raise MiError(f"mi_prover_commit rc={rc}: {self.lib.mi_prover_last_error(self.h).decode()}")
        return out

    def submit_bsb22(self, pkh, W, a, b, c, r, s, commitments, challenge) -> int:
        """host inputs; commitments = [(pedersen key handle, private committed values)]; wait() returns the proof with res['pok']"""
        out = np.zeros(32, np.uint64); st = Stats(); t = C.c_uint64(); pok = np.zeros(8, np.uint64)
        r, s, challenge = _u64(r), _u64(s), _u64(challenge)
        W, a, b, c = _u64(W), _u64(a), _u64(b), (None if c is None else _u64(c))
        vals = [_u64(v) for _, v in commitments]
        arr = (Bsb22Input * len(commitments))()
        for i, ((key, _), v) in enumerate(zip(commitments, vals)):
            arr[i].key = key if isinstance(key, int) else key.value; arr[i].values = v.ctypes.data; arr[i].n = v.shape[0]
        rc = self.lib.mi_prover_submit_bsb22(self.h, pkh, _p(W), C.c_size_t(W.shape[0]), _p(a), _p(b), _p(c), C.c_size_t(a.shape[0]),
                                             _p(r), _p(s), arr, C.c_uint32(len(commitments)), _p(challenge), _p(out), _p(pok), C.byref(st), C.byref(t))
        if rc != 0:
            raise MiError(f"mi_prover_submit_bsb22: rc={rc}")
        self._pending[t.value] = (out, st, {"keep": (W, a, b, c, vals, arr, challenge), "pok": pok})
        return t.value

    # ---- from W alone (include/mi355x_groth16_r1cs.h)
    def submit_w(self, pkh, rh, W, r, s, flags=0, device=False, n_wires=None) -> int:
        out = np.zeros(32, np.uint64); st = Stats(); t = C.c_uint64()
        r, s = _u64(r), _u64(s)
        if device:
            keep = ()
            rc = self.lib.mi_prover_submit_w_dev(self.h, pkh, rh, _p(W), C.c_size_t(n_wires), C.c_uint32(flags), _p(r), _p(s), _p(out), C.byref(st), C.byref(t))
        else:
            W = _u64(W); keep = (W,)
            rc = self.lib.mi_prover_submit_w(self.h, pkh, rh, _p(W), C.c_size_t(W.shape[0] if n_wires is None else n_wires), C.c_uint32(flags),
                                             _p(r), _p(s), _p(out), C.byref(st), C.byref(t))
        if rc != 0:
            raise MiError(f"mi_prover_submit_w: rc={rc}")
        self._pending[t.value] = (out, st, keep)
        return t.value

    def submit_w_bsb22(self, pkh, rh, W, r, s, commitments, challenge, flags=0) -> int:
        """submit_bsb22 without a, b, c"""
        out = np.zeros(32, np.uint64); st = Stats(); t = C.c_uint64(); pok = np.zeros(8, np.uint64)
        r, s, challenge, W = _u64(r), _u64(s), _u64(challenge), _u64(W)
        vals = [_u64(v) for _, v in commitments]
        arr = (Bsb22Input * len(commitments))()
        for i, ((key, _), v) in enumerate(zip(commitments, vals)):
            arr[i].key = key if isinstance(key, int) else key.value; arr[i].values = v.ctypes.data; arr[i].n = v.shape[0]
        rc = self.lib.mi_prover_submit_w_bsb22(self.h, pkh, rh, _p(W), C.c_size_t(W.shape[0]), C.c_uint32(flags), _p(r), _p(s), arr,
                                               C.c_uint32(len(commitments)), _p(challenge), _p(out), _p(pok), C.byref(st), C.byref(t))
        if rc != 0:
            raise MiError(f"mi_prover_submit_w_bsb22: rc={rc}")
        self._pending[t.value] = (out, st, {"keep": (W, vals, arr, challenge), "pok": pok})
        return t.value

    def trim(self):
        rc = self.lib.mi_prover_trim(self.h)
        if rc != 0:
            raise MiError(f"mi_prover_trim rc={rc}: {self.lib.mi_prover_last_error(self.h).decode()}")

    def close(self):
        if self.h:
            self.lib.mi_prover_destroy(self.h)
            self.h = None


def shard_range(total, world, rank):
    """slice [lo, hi) of rank `rank`: the same cut as the library's (csrc/group.hip range_of)"""
    return total * rank // world, total * (rank + 1) // world


def _fill_pk_desc(pk: dict):
    """whole-key descriptor over HOST arrays (mi_pk_load / mi_pk_load_sharded)"""
    d = PkDesc(); keep = []
    d.log_n, d.nb_public, d.nb_wires = pk["log_n"], pk["nb_public"], pk["nb_wires"]
    for name in ("g1_a", "g1_b", "g1_k", "g1_z", "g2_b"):
        arr = _u64(pk[name]); keep.append(arr)
        setattr(d, name, arr.ctypes.data); setattr(d, "n_" + name, arr.shape[0])
    for name, k in (("alpha1", 8), ("beta1", 8), ("delta1", 8), ("beta2", 16), ("delta2", 16)):
        setattr(d, name, (C.c_uint64 * k)(*[int(v) for v in _u64(pk[name]).reshape(-1)]))
    ia = np.ascontiguousarray(pk["infinity_a"], dtype=np.uint8); ib = np.ascontiguousarray(pk["infinity_b"], dtype=np.uint8)
    keep += [ia, ib]
    d.infinity_a, d.infinity_b = ia.ctypes.data, ib.ctypes.data
    cw = pk.get("committed_wires")
    if cw is not None and len(cw):
        cw = np.ascontiguousarray(cw, dtype=np.uint32); keep.append(cw)
        d.committed_wires, d.n_committed = cw.ctypes.data, cw.shape[0]
    return d, keep


class Group:
    """Several GPUs behind one handle (mi_group_*, include/mi355x_groth16.h): the point-sharded prove and MSM of SURVEY 8e.
    Group([0, 1, ...]) = all ranks in this process (what a Go caller uses); Group.rank(dev, rank, world, id) = one rank per
    process (torch.distributed.run): the 128-byte id comes from Group.unique_id() on rank 0 through the caller's own channel."""

    def __init__(self, dev_ids=None, _h=None):
        self.lib = load()
        if _h is not None:
            self.h = _h
        else:
            arr = (C.c_int * len(dev_ids))(*dev_ids); h = C.c_void_p()
            rc = self.lib.mi_group_create(arr, C.c_int(len(dev_ids)), C.byref(h))
            if rc != 0:
                raise MiError(f"mi_group_create failed: {rc} (no gfx950 device? the product has no CPU path)")
            self.h = h
        self.world = int(self.lib.mi_group_world(self.h)); self.n_local = int(self.lib.mi_group_local(self.h))

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        if load().mi_group_unique_id(buf) != 0:
            raise MiError("mi_group_unique_id failed")
        return bytes(buf)

    @classmethod
    def rank(cls, device_id, rank, world, uid: bytes, transport=1):
        """transport 1 = RCCL (uid from unique_id()), 3 = host-staged through shared memory (uid = any 128 bytes the ranks share)"""
        h = C.c_void_p(); buf = (C.c_uint8 * 128)(*uid)
        rc = load().mi_group_create_rank_ex(C.c_int(device_id), C.c_int(rank), C.c_int(world), buf, C.c_int(transport), C.byref(h))
        if rc != 0:
            raise MiError(f"mi_group_create_rank_ex failed: {rc}")
        return cls(_h=h)

    def _ck(self, rc):
        if rc != 0:
            raise MiError(f"rc={rc}: {self.lib.mi_group_last_error(self.h).decode()}")

    def ctx(self, i=0) -> "Context":
        p = self.lib.mi_group_ctx(self.h, C.c_int(i))
        if not p:
            raise MiError("mi_group_ctx: index out of range")
        return Context(_borrowed=p)

    def transport(self):
        return {1: "rccl", 2: "peer-copy", 3: "host-staged"}[int(self.lib.mi_group_transport(self.h))]

    def rank_index(self):
        return int(self.lib.mi_group_rank(self.h))

    def comm_ranks(self):
        """ranks the RCCL communicator itself reports (ncclCommCount); 0 = the transport is not RCCL"""
        n = int(self.lib.mi_group_comm_ranks(self.h))
        if n < 0:
            raise MiError(f"mi_group_comm_ranks: {n}")
        return n

    def device_pci(self, local_rank=0):
        buf = C.create_string_buffer(32)
        self._ck(self.lib.mi_group_device_pci(self.h, C.c_int(local_rank), buf))
        return buf.value.decode()

    def set_lead_share(self, permille=0xFFFFFFFF):
        """rank 0's share of the wires, permille of an even share (0xFFFFFFFF = automatic); before pk_load*, the same on every rank"""
        self._ck(self.lib.mi_group_set_lead_share(self.h, C.c_uint32(permille)))

    def wire_range(self, nb_wires, rank):
        """wires [lo, hi) of global rank `rank` under the group's lead share (what pk_load_dev slices and W slices must follow)"""
        lo, hi = C.c_uint64(), C.c_uint64()
        self._ck(self.lib.mi_group_wire_range(self.h, C.c_uint64(nb_wires), C.c_int(rank), C.byref(lo), C.byref(hi)))
        return int(lo.value), int(hi.value)

    def set_sharded_compute_h(self, on=True):
        self._ck(self.lib.mi_group_set_sharded_compute_h(self.h, C.c_uint32(1 if on else 0)))

    def compute_h_sharded_dev(self, log_n, a_ptrs, b_ptrs, c_ptrs, n_constraints, h_ptrs):
        """computeH over the ranks: per LOCAL rank device pointers to its rows of a, b (c_ptrs None: c = a o b) and to its M-element h slice"""
        arr = lambda ps: (C.c_void_p * len(ps))(*[C.c_void_p(int(p)) for p in ps])
        self._ck(self.lib.mi_compute_h_sharded_dev(self.h, C.c_uint32(log_n), arr(a_ptrs), arr(b_ptrs), None if c_ptrs is None else arr(c_ptrs),
                                                   C.c_size_t(n_constraints), arr(h_ptrs)))

    def exchange_selftest(self, nbytes=4096):
        self._ck(self.lib.mi_group_exchange_selftest(self.h, C.c_size_t(nbytes)))

    def pk_load(self, pk: dict):
        d, keep = _fill_pk_desc(pk); h = C.c_void_p()
        self._ck(self.lib.mi_pk_load_sharded(self.h, C.byref(d), C.byref(h)))
        return h

    def pk_load_dev(self, pk: dict, slices):
        """pk: header + masks of the WHOLE key (host); slices[i] = {name: (device pointer on local rank i's device, count)} for
        g1_a, g1_b, g1_k, g1_z, g2_b: that rank's slices (mi_pk_load_sharded_dev)"""
        descs = (PkDesc * len(slices))(); keep = []
        ia = np.ascontiguousarray(pk["infinity_a"], dtype=np.uint8); ib = np.ascontiguousarray(pk["infinity_b"], dtype=np.uint8)
        cw = pk.get("committed_wires")
        cw = np.ascontiguousarray(cw, dtype=np.uint32) if cw is not None and len(cw) else None
        keep += [ia, ib, cw]
        for d, sl in zip(descs, slices):
            d.log_n, d.nb_public, d.nb_wires = pk["log_n"], pk["nb_public"], pk["nb_wires"]
            for name in ("g1_a", "g1_b", "g1_k", "g1_z", "g2_b"):
                ptr, cnt = sl[name]
                setattr(d, name, int(ptr)); setattr(d, "n_" + name, int(cnt))
            for name, k in (("alpha1", 8), ("beta1", 8), ("delta1", 8), ("beta2", 16), ("delta2", 16)):
                setattr(d, name, (C.c_uint64 * k)(*[int(v) for v in _u64(pk[name]).reshape(-1)]))
            d.infinity_a, d.infinity_b = ia.ctypes.data, ib.ctypes.data
            if cw is not None:
                d.committed_wires, d.n_committed = cw.ctypes.data, cw.shape[0]
        h = C.c_void_p()
        self._ck(self.lib.mi_pk_load_sharded_dev(self.h, descs, C.byref(h)))
        return h

    def pk_free(self, spk):
        self._ck(self.lib.mi_pk_sharded_free(self.h, spk))

    def prove(self, spk, W, a, b, c, r, s, mode=0):
        """host inputs; a, b, c may be None in a process that does not hold rank 0"""
        out = np.zeros(32, np.uint64); st = Stats()
        W, r, s = _u64(W), _u64(r), _u64(s)
        a, b, c = (None if x is None else _u64(x) for x in (a, b, c))
        self._ck(self.lib.mi_groth16_prove_sharded(self.h, spk, _p(W), C.c_size_t(W.shape[0]), _p(a), _p(b), _p(c), C.c_size_t(0 if a is None else a.shape[0]),
                                                   _p(r), _p(s), C.c_uint32(mode), _p(out), C.byref(st)))
        return {"ar": out[:8].copy(), "bs": out[8:24].copy(), "krs": out[24:].copy(), "raw": out}, st.as_dict()

    def prove_dev(self, spk, W_ptrs, n_wires, a_ptr, b_ptr, c_ptr, n_constraints, r, s, mode=0):
        """inputs resident: W_ptrs[i] = wire range of local rank i on its device; a, b, c on rank 0's device (None elsewhere)"""
        out = np.zeros(32, np.uint64); st = Stats(); r, s = _u64(r), _u64(s)
        ww = (C.c_void_p * len(W_ptrs))(*[int(p) for p in W_ptrs])
        self._ck(self.lib.mi_groth16_prove_sharded_dev(self.h, spk, ww, C.c_size_t(n_wires), _p(a_ptr), _p(b_ptr), _p(c_ptr), C.c_size_t(n_constraints),
                                                       _p(r), _p(s), C.c_uint32(mode), _p(out), C.byref(st)))
        return {"ar": out[:8].copy(), "bs": out[8:24].copy(), "krs": out[24:].copy(), "raw": out}, st.as_dict()

    def prove_slices_dev(self, spk, W_ptrs, n_wires, a_ptrs, b_ptrs, c_ptrs, n_constraints, r, s, mode=0):
        """computeH over the ranks: a_ptrs[i] / b_ptrs[i] / c_ptrs[i] = local rank i's ROWS of a, b, c on its device (c_ptrs None: c = a o b)"""
        out = np.zeros(32, np.uint64); st = Stats(); r, s = _u64(r), _u64(s)
        arr = lambda ps: (C.c_void_p * len(ps))(*[C.c_void_p(int(p)) for p in ps])
        self._ck(self.lib.mi_groth16_prove_sharded_slices_dev(self.h, spk, arr(W_ptrs), C.c_size_t(n_wires), arr(a_ptrs), arr(b_ptrs), None if c_ptrs is None else arr(c_ptrs),
                                                              C.c_size_t(n_constraints), _p(r), _p(s), C.c_uint32(mode), _p(out), C.byref(st)))
        return {"ar": out[:8].copy(), "bs": out[8:24].copy(), "krs": out[24:].copy(), "raw": out}, st.as_dict()

    def msm_g1(self, pts, sc, flags=0, mode=0):
        out = np.zeros(12, np.uint64); pts, sc = _u64(pts), _u64(sc)
        self._ck(self.lib.mi_msm_g1_sharded(self.h, _p(pts), _p(sc), C.c_size_t(pts.shape[0]), C.c_uint32(flags), C.c_uint32(mode), _p(out)))
        return out

    def msm_g2(self, pts, sc, flags=0, mode=0):
        out = np.zeros(24, np.uint64); pts, sc = _u64(pts), _u64(sc)
        self._ck(self.lib.mi_msm_g2_sharded(self.h, _p(pts), _p(sc), C.c_size_t(pts.shape[0]), C.c_uint32(flags), C.c_uint32(mode), _p(out)))
        return out

    def msm_dev(self, pts_ptrs, sc_ptrs, n_local, n_total, flags=0, mode=0, g2=False):
        """pairs already resident: one device pointer / count per LOCAL rank"""
        k = len(n_local)
        pp = (C.c_void_p * k)(*[int(p) for p in pts_ptrs]); ss = (C.c_void_p * k)(*[int(p) for p in sc_ptrs]); nn = (C.c_size_t * k)(*n_local)
        out = np.zeros(24 if g2 else 12, np.uint64)
        f = self.lib.mi_msm_g2_sharded_dev if g2 else self.lib.mi_msm_g1_sharded_dev
        self._ck(f(self.h, pp, ss, nn, C.c_size_t(n_total), C.c_uint32(flags), C.c_uint32(mode), _p(out)))
        return out

    def close(self):
        if self.h:
            self.lib.mi_group_destroy(self.h)
            self.h = None


def proof_write(raw, commitments=None, pok=None):
    n = 0 if commitments is None else commitments.shape[0]
    buf = np.zeros(164 + 32 * n, np.uint8)
    ln = load().mi_proof_write(_p(_u64(raw)), _p(commitments), C.c_uint32(n), _p(pok), _p(buf))
    return bytes(buf[:ln])


def proof_read(data: bytes, n_commitments):
    """mi_proof_read: Proof.WriteTo's bytes -> (raw (32,) uint64, commitments (n, 8), pok (8,)), or None when the library refuses them"""
    raw = np.zeros(32, np.uint64); cm = np.zeros((n_commitments, 8), np.uint64); pok = np.zeros(8, np.uint64)
    rc = load().mi_proof_read(data, C.c_size_t(len(data)), C.c_uint32(n_commitments), _p(raw), _p(cm) if n_commitments else None, _p(pok))
    return (raw, cm, pok) if rc == 0 else None


def hash_to_field(dst: bytes, msg: bytes):
    """mi_hash_to_field -> (4,) uint64 Montgomery"""
    out = np.zeros(4, np.uint64)
    rc = load().mi_hash_to_field(dst, C.c_size_t(len(dst)), msg, C.c_size_t(len(msg)), _p(out))
    if rc != 0:
        raise MiError(f"mi_hash_to_field rc={rc}")
    return out


def g1_compress(p):
    buf = np.zeros(32, np.uint8); load().mi_g1_compress(_p(_u64(p)), _p(buf)); return bytes(buf)


def g2_compress(p):
    buf = np.zeros(64, np.uint8); load().mi_g2_compress(_p(_u64(p)), _p(buf)); return bytes(buf)


def phase1_records_verify(start, start_hash, first_index, records):
    """mi_phase1_records_verify (host only) -> the index of the first record that does not hold, len(records) when all hold; start: (3, 8)
    uint64 = tau_g1[1], alpha_tau_g1[0], beta_tau_g1[0] before the first record"""
    rec = _u64(records).reshape(-1, PHASE1_RECORD_WORDS); fb = C.c_uint64()
    rc = load().mi_phase1_records_verify(_p(_u64(np.array(start, np.uint64).reshape(3, 8))), start_hash, C.c_uint64(first_index), _p(rec) if rec.shape[0] else None,
                                         C.c_size_t(rec.shape[0]), C.byref(fb))
    if rc != 0:
        raise MiError(f"rc={rc}: mi_phase1_records_verify")
    return int(fb.value)


def phase2_sigma_records_verify(start, start_hash, first_index, proofs, hashes):
    """mi_phase2_sigma_records_verify (host only); start: (nc, 16) uint64, proofs: (m, nc, PHASE2_SIGMA_PROOF_WORDS), hashes: m chain values
    -> the index of the first step that does not hold, m when all hold"""
    st = _u64(start).reshape(-1, 16); nc = st.shape[0]
    pr, hs, m = _sigma_steps(proofs, hashes, max(nc, 1)); fb = C.c_uint64()
    rc = load().mi_phase2_sigma_records_verify(_p(st) if nc else None, C.c_uint32(nc), start_hash, C.c_uint64(first_index), _p(pr) if m else None,
                                               hs if m else None, C.c_size_t(m), C.byref(fb))
    if rc:
        raise MiError(f"rc={rc}: mi_phase2_sigma_records_verify")
    return int(fb.value)


def phase2_records_verify(delta1_start, start_hash, first_index, records):
    """mi_phase2_records_verify (host only) -> the index of the first record that does not hold, len(records) when all hold"""
    rec = _u64(records).reshape(-1, PHASE2_RECORD_WORDS); fb = C.c_uint64()
    rc = load().mi_phase2_records_verify(_p(_u64(delta1_start)), start_hash, C.c_uint64(first_index), _p(rec), C.c_size_t(rec.shape[0]), C.byref(fb))
    if rc != 0:
        raise MiError(f"rc={rc}: mi_phase2_records_verify")
    return int(fb.value)


def pedersen_fold(points, challenge):
    points = _u64(points); out = np.zeros(8, np.uint64)
    assert load().mi_pedersen_fold(_p(points), C.c_size_t(points.shape[0]), _p(_u64(challenge)), _p(out)) == 0
    return out


def g1_sum(parts):
    parts = _u64(parts); out = np.zeros(12, np.uint64)
    assert load().mi_g1_sum(_p(parts), C.c_size_t(parts.shape[0]), _p(out)) == 0
    return out


def g2_sum(parts):
    parts = _u64(parts); out = np.zeros(24, np.uint64)
    assert load().mi_g2_sum(_p(parts), C.c_size_t(parts.shape[0]), _p(out)) == 0
    return out

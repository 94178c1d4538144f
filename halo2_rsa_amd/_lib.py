"""ctypes binding of libh2r.so (the C ABI declared in include/h2r.h).

The product path has NO CPU fallback: if the HIP library is missing this module raises.
"""
import ctypes
import os

from . import _build

H2R_PL_COUNT = 29
PLANES = ["Q", "R", "Q_SUB", "R_SUB", "AB_LO", "AB_HI", "QN_LO", "QN_HI", "EQB_LO", "EQB_HI", "AMB_LO", "AMB_HI",
          "SUM_LO", "SUM_HI", "CARRY", "CMOD", "NQ1_LO", "NQ1_HI", "AMNQ1", "ACCX_LO", "ACCX_HI", "QACC", "MODACC",
          "NQ2_LO", "NQ2_HI", "AMNQ2", "FLAGS", "CARRY_DUP", "CARRY_SUB"]
assert len(PLANES) == H2R_PL_COUNT

H2R_OK, H2R_E_SHAPE, H2R_E_ZERO_MODULUS, H2R_E_NOT_REDUCED, H2R_E_FIELD_TOO_SMALL, H2R_E_HIP, H2R_E_UNSUPPORTED, \
    H2R_E_NULL, H2R_E_NOT_IN_FIELD, H2R_E_ASSERTION = range(10)
FIELDS = {"bn254_fr": 0, "bn254_fq": 1, "pasta_fp": 2, "pasta_fq": 3}
# delta per field, canonical: g^(2^S) for p - 1 = 2^S * odd and g the smallest quadratic non-residue -- halo2's generator of the odd-order
# subgroup, the permutation argument's column shift (tests/permutation_ref.py::domain derives it; tests/test_keygen_host.py compares)
FIELD_DELTA = {"bn254_fr": 0x0ba49465f79ce3ca21f1ec72be9f9a263f544c14cc40ac6ba1458af683d28e01,
               "bn254_fq": 0x9,
               "pasta_fp": 0x0a757d0f0006ab6cbd455b7112a5049df5e4f3f13eee56366a6ccd20dd7b9ba2,
               "pasta_fq": 0x2237d5442372416606f0a88e7f7949f8e3ac3376541d11408494392472d1683c}
# (S, g^t) for p - 1 = 2^S * t with t odd and the same g: halo2's root of unity of order 2^S, canonical, for the fields with a curve
# (prover.setup squares it down to the 2^k domain; tests/test_setup_host.py compares with tests/permutation_ref.py::domain)
FIELD_ROOT_OF_UNITY = {"bn254_fr": (28, 0x2a3c09f0a58a7e8500e0a7eb8ef62abc402d111e41112ed49bd61b6e725b19f0)}
# (q, (x, y)): the coordinate field's modulus and the generator of the curve of a field that has one (bn256 G1 over Fq, of order r)
CURVE_GENERATOR = {"bn254_fr": (21888242871839275222246405745257275088696311157297823662689037894645226208583, (1, 2))}
H2R_F_SHARED_MODULUS = 1
H2R_F_KEYED_MODULI = 2   # `n` points to a host H2RKeyedModuli: a per-element index into a key table (h2r_key_table_build)


class H2RParams(ctypes.Structure):
    _fields_ = [("limb_width", ctypes.c_uint32), ("bits_len", ctypes.c_uint32), ("field", ctypes.c_uint32),
                ("device", ctypes.c_int32)]


class H2RAdviceRepr(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("col_stride", ctypes.c_uint64)]


H2R_ADVICE_COLUMNS, H2R_ADVICE_MONTGOMERY = 0x400, 0x800
H2R_VERSION = 5


class H2RKeyedModuli(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("num_keys", ctypes.c_uint64),
                ("table", ctypes.c_void_p), ("key_idx", ctypes.c_void_p)]


class H2RPipelineInfo(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("depth", ctypes.c_uint32), ("side_streams", ctypes.c_uint32), ("record_form", ctypes.c_uint32),
                ("three_queues", ctypes.c_uint32), ("probe_ms", ctypes.c_float), ("probe_span_ms", ctypes.c_float)]


H2R_PIPE_ONE_LAUNCH_STEP, H2R_PIPE_TWO_QUEUE, H2R_PIPE_SIDE_STREAM, H2R_PIPE_AUTO = 0, 1, 2, 3


class H2RLayout(ctypes.Structure):
    _fields_ = [("limb_width", ctypes.c_uint32), ("num_limbs", ctypes.c_uint32), ("num_cols", ctypes.c_uint32),
                ("limb_bytes", ctypes.c_uint32), ("wide_bytes", ctypes.c_uint32), ("carry_bytes", ctypes.c_uint32),
                ("limb_sub_bits", ctypes.c_uint32), ("limb_nsub", ctypes.c_uint32),
                ("carry_bits", ctypes.c_uint32), ("carry_sub_bits", ctypes.c_uint32), ("carry_nsub", ctypes.c_uint32),
                ("carry_sub_stride", ctypes.c_uint32), ("word_max_bits", ctypes.c_uint32), ("reserved0", ctypes.c_uint32),
                ("record_stride", ctypes.c_uint64), ("stream_bytes", ctypes.c_uint64),
                ("plane_off", ctypes.c_uint64 * H2R_PL_COUNT), ("plane_elem", ctypes.c_uint32 * H2R_PL_COUNT),
                ("plane_count", ctypes.c_uint32 * H2R_PL_COUNT),
                ("acc_steps_per_group", ctypes.c_uint32), ("acc_lo_row_bytes", ctypes.c_uint32),
                ("acc_lo_group_bytes", ctypes.c_uint64), ("acc_hi_group_bytes", ctypes.c_uint64)]


class H2RPowLayout(ctypes.Structure):
    _fields_ = [("num_mul_mods", ctypes.c_uint32), ("num_exp_bits", ctypes.c_uint32),
                ("elem_stride", ctypes.c_uint64), ("off_records", ctypes.c_uint64), ("off_result", ctypes.c_uint64),
                ("off_e_bits", ctypes.c_uint64), ("off_selected", ctypes.c_uint64), ("selected_stride", ctypes.c_uint64),
                ("stream_bytes", ctypes.c_uint64), ("exp_limb_bits", ctypes.c_uint32), ("e_num_limbs", ctypes.c_uint32)]


class H2RCopy(ctypes.Structure):
    _fields_ = [("row", ctypes.c_uint32), ("col", ctypes.c_uint32), ("src_row", ctypes.c_uint32), ("src_col", ctypes.c_uint32)]


class H2RAdviceLayout(ctypes.Structure):
    _fields_ = [("version", ctypes.c_uint32), ("column_of", (ctypes.c_uint8 * 5) * 256)]


H2R_COPY_SRC_A, H2R_COPY_SRC_B, H2R_COPY_SRC_N = 0xFFFFFF01, 0xFFFFFF02, 0xFFFFFF03
H2R_SRC_X, H2R_SRC_ONE = -1, -2


class H2RVerifyLayout(ctypes.Structure):
    _fields_ = [("pow", H2RPowLayout), ("off_in_field", ctypes.c_uint64), ("in_field_stream_bytes", ctypes.c_uint64),
                ("off_em", ctypes.c_uint64), ("em_stream_bytes", ctypes.c_uint64), ("elem_stride", ctypes.c_uint64),
                ("stream_bytes", ctypes.c_uint64)]


class H2RLookupConfig(ctypes.Structure):
    _fields_ = [("n_lens", ctypes.c_uint32), ("bit_len", ctypes.c_uint32 * 8), ("tag", ctypes.c_uint32 * 8),
                ("row_off", ctypes.c_uint32 * 8), ("n_rows", ctypes.c_uint32)]


H2R_PERM_MAX_COLUMNS, H2R_PERM_MAX_EXTRA = 8, 3


class H2RPermutationConfig(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("num_columns", ctypes.c_uint32), ("chunk_len", ctypes.c_uint32), ("n_extra", ctypes.c_uint32),
                ("column_src", ctypes.c_uint8 * H2R_PERM_MAX_COLUMNS), ("delta", ctypes.c_uint64 * 4), ("omega", ctypes.c_uint64 * 4)]


H2R_NTT_INVERSE = 1


class H2RNttConfig(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("log_n_in", ctypes.c_uint32), ("log_n_out", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("omega", ctypes.c_uint64 * 4), ("shift", ctypes.c_uint64 * 4)]


H2R_LOOKUP_ARGS, H2R_QUOTIENT_MAX_FIXED = 5, 16


class H2RColumnGroup(ctypes.Structure):
    _fields_ = [("base", ctypes.c_void_p), ("elem_stride", ctypes.c_uint64), ("col_stride", ctypes.c_uint64)]


class H2RQuotientInputs(ctypes.Structure):
    GROUPS = ("advice", "extra", "perm_z", "lookup_a_perm", "lookup_s_perm", "lookup_z", "fixed", "sigma", "l")
    CHALLENGES = ("theta", "beta", "gamma", "y")
    _fields_ = [(nm, H2RColumnGroup) for nm in GROUPS] + [(nm, ctypes.c_void_p) for nm in CHALLENGES]


class H2RQuotientConfig(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("log_n", ctypes.c_uint32), ("log_ext", ctypes.c_uint32), ("blinding_factors", ctypes.c_uint32),
                ("omega_ext", ctypes.c_uint64 * 4), ("zeta", ctypes.c_uint64 * 4), ("delta", ctypes.c_uint64 * 4),
                ("num_fixed", ctypes.c_uint32), ("num_columns", ctypes.c_uint32), ("chunk_len", ctypes.c_uint32), ("n_extra", ctypes.c_uint32),
                ("lookup_mask", ctypes.c_uint32), ("gate_fixed", ctypes.c_uint8 * 9), ("column_src", ctypes.c_uint8 * H2R_PERM_MAX_COLUMNS),
                ("lookup_advice", ctypes.c_uint8 * H2R_LOOKUP_ARGS), ("lookup_tag", ctypes.c_uint8 * H2R_LOOKUP_ARGS),
                ("lookup_enable", ctypes.c_uint8 * H2R_LOOKUP_ARGS), ("table_tag", ctypes.c_uint8), ("table_value", ctypes.c_uint8)]


H2R_OPEN_MAX_COLUMNS, H2R_OPEN_MAX_POINTS = 64, 4


class H2ROpenColumn(ctypes.Structure):
    _fields_ = [("base", ctypes.c_void_p), ("elem_stride", ctypes.c_uint64), ("point_mask", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class H2ROpenConfig(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("n_coeffs", ctypes.c_uint32), ("num_cols", ctypes.c_uint32), ("num_points", ctypes.c_uint32)]


H2R_MSM_MAX_COLUMNS = 64


class H2RMsmColumn(ctypes.Structure):
    _fields_ = [("base", ctypes.c_void_p), ("elem_stride", ctypes.c_uint64)]


class H2RMsmConfig(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("n", ctypes.c_uint32), ("num_cols", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class H2RMsmInfo(ctypes.Structure):
    _fields_ = [("window_bits", ctypes.c_uint32), ("num_windows", ctypes.c_uint32), ("slice_points", ctypes.c_uint32), ("num_slices", ctypes.c_uint32),
                ("workspace_bytes", ctypes.c_uint64)]


H2R_CURVE_NTT_INVERSE = 1


class H2RCurveNttConfig(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("log_n", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("omega", ctypes.c_uint64 * 4)]


H2R_TRANSCRIPT_MAX_ITEMS, H2R_TRANSCRIPT_MAX_SQUEEZE, H2R_TRANSCRIPT_MAX_DERIVE, H2R_TRANSCRIPT_MAX_COUNT = 64, 8, 16, 65536
H2R_TRANSCRIPT_INIT, H2R_TRANSCRIPT_POINT, H2R_TRANSCRIPT_SCALAR, H2R_TRANSCRIPT_COMMON = 1, 1, 2, 1


class H2RTranscriptConfig(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("num_items", ctypes.c_uint32), ("num_squeeze", ctypes.c_uint32), ("num_derive", ctypes.c_uint32),
                ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class H2RTranscriptItem(ctypes.Structure):
    _fields_ = [("base", ctypes.c_void_p), ("elem_stride", ctypes.c_uint64), ("count", ctypes.c_uint32), ("kind", ctypes.c_uint32),
                ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class H2RTranscriptDerive(ctypes.Structure):
    _fields_ = [("src", ctypes.c_uint32), ("log2_pow", ctypes.c_uint32), ("mult", ctypes.c_uint64 * 4)]


H2R_RANDOM_MAX_COLUMNS = 64


class H2RRandomConfig(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("num_cols", ctypes.c_uint32), ("row_begin", ctypes.c_uint64), ("row_end", ctypes.c_uint64),
                ("first_circuit", ctypes.c_uint64), ("reserved", ctypes.c_uint64), ("seed", ctypes.c_uint8 * 32)]


class H2RRandomColumn(ctypes.Structure):
    _fields_ = [("base", ctypes.c_void_p), ("elem_stride", ctypes.c_uint64), ("tag", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


H2R_VERIFY_MAX_SECTIONS, H2R_VERIFY_MAX_PLAN, H2R_VERIFY_MAX_TERMS = 16, 64, 4096
VERIFY_GROUPS = ("advice", "fixed", "random", "sigma", "perm_z", "lookup_z", "lookup_a_perm", "lookup_s_perm", "h")   # H2R_VERIFY_G_*


class H2RProofSection(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_uint32), ("count", ctypes.c_uint32)]


class H2RProofDecodeConfig(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("num_sections", ctypes.c_uint32), ("reserved", ctypes.c_uint64)]


class H2RVerifyPlanEntry(ctypes.Structure):
    _fields_ = [("group", ctypes.c_uint8), ("index", ctypes.c_uint8), ("mask", ctypes.c_uint8), ("reserved", ctypes.c_uint8)]


class H2RVerifyScalarsConfig(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("log_n", ctypes.c_uint32), ("blinding_factors", ctypes.c_uint32), ("num_fixed", ctypes.c_uint32),
                ("num_columns", ctypes.c_uint32), ("chunk_len", ctypes.c_uint32), ("lookup_mask", ctypes.c_uint32),
                ("num_eval_plan", ctypes.c_uint32), ("num_open_plan", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("omega", ctypes.c_uint64 * 4), ("delta", ctypes.c_uint64 * 4), ("gate_fixed", ctypes.c_uint8 * 9),
                ("column_src", ctypes.c_uint8 * H2R_PERM_MAX_COLUMNS), ("lookup_advice", ctypes.c_uint8 * H2R_LOOKUP_ARGS),
                ("lookup_tag", ctypes.c_uint8 * H2R_LOOKUP_ARGS), ("lookup_enable", ctypes.c_uint8 * H2R_LOOKUP_ARGS),
                ("table_tag", ctypes.c_uint8), ("table_value", ctypes.c_uint8),
                ("eval_plan", H2RVerifyPlanEntry * H2R_VERIFY_MAX_PLAN), ("open_plan", H2RVerifyPlanEntry * H2R_VERIFY_MAX_PLAN)]


class H2RVerifyChallenges(ctypes.Structure):
    NAMES = ("theta", "beta", "gamma", "y", "x", "v", "u")
    _fields_ = [(nm, ctypes.c_void_p) for nm in NAMES]


class H2RMsmTermsConfig(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("num_terms", ctypes.c_uint32), ("reserved", ctypes.c_uint64)]


class H2RPairingConfig(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("num_pairs", ctypes.c_uint32), ("negate_mask", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class H2RSetupConfig(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("mode", ctypes.c_uint32), ("log_n", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("n", ctypes.c_uint64), ("tau", ctypes.c_uint64 * 4), ("omega", ctypes.c_uint64 * 4)]


class H2RKeygenSigmaInfo(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("hook_rounds", ctypes.c_uint32), ("touched_cells", ctypes.c_uint32), ("sort_passes", ctypes.c_uint32)]


class H2RFixedRow(ctypes.Structure):
    NAMES = ("sa", "sb", "sc", "sd", "se", "s_mul_ab", "s_mul_cd", "se_next", "s_const")
    _fields_ = [(nm, ctypes.c_uint64 * 4) for nm in NAMES] + [("tag_composition", ctypes.c_uint32), ("tag_overflow", ctypes.c_uint32)]

    def as_dict(self):
        d = {nm: sum(int(getattr(self, nm)[k]) << (64 * k) for k in range(4)) for nm in self.NAMES}
        d["tag_composition"], d["tag_overflow"] = int(self.tag_composition), int(self.tag_overflow)
        return d


class H2RError(RuntimeError):
    def __init__(self, code, where):
        self.code = code
        msg = lib().h2r_status_str(code).decode()
        if code == H2R_E_HIP:
            msg += " (" + lib().h2r_last_hip_error().decode() + ")"
        super().__init__("%s: h2r status %d: %s" % (where, code, msg))


_lib = None
EXPORTS = ["h2r_ctx_create", "h2r_ctx_create_ex", "h2r_ctx_advice_repr", "h2r_abi_version", "h2r_build_id", "h2r_ctx_destroy", "h2r_compute_range_lens", "h2r_rsa_compute_range_lens",
           "h2r_trace_layout", "h2r_pow_fixed_layout", "h2r_pow_var_layout", "h2r_workspace_bytes",
           "h2r_key_table_bytes", "h2r_key_table_build", "h2r_key_table_expand",
           "h2r_mul_mod_batch", "h2r_square_mod_batch", "h2r_pow_mod_fixed_exp_batch", "h2r_pow_mod_batch",
           "h2r_modpow_public_key_batch", "h2r_modpow_public_key_var_batch", "h2r_pipeline_create", "h2r_pipeline_create_ex", "h2r_pipeline_destroy",
           "h2r_pipeline_modpow_public_key", "h2r_pipeline_modpow_public_key_advice", "h2r_pipeline_modpow_public_key_var", "h2r_pipeline_verify_pkcs1v15", "h2r_pipeline_join", "h2r_pipeline_info", "h2r_pipeline_set_form", "h2r_pipeline_call_plan", "h2r_exp_segment_plan", "h2r_arena_create", "h2r_arena_create_ex", "h2r_image_arena_create", "h2r_arena_region", "h2r_arena_region_bytes", "h2r_arena_region_ms", "h2r_arena_measurements", "h2r_arena_restore_constants", "h2r_arena_destroy", "h2r_verify_layout_fixed", "h2r_verify_pkcs1v15_batch",
           "h2r_verify_trace_flatten", "h2r_fresh_op_layout", "h2r_fresh_op_batch", "h2r_fresh_op_flatten",
           "h2r_mul_stream_bytes", "h2r_is_equal_muled_stream_bytes", "h2r_refresh_stream_bytes", "h2r_mul_batch",
           "h2r_mul_trace_flatten", "h2r_is_equal_muled_batch", "h2r_is_equal_muled_flatten", "h2r_refresh_batch",
           "h2r_mul_stream_bytes_ex", "h2r_mul_batch_ex", "h2r_mul_trace_flatten_ex", "h2r_refresh_layout", "h2r_refresh_batch_ex",
           "h2r_is_equal_muled_stream_bytes_ex", "h2r_is_equal_muled_batch_ex",
           "h2r_range_decompose_batch", "h2r_hist_len", "h2r_trace_lookup_hist", "h2r_lookups_per_record",
           "h2r_trace_lookup_permutation", "h2r_trace_lookup_permutation_hist",
           "h2r_trace_flatten", "h2r_pow_trace_flatten", "h2r_stream_bytes", "h2r_pow_stream_bytes", "h2r_trace_flatten_ex",
           "h2r_pow_trace_flatten_ex", "h2r_trace_emit_stream", "h2r_pow_trace_emit_stream", "h2r_mul_mod_trace_check", "h2r_pow_trace_check",
           "h2r_modpow_public_key_advice_rows", "h2r_modpow_public_key_emit_advice",
           "h2r_advice_copy_map", "h2r_pow_operand_sources", "h2r_advice_layout_default", "h2r_advice_layout_custom", "h2r_advice_fixed_row_ex",
           "h2r_advice_apply_layout", "h2r_advice_check", "h2r_pow_copy_map", "h2r_fresh_op_copy_map", "h2r_verify_circuit_rows", "h2r_verify_circuit_row_kinds",
           "h2r_verify_circuit_emit_frame", "h2r_verify_circuit_copy_map", "h2r_lookup_hist_advice",
           "h2r_advice_rows", "h2r_mul_mod_emit_advice", "h2r_pow_trace_emit_advice", "h2r_pow_advice_rows", "h2r_pow_row_kinds", "h2r_advice_row_kinds",
           "h2r_advice_fixed_row", "h2r_fresh_op_advice_rows", "h2r_fresh_op_row_kinds", "h2r_fresh_op_emit_advice",
           "h2r_verify_advice_rows", "h2r_verify_row_kinds", "h2r_verify_emit_advice", "h2r_verify_layout_compact", "h2r_pipeline_verify_pkcs1v15_advice", "h2r_pow_layout_compact", "h2r_pipeline_modpow_public_key_var_advice", "h2r_pipeline_verify_pkcs1v15_var_advice", "h2r_verify_layout_var", "h2r_verify_pkcs1v15_var_batch", "h2r_pipeline_verify_pkcs1v15_var",
           "h2r_sha256_hashed_msg_batch", "h2r_signature_verifier_batch", "h2r_pipeline_signature_verifier", "h2r_hashed_msg_advice_rows", "h2r_hashed_msg_row_kinds",
           "h2r_hashed_msg_emit_advice",
           "h2r_lookup_config_default", "h2r_lookup_config_custom", "h2r_lookup_table_image", "h2r_lookup_hist_records",
           "h2r_lookup_hist_values", "h2r_lookup_hist_values_strided", "h2r_lookup_hist_verify", "h2r_lookup_hist_fresh_op", "h2r_lookup_workspace_bytes", "h2r_lookup_permuted_columns", "h2r_field_eval",
           "h2r_lookup_input_columns", "h2r_lookup_product_workspace_bytes", "h2r_lookup_product_columns",
           "h2r_permutation_sets", "h2r_permutation_product_workspace_bytes", "h2r_permutation_product_columns",
           "h2r_ntt_workspace_bytes", "h2r_ntt_columns", "h2r_quotient_sets", "h2r_quotient_columns",
           "h2r_open_queries", "h2r_open_workspace_bytes", "h2r_open_eval_columns", "h2r_open_witness_columns", "h2r_fold_columns",
           "h2r_msm_plan", "h2r_msm_workspace_bytes", "h2r_msm_columns", "h2r_curve_eval",
           "h2r_curve_ntt_workspace_bytes", "h2r_curve_ntt",
           "h2r_transcript_state_bytes", "h2r_transcript_round", "h2r_transcript_eval",
           "h2r_random_columns", "h2r_random_eval",
           "h2r_proof_decode", "h2r_verify_bases", "h2r_verify_scalars", "h2r_msm_terms", "h2r_verify_eval",
           "h2r_pairing_prepare", "h2r_pairing_products", "h2r_pairing_eval",
           "h2r_keygen_fixed_workspace_bytes", "h2r_keygen_fixed_columns", "h2r_keygen_sigma_workspace_bytes", "h2r_keygen_sigma_columns", "h2r_keygen_vk_repr",
           "h2r_fixed_base_table", "h2r_fixed_base_mul", "h2r_fixed_base_eval", "h2r_kzg_setup_scalars", "h2r_g2_mul", "h2r_g2_generator",
           "h2r_dist_unique_id", "h2r_dist_init", "h2r_dist_destroy", "h2r_dist_rank", "h2r_dist_world", "h2r_dist_version", "h2r_dist_shard_range",
           "h2r_dist_bcast", "h2r_dist_gather_results", "h2r_dist_allreduce_max_f64",
           "h2r_profile_enable", "h2r_profile_read", "h2r_status_str",
           "h2r_last_hip_error"]
H2R_ADVICE_ASSERT_ONE = 0x100
H2R_ADVICE_DIRECT = 0x200
KERNEL_CHAIN, KERNEL_TRACE, KERNEL_HIST, KERNEL_AUX, KERNEL_EMIT, KERNEL_STEP, KERNEL_LOOKUP, KERNEL_SHA256, KERNEL_CELLS = 0, 1, 2, 3, 4, 5, 6, 7, 8
KERNEL_LOOKUP_INPUT, KERNEL_LOOKUP_PRODUCT_TILES, KERNEL_LOOKUP_PRODUCT_CARRY, KERNEL_LOOKUP_PRODUCT_SCAN = 9, 10, 11, 12
KERNEL_PERM_PRODUCT_TILES, KERNEL_PERM_PRODUCT_CARRY, KERNEL_PERM_PRODUCT_SCAN = 13, 14, 15
KERNEL_NTT_SETUP, KERNEL_NTT_PASS = 16, 17
KERNEL_QUOTIENT = 18
KERNEL_OPEN_TILES, KERNEL_OPEN_CARRY, KERNEL_OPEN_SCAN, KERNEL_FOLD = 19, 20, 21, 22
KERNEL_MSM_BUCKET, KERNEL_MSM_FOLD = 23, 24
KERNEL_CURVE_NTT_TWIDDLE, KERNEL_CURVE_NTT_LOAD, KERNEL_CURVE_NTT_STAGE, KERNEL_CURVE_NTT_STORE = 25, 26, 27, 28
KERNEL_TRANSCRIPT = 29
KERNEL_RANDOM = 30
KERNEL_PROOF_DECODE, KERNEL_VERIFY_SCALARS, KERNEL_MSM_TERMS = 31, 32, 33
KERNEL_PAIRING = 34
KERNEL_KEYGEN_FIXED, KERNEL_KEYGEN_COMPONENTS, KERNEL_KEYGEN_COMPACT, KERNEL_KEYGEN_SORT, KERNEL_KEYGEN_WRITE = 35, 36, 37, 38, 39
KERNEL_FIXED_BASE_TABLE, KERNEL_FIXED_BASE_MUL, KERNEL_SETUP_SCALARS = 40, 41, 42
H2R_KEYGEN_NUM_FIXED = 15
H2R_FIXED_BASE_TABLE_BYTES, H2R_FIXED_BASE_MAX_POINTS = 524288, 1 << 24
H2R_SETUP_POWERS, H2R_SETUP_LAGRANGE = 0, 1
H2R_PAIRING_STEPS, H2R_PAIRING_TABLE_BYTES, H2R_PAIRING_MAX_PAIRS = 102, 13056, 4
FIELD_MUL, FIELD_TO_MONTGOMERY, FIELD_FROM_MONTGOMERY = 2, 6, 7   # h2r_field_eval's operations a * b, a * R and a * R^-1 mod p (include/h2r.h)
H2R_HASHED_MSG_STREAM_BYTES = 288
H2R_STREAM_FIELD_AB = 1
FRESH_OPS = ["add", "sub", "add_mod", "sub_mod", "is_zero", "is_equal_fresh", "is_less_than", "is_less_than_or_equal",
             "is_greater_than", "is_greater_than_or_equal", "is_in_field"]


def lib_path():
    # H2R_LIB: developer override used by tools/ for same-box A/B runs of build variants
    return os.environ.get("H2R_LIB") or _build.LIB


def lib():
    """Load libh2r.so.  `import torch` must happen first so that the HIP runtime torch ships
    (same SONAME libamdhip64.so.7) is the one both share."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError("libh2r.so is not built (%s). Run `python -m halo2_rsa_amd._build`; there is no CPU fallback." % path)
    try:
        import torch  # noqa: F401  (loads torch's libamdhip64 first)
    except Exception:  # pragma: no cover - torch-less use links /opt/rocm's runtime
        pass
    L = ctypes.CDLL(path)
    vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int32
    L.h2r_ctx_create.argtypes = [ctypes.POINTER(H2RParams), ctypes.POINTER(vp)]
    L.h2r_ctx_create_ex.argtypes = [ctypes.POINTER(H2RParams), ctypes.POINTER(H2RAdviceRepr), ctypes.POINTER(vp)]
    L.h2r_ctx_advice_repr.argtypes = [vp, ctypes.POINTER(H2RAdviceRepr)]
    L.h2r_abi_version.argtypes = []
    L.h2r_abi_version.restype = u32
    L.h2r_build_id.argtypes = []
    L.h2r_build_id.restype = ctypes.c_char_p
    L.h2r_ctx_destroy.argtypes = [vp]
    L.h2r_ctx_destroy.restype = None
    L.h2r_compute_range_lens.argtypes = [u32, u32, ctypes.POINTER(u32), ctypes.POINTER(u32)]
    L.h2r_rsa_compute_range_lens.argtypes = [u32, ctypes.POINTER(u32), ctypes.POINTER(u32)]
    L.h2r_trace_layout.argtypes = [vp, ctypes.POINTER(H2RLayout)]
    L.h2r_pow_fixed_layout.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(H2RPowLayout)]
    L.h2r_pow_var_layout.argtypes = [vp, u32, u32, ctypes.POINTER(H2RPowLayout)]
    L.h2r_workspace_bytes.argtypes = [vp, u64, u32]
    L.h2r_workspace_bytes.restype = u64
    L.h2r_key_table_bytes.argtypes = [vp, u64]
    L.h2r_key_table_bytes.restype = u64
    L.h2r_key_table_build.argtypes = [vp, vp, u64, vp, vp, vp]
    L.h2r_key_table_expand.argtypes = [vp, vp, u64, vp, u64, vp, vp]
    L.h2r_mul_mod_batch.argtypes = [vp, vp, vp, vp, u64, u32, vp, vp, vp, vp, vp]
    L.h2r_square_mod_batch.argtypes = [vp, vp, vp, u64, u32, vp, vp, vp, vp, vp]
    L.h2r_pow_mod_fixed_exp_batch.argtypes = [vp, vp, vp, ctypes.c_char_p, ctypes.c_size_t, u64, u32, vp, vp, vp, vp, vp]
    L.h2r_modpow_public_key_batch.argtypes = [vp, vp, vp, ctypes.c_char_p, ctypes.c_size_t, u64, u32, vp, vp, vp, vp, vp, vp]
    L.h2r_pow_mod_batch.argtypes = [vp, vp, vp, u32, u32, vp, u64, u32, vp, vp, vp, vp, vp]
    L.h2r_modpow_public_key_var_batch.argtypes = [vp, vp, vp, u32, u32, vp, u64, u32, vp, vp, vp, vp, vp, vp]
    L.h2r_pipeline_create.argtypes = [vp, ctypes.POINTER(vp)]
    L.h2r_pipeline_create_ex.argtypes = [vp, u32, u32, ctypes.POINTER(vp)]
    L.h2r_pipeline_destroy.argtypes = [vp]
    L.h2r_pipeline_destroy.restype = None
    L.h2r_pipeline_modpow_public_key.argtypes = L.h2r_modpow_public_key_batch.argtypes
    L.h2r_pipeline_modpow_public_key_advice.argtypes = [vp, vp, vp, ctypes.c_char_p, ctypes.c_size_t, u64, u32, vp, vp, vp, vp, vp, u64, vp]
    L.h2r_pipeline_modpow_public_key_var.argtypes = [vp, vp, vp, u32, u32, vp, u64, u32, vp, vp, vp, vp, vp, vp]
    L.h2r_pow_layout_compact.argtypes = [vp, ctypes.POINTER(H2RPowLayout), ctypes.POINTER(H2RPowLayout)]
    L.h2r_pipeline_modpow_public_key_var_advice.argtypes = [vp, vp, vp, u32, u32, vp, u64, u32, vp, vp, vp, vp, vp, vp, u64, vp]
    L.h2r_pipeline_verify_pkcs1v15_var_advice.argtypes = [vp, vp, vp, vp, u32, u32, vp, u64, u32, vp, vp, vp, vp, vp, vp, u64, vp]
    L.h2r_lookup_hist_advice.argtypes = [vp, vp, vp, vp, u64, vp, u64, u64, vp, vp, vp]
    L.h2r_verify_layout_compact.argtypes = [vp, ctypes.POINTER(H2RVerifyLayout), ctypes.POINTER(H2RVerifyLayout)]
    L.h2r_pipeline_verify_pkcs1v15_advice.argtypes = [vp, vp, vp, ctypes.c_char_p, ctypes.c_size_t, vp, u64, u32, vp, vp, vp, vp, vp, vp, u64, vp]
    L.h2r_pipeline_join.argtypes = [vp, vp]
    L.h2r_pipeline_info.argtypes = [vp, vp, u64, ctypes.POINTER(H2RPipelineInfo)]
    L.h2r_arena_create.argtypes = [vp, u64, u64, u32, u64, u32, u32, vp, ctypes.POINTER(vp)]
    L.h2r_arena_create_ex.argtypes = [vp, u64, u64, u32, u64, u32, u32, u64, vp, ctypes.POINTER(vp)]
    L.h2r_image_arena_create.argtypes = [vp, u64, u32, u32, u64, vp, ctypes.POINTER(vp)]
    L.h2r_dist_version.argtypes = []
    L.h2r_dist_version.restype = ctypes.c_int32
    L.h2r_arena_region.argtypes = [vp, u32]
    L.h2r_arena_region.restype = vp
    L.h2r_arena_region_bytes.argtypes = [vp]
    L.h2r_arena_region_bytes.restype = u64
    L.h2r_arena_region_ms.argtypes = [vp, u32]
    L.h2r_arena_region_ms.restype = ctypes.c_double
    L.h2r_arena_measurements.argtypes = [vp, ctypes.POINTER(ctypes.c_double), u32]
    L.h2r_arena_measurements.restype = u32
    L.h2r_arena_destroy.argtypes = [vp]
    L.h2r_arena_restore_constants.argtypes = [vp, u32, vp]
    L.h2r_pipeline_set_form.argtypes = [vp, u32]
    L.h2r_arena_destroy.restype = None
    L.h2r_exp_segment_plan.argtypes = [vp, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32),
                                       ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
    L.h2r_pipeline_call_plan.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32,
                                         ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    L.h2r_verify_layout_fixed.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(H2RVerifyLayout)]
    L.h2r_verify_pkcs1v15_batch.argtypes = [vp, vp, vp, ctypes.c_char_p, ctypes.c_size_t, vp, u64, u32, vp, vp, vp, vp, vp, vp]
    L.h2r_verify_trace_flatten.argtypes = [vp, ctypes.POINTER(H2RVerifyLayout), vp, vp]
    L.h2r_verify_layout_var.argtypes = [vp, u32, u32, ctypes.POINTER(H2RVerifyLayout)]
    L.h2r_verify_pkcs1v15_var_batch.argtypes = [vp, vp, vp, vp, u32, u32, vp, u64, u32, vp, vp, vp, vp, vp, vp]
    L.h2r_pipeline_verify_pkcs1v15_var.argtypes = [vp, vp, vp, vp, u32, u32, vp, u64, u32, vp, vp, vp, vp, vp, vp]
    L.h2r_pipeline_verify_pkcs1v15.argtypes = L.h2r_verify_pkcs1v15_batch.argtypes
    L.h2r_fresh_op_layout.argtypes = [vp, u32, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u32)]
    L.h2r_fresh_op_batch.argtypes = [vp, u32, vp, vp, vp, u64, u32, vp, vp, vp, vp, vp]
    L.h2r_fresh_op_flatten.argtypes = [vp, u32, vp, vp]
    for nm in ("h2r_mul_stream_bytes", "h2r_is_equal_muled_stream_bytes", "h2r_refresh_stream_bytes"):
        getattr(L, nm).argtypes = [vp]
        getattr(L, nm).restype = u64
    L.h2r_mul_batch.argtypes = [vp, vp, vp, u64, vp, vp, vp]
    L.h2r_mul_trace_flatten.argtypes = [vp, vp, vp]
    L.h2r_is_equal_muled_batch.argtypes = [vp, vp, vp, u64, vp, vp, vp]
    L.h2r_is_equal_muled_flatten.argtypes = [vp, vp, vp]
    L.h2r_refresh_batch.argtypes = [vp, vp, u64, vp, vp, vp, vp]
    L.h2r_mul_stream_bytes_ex.argtypes = [vp, u32, u32]
    L.h2r_mul_stream_bytes_ex.restype = u64
    L.h2r_mul_batch_ex.argtypes = [vp, vp, u32, vp, u32, u64, vp, vp, vp]
    L.h2r_mul_trace_flatten_ex.argtypes = [vp, vp, u32, u32, vp]
    L.h2r_refresh_layout.argtypes = [vp, u32, u32, ctypes.POINTER(u32), ctypes.POINTER(u64), ctypes.POINTER(u64)]
    L.h2r_refresh_batch_ex.argtypes = [vp, vp, u64, u32, u32, u64, vp, vp, vp, vp]
    L.h2r_is_equal_muled_stream_bytes_ex.argtypes = [vp, u32, u32, u32]
    L.h2r_is_equal_muled_stream_bytes_ex.restype = u64
    L.h2r_is_equal_muled_batch_ex.argtypes = [vp, vp, vp, u64, u32, u32, u64, u32, vp, u64, vp, vp]
    L.h2r_range_decompose_batch.argtypes = [vp, vp, u32, u64, u32, u32, vp, u32, vp, vp]
    L.h2r_hist_len.argtypes = [vp]
    L.h2r_hist_len.restype = u32
    L.h2r_trace_lookup_hist.argtypes = [vp, vp, u64, u64, u64, u32, vp, vp]
    L.h2r_lookups_per_record.argtypes = [vp]
    L.h2r_lookups_per_record.restype = u32
    L.h2r_trace_lookup_permutation.argtypes = [vp, vp, u64, u64, u64, u32, vp, vp, vp]
    L.h2r_trace_lookup_permutation_hist.argtypes = [vp, vp, u64, u64, u64, u32, vp, vp, vp, vp]
    L.h2r_trace_flatten.argtypes = [vp, vp, vp]
    L.h2r_pow_trace_flatten.argtypes = [vp, ctypes.POINTER(H2RPowLayout), vp, vp]
    L.h2r_stream_bytes.argtypes = [vp, u32]
    L.h2r_stream_bytes.restype = u64
    L.h2r_pow_stream_bytes.argtypes = [vp, ctypes.POINTER(H2RPowLayout), u32]
    L.h2r_pow_stream_bytes.restype = u64
    L.h2r_trace_flatten_ex.argtypes = [vp, vp, u32, vp]
    L.h2r_pow_trace_flatten_ex.argtypes = [vp, ctypes.POINTER(H2RPowLayout), vp, u32, vp]
    L.h2r_trace_emit_stream.argtypes = [vp, vp, u64, u32, vp, u64, u64, vp]
    L.h2r_pow_trace_emit_stream.argtypes = [vp, ctypes.POINTER(H2RPowLayout), vp, u64, u64, u32, vp, u64, u64, vp]
    L.h2r_advice_rows.argtypes = [vp]
    L.h2r_advice_rows.restype = u32
    L.h2r_pow_advice_rows.argtypes = [vp, ctypes.POINTER(H2RPowLayout)]
    L.h2r_pow_advice_rows.restype = u64
    L.h2r_advice_row_kinds.argtypes = [vp, vp]
    L.h2r_advice_fixed_row.argtypes = [vp, ctypes.POINTER(H2RLookupConfig), u32, ctypes.POINTER(H2RFixedRow)]
    L.h2r_fresh_op_advice_rows.argtypes = [vp, u32, u32]
    L.h2r_fresh_op_advice_rows.restype = u32
    L.h2r_fresh_op_row_kinds.argtypes = [vp, u32, u32, vp]
    L.h2r_fresh_op_emit_advice.argtypes = [vp, u32, u32, vp, vp, vp, vp, u64, u64, u64, vp, vp, u64, vp]
    L.h2r_verify_advice_rows.argtypes = [vp, ctypes.POINTER(H2RVerifyLayout), vp]
    L.h2r_verify_advice_rows.restype = u64
    L.h2r_verify_row_kinds.argtypes = [vp, ctypes.POINTER(H2RVerifyLayout), vp]
    L.h2r_verify_emit_advice.argtypes = [vp, ctypes.POINTER(H2RVerifyLayout), vp, vp, vp, vp, u32, vp, vp, u64, vp, vp, u64, vp]
    L.h2r_sha256_hashed_msg_batch.argtypes = [vp, vp, vp, u64, u64, vp, vp, vp, u64, vp]
    L.h2r_signature_verifier_batch.argtypes = [vp, vp, vp, u64, vp, vp, ctypes.c_char_p, ctypes.c_size_t, u64, u32, vp, vp, u64, vp, vp, vp,
                                               vp, vp, vp, vp]
    L.h2r_pipeline_signature_verifier.argtypes = [vp, vp, vp, u64, vp, vp, ctypes.c_char_p, ctypes.c_size_t, u64, u32, vp, vp, u64, vp, vp, vp,
                                                  vp, vp, vp, vp]
    L.h2r_hashed_msg_advice_rows.argtypes = [vp]
    L.h2r_hashed_msg_advice_rows.restype = u32
    L.h2r_hashed_msg_row_kinds.argtypes = [vp, vp]
    L.h2r_hashed_msg_emit_advice.argtypes = [vp, vp, u64, u64, vp, vp, u64, vp]
    L.h2r_mul_mod_emit_advice.argtypes = [vp, vp, vp, vp, u32, vp, u64, vp, vp, u64, vp]
    L.h2r_pow_row_kinds.argtypes = [vp, ctypes.POINTER(H2RPowLayout), vp]
    L.h2r_advice_copy_map.argtypes = [vp, vp, u32]
    L.h2r_advice_copy_map.restype = u32
    L.h2r_pow_operand_sources.argtypes = [vp, ctypes.POINTER(H2RPowLayout), ctypes.c_char_p, ctypes.c_size_t, vp, vp]
    L.h2r_advice_layout_default.argtypes = [vp]
    L.h2r_advice_layout_custom.argtypes = [vp, vp, vp, u32, vp]
    L.h2r_advice_fixed_row_ex.argtypes = [vp, vp, vp, u32, vp]
    L.h2r_advice_apply_layout.argtypes = [vp, vp, vp, u64, vp, u64, u64, vp, vp]
    L.h2r_advice_check.argtypes = [vp, vp, vp, vp, u64, vp, u64, u64, vp, vp, u64, vp, vp, vp, u32, vp, vp, vp]
    L.h2r_pow_copy_map.argtypes = [vp, ctypes.POINTER(H2RPowLayout), ctypes.c_char_p, ctypes.c_size_t, u64, vp, u64]
    L.h2r_pow_copy_map.restype = u64
    L.h2r_fresh_op_copy_map.argtypes = [vp, u32, u32, u64, vp, u64]
    L.h2r_fresh_op_copy_map.restype = u64
    L.h2r_verify_circuit_rows.argtypes = [vp, ctypes.POINTER(H2RVerifyLayout), vp]
    L.h2r_verify_circuit_rows.restype = u64
    L.h2r_verify_circuit_row_kinds.argtypes = [vp, ctypes.POINTER(H2RVerifyLayout), vp]
    L.h2r_verify_circuit_emit_frame.argtypes = [vp, ctypes.POINTER(H2RVerifyLayout), vp, vp, vp, vp, u32, u64, vp, vp, u64, vp]
    L.h2r_verify_circuit_copy_map.argtypes = [vp, ctypes.POINTER(H2RVerifyLayout), ctypes.c_char_p, ctypes.c_size_t, vp, u64]
    L.h2r_verify_circuit_copy_map.restype = u64
    L.h2r_modpow_public_key_advice_rows.argtypes = [vp, ctypes.POINTER(H2RPowLayout), vp]
    L.h2r_modpow_public_key_advice_rows.restype = u64
    L.h2r_modpow_public_key_emit_advice.argtypes = [vp, ctypes.POINTER(H2RPowLayout), vp, vp, u32, vp, vp, vp, u64, vp, vp, u64, vp]
    L.h2r_pow_trace_emit_advice.argtypes = [vp, ctypes.POINTER(H2RPowLayout), vp, u32, vp, u64, vp, u64, vp, vp, u64, vp]
    L.h2r_mul_mod_trace_check.argtypes = [vp, vp, vp, vp, u32, vp, u64, vp, vp, vp, vp]
    L.h2r_pow_trace_check.argtypes = [vp, ctypes.POINTER(H2RPowLayout), vp, vp, ctypes.c_char_p, ctypes.c_size_t, u32, vp, u64, vp, u64, vp,
                                      vp, vp, vp]
    pcfg, pu32, pu64 = ctypes.POINTER(H2RLookupConfig), ctypes.POINTER(u32), ctypes.POINTER(u64)
    L.h2r_lookup_config_default.argtypes = [vp, u32, pcfg]
    L.h2r_lookup_config_custom.argtypes = [pu32, pu32, u32, pcfg]
    L.h2r_lookup_table_image.argtypes = [vp, pcfg, vp, vp]
    L.h2r_lookup_hist_records.argtypes = [vp, pcfg, vp, u64, u64, u64, u32, vp, vp, vp]
    L.h2r_lookup_hist_values.argtypes = [vp, pcfg, vp, u32, u64, u64, u32, u32, vp, vp]
    L.h2r_lookup_hist_values_strided.argtypes = [vp, pcfg, vp, u32, u64, u64, u64, u64, u32, u32, vp, vp, vp]
    L.h2r_lookup_hist_verify.argtypes = [vp, pcfg, ctypes.POINTER(H2RVerifyLayout), vp, u64, vp, vp, vp]
    L.h2r_lookup_hist_fresh_op.argtypes = [vp, pcfg, u32, vp, u64, u64, u64, vp, vp]
    L.h2r_lookup_workspace_bytes.argtypes = [pcfg, u64]
    L.h2r_lookup_workspace_bytes.restype = u64
    L.h2r_lookup_permuted_columns.argtypes = [vp, pcfg, vp, vp, u64, u32, u32, vp, vp, u64, vp, vp, vp]
    L.h2r_lookup_input_columns.argtypes = [vp, pcfg, vp, vp, u64, vp, u64, u64, vp, vp, u32, u32, u32, vp, u64, vp]
    L.h2r_lookup_product_workspace_bytes.argtypes = [u32, u64]
    L.h2r_lookup_product_workspace_bytes.restype = u64
    L.h2r_lookup_product_columns.argtypes = [vp, pcfg, vp, vp, vp, u64, vp, vp, vp, u64, u32, u32, vp, u64, u64, vp, vp, vp]
    pperm = ctypes.POINTER(H2RPermutationConfig)
    L.h2r_permutation_sets.argtypes = [pperm]
    L.h2r_permutation_sets.restype = u32
    L.h2r_permutation_product_workspace_bytes.argtypes = [pperm, u32, u64]
    L.h2r_permutation_product_workspace_bytes.restype = u64
    L.h2r_permutation_product_columns.argtypes = [vp, pperm, vp, u64, u64, u32, u64, vp, u64, u64, vp, u64, vp, vp, u32, vp, u64, u64, vp, vp, vp]
    pntt = ctypes.POINTER(H2RNttConfig)
    L.h2r_ntt_workspace_bytes.argtypes = [pntt]
    L.h2r_ntt_workspace_bytes.restype = u64
    L.h2r_ntt_columns.argtypes = [vp, pntt, vp, u64, u64, vp, u64, u64, u32, u64, vp, vp]
    pquot = ctypes.POINTER(H2RQuotientConfig)
    L.h2r_quotient_sets.argtypes = [pquot, ctypes.POINTER(u32), ctypes.POINTER(u32)]
    L.h2r_quotient_sets.restype = u32
    L.h2r_quotient_columns.argtypes = [vp, pquot, ctypes.POINTER(H2RQuotientInputs), u64, vp, u64, vp, vp]
    popen, pcols = ctypes.POINTER(H2ROpenConfig), ctypes.POINTER(H2ROpenColumn)
    L.h2r_open_queries.argtypes = [popen, pcols, ctypes.POINTER(u32)]
    L.h2r_open_queries.restype = u32
    L.h2r_open_workspace_bytes.argtypes = [popen, pcols, u64]
    L.h2r_open_workspace_bytes.restype = u64
    L.h2r_open_eval_columns.argtypes = [vp, popen, pcols, vp, u64, vp, vp, vp, vp]
    L.h2r_open_witness_columns.argtypes = [vp, popen, pcols, vp, vp, u64, vp, u64, u64, vp, vp, vp, vp]
    L.h2r_fold_columns.argtypes = [vp, vp, u64, u64, u32, u32, vp, u64, vp, u64, vp, vp]
    L.h2r_field_eval.argtypes = [vp, u32, pu64, pu64, pu64]
    pmsm, pmcols = ctypes.POINTER(H2RMsmConfig), ctypes.POINTER(H2RMsmColumn)
    L.h2r_msm_plan.argtypes = [pmsm, u64, ctypes.POINTER(H2RMsmInfo)]
    L.h2r_msm_plan.restype = u64
    L.h2r_msm_workspace_bytes.argtypes = [pmsm, u64]
    L.h2r_msm_workspace_bytes.restype = u64
    L.h2r_msm_columns.argtypes = [vp, pmsm, pmcols, vp, u64, vp, vp, vp, vp]
    L.h2r_curve_eval.argtypes = [vp, u32, pu64, pu64, pu64]
    L.h2r_curve_ntt_workspace_bytes.argtypes = [ctypes.POINTER(H2RCurveNttConfig)]
    L.h2r_curve_ntt_workspace_bytes.restype = u64
    L.h2r_curve_ntt.argtypes = [vp, ctypes.POINTER(H2RCurveNttConfig), vp, vp, vp, vp]
    L.h2r_transcript_state_bytes.argtypes = []
    L.h2r_transcript_state_bytes.restype = u64
    L.h2r_transcript_round.argtypes = [vp, ctypes.POINTER(H2RTranscriptConfig), ctypes.POINTER(H2RTranscriptItem), ctypes.POINTER(H2RTranscriptDerive),
                                       vp, u64, vp, vp, vp, u64, u64, vp, vp]
    L.h2r_transcript_eval.argtypes = [vp, u32, vp, ctypes.c_char_p, u64, pu64]
    L.h2r_random_columns.argtypes = [vp, ctypes.POINTER(H2RRandomConfig), ctypes.POINTER(H2RRandomColumn), u64, vp]
    L.h2r_random_eval.argtypes = [vp, ctypes.c_char_p, u64, u32, u64, pu64]
    pvs = ctypes.POINTER(H2RVerifyScalarsConfig)
    L.h2r_proof_decode.argtypes = [vp, ctypes.POINTER(H2RProofDecodeConfig), ctypes.POINTER(H2RProofSection), vp, u64, u64, vp, u64, vp, u64, vp, vp]
    L.h2r_verify_bases.argtypes = [pvs, pu32]
    L.h2r_verify_bases.restype = u32
    L.h2r_verify_scalars.argtypes = [vp, pvs, vp, u64, ctypes.POINTER(H2RVerifyChallenges), u64, vp, u64, vp, vp, vp]
    L.h2r_msm_terms.argtypes = [vp, ctypes.POINTER(H2RMsmTermsConfig), vp, u64, vp, u64, u64, vp, vp, vp]
    L.h2r_verify_eval.argtypes = [vp, u32, pvs, ctypes.c_char_p, u64, vp, u64]
    L.h2r_pairing_prepare.argtypes = [vp, ctypes.c_char_p, vp]
    L.h2r_pairing_products.argtypes = [vp, ctypes.POINTER(H2RPairingConfig), vp, vp, u64, u64, vp, vp, vp, vp]
    L.h2r_pairing_eval.argtypes = [vp, u32, ctypes.c_char_p, u64, vp, u64]
    L.h2r_keygen_fixed_workspace_bytes.argtypes = [ctypes.POINTER(H2RLookupConfig)]
    L.h2r_keygen_fixed_workspace_bytes.restype = u64
    L.h2r_keygen_fixed_columns.argtypes = [vp, ctypes.POINTER(H2RLookupConfig), ctypes.POINTER(H2RAdviceLayout), vp, u64, u32, u32, u32, vp, u64, vp, vp, vp]
    L.h2r_keygen_sigma_workspace_bytes.argtypes = [u32, u32, u64]
    L.h2r_keygen_sigma_workspace_bytes.restype = u64
    L.h2r_keygen_sigma_columns.argtypes = [vp, ctypes.POINTER(H2RPermutationConfig), vp, u64, u32, u32, u32, vp, u64, vp, vp, ctypes.POINTER(H2RKeygenSigmaInfo), vp]
    L.h2r_keygen_vk_repr.argtypes = [vp, pvs, u32, ctypes.c_char_p, pu64]
    L.h2r_fixed_base_table.argtypes = [vp, ctypes.c_char_p, vp, vp]
    L.h2r_fixed_base_mul.argtypes = [vp, vp, vp, u64, vp, vp]
    L.h2r_fixed_base_eval.argtypes = [vp, u32, pu64, pu64, pu64]
    L.h2r_kzg_setup_scalars.argtypes = [vp, ctypes.POINTER(H2RSetupConfig), vp, vp]
    L.h2r_g2_mul.argtypes = [vp, ctypes.c_char_p, pu64, vp]
    L.h2r_g2_generator.argtypes = [vp, vp]
    L.h2r_dist_unique_id.argtypes = [vp]
    L.h2r_dist_init.argtypes = [vp, vp, u32, u32, ctypes.POINTER(vp)]
    L.h2r_dist_destroy.argtypes = [vp]
    L.h2r_dist_destroy.restype = None
    L.h2r_dist_rank.argtypes = [vp]
    L.h2r_dist_rank.restype = u32
    L.h2r_dist_world.argtypes = [vp]
    L.h2r_dist_world.restype = u32
    L.h2r_dist_shard_range.argtypes = [u64, u32, u32, pu64, pu64]
    L.h2r_dist_bcast.argtypes = [vp, vp, u64, u32, vp]
    L.h2r_dist_gather_results.argtypes = [vp, vp, vp, u64, vp, vp, vp]
    L.h2r_dist_allreduce_max_f64.argtypes = [vp, vp, u64, vp]
    L.h2r_profile_enable.argtypes = [u32]
    L.h2r_profile_read.argtypes = [u32, ctypes.POINTER(ctypes.c_float), u32, ctypes.POINTER(u32)]
    L.h2r_status_str.argtypes = [i32]
    L.h2r_status_str.restype = ctypes.c_char_p
    L.h2r_last_hip_error.restype = ctypes.c_char_p
    for name in EXPORTS:
        fn = getattr(L, name)
        if fn.restype is ctypes.c_int:
            fn.restype = i32
    _lib = L
    return _lib


def check(code, where):
    if code != H2R_OK:
        raise H2RError(code, where)


def profile_enable(capacity):
    check(lib().h2r_profile_enable(capacity), "h2r_profile_enable")


def profile_read(kernel, max_count=1 << 16):
    """Durations (ms) of the recorded launches of one kernel class, in launch order."""
    n = ctypes.c_uint32(0)
    check(lib().h2r_profile_read(kernel, None, 0, ctypes.byref(n)), "h2r_profile_read")
    k = min(n.value, max_count)
    buf = (ctypes.c_float * max(k, 1))()
    check(lib().h2r_profile_read(kernel, buf, k, ctypes.byref(n)), "h2r_profile_read")
    return [float(buf[i]) for i in range(k)]

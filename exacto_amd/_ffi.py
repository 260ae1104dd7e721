"""ctypes binding of the C ABI in include/exacto_hip.h (libexacto_hip.so, built in-tree).

This is the only way the Python side reaches the GPU path; there is no CPU fallback:
if the shared library is missing, importing anything that needs it raises.
"""

from __future__ import annotations

import ctypes as C
import os

import numpy as np

_LIB_PATH = os.environ.get("EXACTO_HIP_LIB") or os.path.join(
    os.path.dirname(os.path.abspath(__file__)), "lib", "libexacto_hip.so")  # env: kernel-variant builds (tools/)

VARIANTS = ("InvalidParam", "DimensionMismatch", "ModulusMismatch", "InvalidRingDegree",
            "DecryptionError", "DecompositionError", "LatticeError", "MissingKey", "NotImplemented")

PATH_EXACT_RNS, PATH_HPS, PATH_SCHOOLBOOK = 0, 1, 2


class ExactoError(Exception):
    """Mirror of reference src/error.rs ExactoError: ``variant`` + Display text."""

    def __init__(self, code: int, message: str):
        super().__init__(message)
        self.code = code
        self.variant = VARIANTS[code - 1] if 1 <= code <= 9 else "HipError"


NTT_ORDER = 1   # exacto_hip.h EXACTO_NTT_ORDER: evaluation k at (k mod 16) n/16 + k/16


class CtxInfo(C.Structure):
    _fields_ = [("ring_degree", C.c_size_t), ("num_ct_moduli", C.c_size_t),
                ("num_aux_moduli", C.c_size_t), ("num_internal_aux", C.c_size_t),
                ("gadget_digits", C.c_size_t), ("gadget_base", C.c_uint64),
                ("plain_modulus", C.c_uint64), ("mul_path", C.c_int), ("device", C.c_int),
                ("ks32_primes", C.c_int), ("psum_max", C.c_int),
                ("ks32_lazy", C.c_int), ("ntt_order", C.c_int), ("dbfv_key_switch", C.c_int)]


_lib = None

# (name, argtypes, restype)
_P = C.c_void_p
_SZ = C.c_size_t
_U64 = C.c_uint64
_SIGS = [
    ("exacto_ctx_create", [C.POINTER(_P), _SZ, _P, _SZ, _P, _SZ, _U64, _U64, C.c_int], C.c_int),
    ("exacto_ctx_destroy", [_P], None),
    ("exacto_ctx_get_info", [_P, C.POINTER(CtxInfo)], C.c_int),
    ("exacto_ctx_set_stream", [_P, _P], C.c_int),
    ("exacto_ctx_set_chunk", [_P, _SZ], C.c_int),
    ("exacto_synchronize", [_P], C.c_int),
    ("exacto_ctx_load_relin_key", [_P, _P, _SZ], C.c_int),
    ("exacto_ctx_load_relin_key_dev", [_P, _P, _SZ], C.c_int),
    ("exacto_ctx_relin_key_buffer", [_P, _SZ], _P),
    ("exacto_ntt_fwd", [_P, _P, _SZ, _SZ], C.c_int),
    ("exacto_ntt_inv", [_P, _P, _SZ, _SZ], C.c_int),
    ("exacto_ntt_fwd_dev", [_P, _P, _SZ, _SZ], C.c_int),
    ("exacto_ntt_inv_dev", [_P, _P, _SZ, _SZ], C.c_int),
    ("exacto_rns_fwd_dev", [_P, _P, _SZ], C.c_int),
    ("exacto_rns_inv_dev", [_P, _P, _SZ], C.c_int),
    ("exacto_rns_add_dev", [_P, _P, _P, _P, _SZ], C.c_int),
    ("exacto_rns_sub_dev", [_P, _P, _P, _P, _SZ], C.c_int),
    ("exacto_rns_neg_dev", [_P, _P, _P, _SZ], C.c_int),
    ("exacto_rns_mul_dev", [_P, _P, _P, _P, _SZ], C.c_int),
    ("exacto_rns_mul_inv_dev", [_P, _P, _P, _P, _SZ], C.c_int),
    ("exacto_rns_polymul_dev", [_P, _P, _P, _P, _SZ], C.c_int),
    ("exacto_rns_scalar_mul_dev", [_P, _P, _U64, _P, _SZ], C.c_int),
    ("exacto_bfv_add", [_P, _P, _SZ, _P, _SZ, _P, _SZ], C.c_int),
    ("exacto_bfv_add_dev", [_P, _P, _SZ, _P, _SZ, _P, _SZ], C.c_int),
    ("exacto_bfv_sub", [_P, _P, _SZ, _P, _SZ, _P, _SZ], C.c_int),
    ("exacto_bfv_sub_dev", [_P, _P, _SZ, _P, _SZ, _P, _SZ], C.c_int),
    ("exacto_bfv_neg", [_P, _P, _SZ, _P, _SZ], C.c_int),
    ("exacto_bfv_neg_dev", [_P, _P, _SZ, _P, _SZ], C.c_int),
    ("exacto_bfv_mul_no_relin", [_P, _P, _SZ, _P, _SZ, _P, _SZ], C.c_int),
    ("exacto_bfv_mul_no_relin_dev", [_P, _P, _SZ, _P, _SZ, _P, _SZ], C.c_int),
    ("exacto_relinearize", [_P, _P, _SZ, _P, _SZ], C.c_int),
    ("exacto_relinearize_dev", [_P, _P, _SZ, _P, _SZ], C.c_int),
    ("exacto_bfv_mul_and_relin", [_P, _P, _P, _P, _SZ], C.c_int),
    ("exacto_bfv_mul_and_relin_dev", [_P, _P, _P, _P, _SZ], C.c_int),
    ("exacto_gadget_decompose_dev", [_P, _P, _P, _SZ, _SZ], C.c_int),
    ("exacto_bfv_square_no_relin", [_P, _P, _SZ, _P, _SZ], C.c_int),
    ("exacto_bfv_square_no_relin_dev", [_P, _P, _SZ, _P, _SZ], C.c_int),
    ("exacto_bfv_square_and_relin", [_P, _P, _P, _SZ], C.c_int),
    ("exacto_bfv_square_and_relin_dev", [_P, _P, _P, _SZ], C.c_int),
    ("exacto_ctx_set_square_hook", [_P, C.c_int], C.c_int),
    ("exacto_dbfv_square", [_P, _SZ, _U64, _U64, _P, _P, _SZ, _P, _P], C.c_int),
    ("exacto_dbfv_square_dev", [_P, _SZ, _U64, _U64, _P, _P, _SZ, _P, _P], C.c_int),
    ("exacto_dbfv_mul_plan", [_SZ, _U64, _U64, C.c_int, _P, _SZ, _P, _P, _P, _SZ, _P], C.c_int),
    ("exacto_dbfv_mul", [_P, _SZ, _U64, _U64, _P, _P, _P, _SZ, _P, _P, _P], C.c_int),
    ("exacto_dbfv_mul_dev", [_P, _SZ, _U64, _U64, _P, _P, _P, _SZ, _P, _P, _P], C.c_int),
    ("exacto_dbfv_mul_chain", [_P, _SZ, _U64, _U64, _P, _P, _P, _SZ, _SZ], C.c_int),
    ("exacto_dbfv_mul_limbs", [_P, _SZ, _U64, _U64, _P, _P, _P, _SZ, _P, _SZ], C.c_int),
    ("exacto_dbfv_mul_limbs_dev", [_P, _SZ, _U64, _U64, _P, _P, _P, _SZ, _P, _SZ], C.c_int),
    ("exacto_bfv_mul_sum", [_P, _P, _SZ, _P, _SZ, _P, _P, _P, _SZ, _SZ, _P, _SZ], C.c_int),
    ("exacto_bfv_mul_sum_dev", [_P, _P, _SZ, _P, _SZ, _P, _P, _P, _SZ, _SZ, _P, _SZ], C.c_int),
    ("exacto_ctx_set_mul_sum_group", [_P, _SZ], C.c_int),
    ("exacto_bfv_mul_sum_info", [_P, C.POINTER(_SZ), C.POINTER(C.c_int)], C.c_int),
    ("exacto_bfv_decrypt", [_P, _P, _SZ, _P, _P, _SZ], C.c_int),
    ("exacto_bfv_decrypt_dev", [_P, _P, _SZ, _P, _P, _SZ], C.c_int),
    ("exacto_dbfv_decrypt", [_P, _SZ, _U64, _U64, _P, _P, _P, _SZ], C.c_int),
    ("exacto_dbfv_decrypt_dev", [_P, _SZ, _U64, _U64, _P, _P, _P, _SZ], C.c_int),
    ("exacto_dbfv_decrypt_poly", [_P, _SZ, _U64, _U64, _P, _P, _P, _SZ], C.c_int),
    ("exacto_dbfv_decrypt_poly_dev", [_P, _SZ, _U64, _U64, _P, _P, _P, _SZ], C.c_int),
    ("exacto_dbfv_mul_chain_dev", [_P, _SZ, _U64, _U64, _P, _P, _P, _SZ, _SZ], C.c_int),
    ("exacto_bfv_mod_switch", [_P, _P, _SZ, _SZ, _SZ, C.c_int, _P, _SZ], C.c_int),
    ("exacto_bfv_mod_switch_dev", [_P, _P, _SZ, _SZ, _SZ, C.c_int, _P, _SZ], C.c_int),
    ("exacto_bfv_noise", [_P, _P, _SZ, _P, _P, _P, _P, _SZ], C.c_int),
    ("exacto_bfv_noise_dev", [_P, _P, _SZ, _P, _P, _P, _P, _SZ], C.c_int),
    ("exacto_dbfv_noise", [_P, _SZ, _P, _P, _P, _SZ], C.c_int),
    ("exacto_dbfv_noise_dev", [_P, _SZ, _P, _P, _P, _SZ], C.c_int),
    *[(f"exacto_dbfv_encrypt_{kind}{sfx}", [_P, _SZ, _U64, _U64, _P, _P, C.c_double, _P, _U64, _P, _SZ], C.c_int)
      for kind in ("sk", "pk", "poly_sk", "poly_pk") for sfx in ("", "_dev")],
    *[(f"exacto_dbfv_{op}{sfx}", [_P, _P, _SZ, _SZ, _P, _SZ, _SZ, _P, _SZ, _P, _P, _P], C.c_int)
      for op in ("add", "sub") for sfx in ("", "_dev")],
    ("exacto_dbfv_neg", [_P, _P, _SZ, _SZ, _P, _SZ], C.c_int),
    ("exacto_dbfv_neg_dev", [_P, _P, _SZ, _SZ, _P, _SZ], C.c_int),
    ("exacto_dbfv_relinearize", [_P, _P, _SZ, _SZ, _P, _SZ], C.c_int),
    ("exacto_dbfv_relinearize_dev", [_P, _P, _SZ, _SZ, _P, _SZ], C.c_int),
    ("exacto_dbfv_apply_automorphism", [_P, _P, _SZ, _SZ, _U64, _P, _SZ, _P, _SZ], C.c_int),
    ("exacto_dbfv_apply_automorphism_dev", [_P, _P, _SZ, _SZ, _U64, _P, _SZ, _P, _SZ], C.c_int),
    ("exacto_dbfv_linear_map", [_P, _SZ, _SZ, _SZ, _P, _P, _P, _SZ], C.c_int),
    ("exacto_dbfv_linear_map_dev", [_P, _SZ, _SZ, _SZ, _P, _P, _P, _SZ], C.c_int),
    ("exacto_dbfv_change_base_matrix", [_SZ, _U64, _U64, _U64, _SZ, _P], C.c_int),
    ("exacto_dbfv_change_base", [_P, _SZ, _U64, _U64, _U64, _SZ, _P, _P, _SZ], C.c_int),
    ("exacto_dbfv_change_base_dev", [_P, _SZ, _U64, _U64, _U64, _SZ, _P, _P, _SZ], C.c_int),
    ("exacto_dbfv_div_by_base", [_P, _SZ, _U64, _U64, _P, _P, _SZ, C.POINTER(_U64)], C.c_int),
    ("exacto_dbfv_div_by_base_dev", [_P, _SZ, _U64, _U64, _P, _P, _SZ, C.POINTER(_U64)], C.c_int),
    ("exacto_gen_secret_key", [_P, _P, _U64, _P], C.c_int),
    ("exacto_gen_secret_key_dev", [_P, _P, _U64, _P], C.c_int),
    ("exacto_gen_public_key", [_P, _P, C.c_double, _P, _U64, _P], C.c_int),
    ("exacto_gen_public_key_dev", [_P, _P, C.c_double, _P, _U64, _P], C.c_int),
    ("exacto_gen_relin_key", [_P, _P, C.c_double, _P, _U64, _SZ, _P], C.c_int),
    ("exacto_gen_relin_key_dev", [_P, _P, C.c_double, _P, _U64, _SZ, _P], C.c_int),
    ("exacto_encrypt_sk", [_P, _P, _P, C.c_double, _P, _U64, _P, _SZ], C.c_int),
    ("exacto_encrypt_sk_dev", [_P, _P, _P, C.c_double, _P, _U64, _P, _SZ], C.c_int),
    ("exacto_encrypt_pk", [_P, _P, _P, C.c_double, _P, _U64, _P, _SZ], C.c_int),
    ("exacto_encrypt_pk_dev", [_P, _P, _P, C.c_double, _P, _U64, _P, _SZ], C.c_int),
    ("exacto_gen_galois_key", [_P, _P, _U64, C.c_double, _P, _U64, _SZ, _P], C.c_int),
    ("exacto_gen_galois_key_dev", [_P, _P, _U64, C.c_double, _P, _U64, _SZ, _P], C.c_int),
    ("exacto_bfv_apply_automorphism", [_P, _P, _SZ, _U64, _P, _SZ, _P, _SZ], C.c_int),
    ("exacto_bfv_apply_automorphism_dev", [_P, _P, _SZ, _U64, _P, _SZ, _P, _SZ], C.c_int),
    ("exacto_batch_info", [_P, C.POINTER(_U64)], C.c_int),
    *[(f"exacto_batch_{op}{sfx}", [_P, _P, _P, _SZ], C.c_int) for op in ("encode", "decode") for sfx in ("", "_dev")],
    ("exacto_galois_element_rotate_rows", [_SZ, C.c_int64, C.POINTER(_U64)], C.c_int),
    ("exacto_galois_element_swap_rows", [_SZ, C.POINTER(_U64)], C.c_int),
    ("exacto_bfv_rotate_rows", [_P, _P, _SZ, C.c_int64, _P, _SZ, _P, _SZ], C.c_int),
    ("exacto_bfv_rotate_rows_dev", [_P, _P, _SZ, C.c_int64, _P, _SZ, _P, _SZ], C.c_int),
    ("exacto_bfv_swap_rows", [_P, _P, _SZ, _P, _SZ, _P, _SZ], C.c_int),
    ("exacto_bfv_swap_rows_dev", [_P, _P, _SZ, _P, _SZ, _P, _SZ], C.c_int),
    *[(f"exacto_batch_encrypt_{kind}{sfx}", [_P, _P, _P, C.c_double, _P, _U64, _P, _SZ], C.c_int)
      for kind in ("sk", "pk") for sfx in ("", "_dev")],
    ("exacto_batch_decrypt", [_P, _P, _SZ, _P, _P, _SZ], C.c_int),
    ("exacto_batch_decrypt_dev", [_P, _P, _SZ, _P, _P, _SZ], C.c_int),
    *[(f"exacto_dbfv_batch_{op}{sfx}", [_P, _SZ, _U64, _U64, _P, _P, _SZ], C.c_int)
      for op in ("encode", "decode") for sfx in ("", "_dev")],
    *[(f"exacto_dbfv_batch_encrypt_{kind}{sfx}", [_P, _SZ, _U64, _U64, _P, _P, C.c_double, _P, _U64, _P, _SZ], C.c_int)
      for kind in ("sk", "pk") for sfx in ("", "_dev")],
    ("exacto_dbfv_batch_decrypt", [_P, _SZ, _U64, _U64, _P, _P, _P, _SZ], C.c_int),
    ("exacto_dbfv_batch_decrypt_dev", [_P, _SZ, _U64, _U64, _P, _P, _P, _SZ], C.c_int),
    *[(f"exacto_dbfv_plain_mul_sum{sfx}", [_P, _SZ, _U64, _U64, _P, _SZ, _SZ, _P, _SZ, _P, _SZ, _P, _P], C.c_int)
      for sfx in ("", "_dev")],
    *[(f"exacto_dbfv_plain_mul{sfx}", [_P, _SZ, _U64, _U64, _P, _SZ, _P, _SZ, _P, _SZ, _P, _P], C.c_int)
      for sfx in ("", "_dev")],
    *[(f"exacto_dbfv_plain_{op}{sfx}", [_P, _SZ, _P, _SZ, _P, _SZ, _P, _SZ], C.c_int)
      for op in ("add", "sub") for sfx in ("", "_dev")],
    ("exacto_ctx_set_plain_terms", [_P, _SZ], C.c_int),
    ("exacto_dbfv_plain_limits", [_P, C.POINTER(_SZ), C.POINTER(_SZ)], C.c_int),
    ("exacto_bfv_plain_mul", [_P, _P, _SZ, _P, _P, _SZ], C.c_int),
    ("exacto_bfv_plain_mul_dev", [_P, _P, _SZ, _P, _P, _SZ], C.c_int),
    ("exacto_bfv_plain_add", [_P, _P, _SZ, _P, _P, _SZ], C.c_int),
    ("exacto_bfv_plain_add_dev", [_P, _P, _SZ, _P, _P, _SZ], C.c_int),
    ("exacto_bfv_inner_product", [_P, _P, _P, _SZ, _SZ, _P], C.c_int),
    ("exacto_bfv_inner_product_dev", [_P, _P, _P, _SZ, _SZ, _P], C.c_int),
    ("exacto_bfv_monomial_mul", [_P, _P, _SZ, _U64, _P, _SZ], C.c_int),
    ("exacto_bfv_monomial_mul_dev", [_P, _P, _SZ, _U64, _P, _SZ], C.c_int),
    ("exacto_bfv_trace", [_P, _P, _SZ, _P, _SZ, _P, _SZ, _P, _SZ], C.c_int),
    ("exacto_bfv_trace_dev", [_P, _P, _SZ, _P, _SZ, _P, _SZ, _P, _SZ], C.c_int),
    ("exacto_required_trace_elements", [_SZ, _P, _SZ], _SZ),
    ("exacto_extract_coefficients", [_P, _P, _U64, _SZ, _P, _SZ, _P, _SZ, _P], C.c_int),
    ("exacto_extract_coefficients_dev", [_P, _P, _U64, _SZ, _P, _SZ, _P, _SZ, _P], C.c_int),
    ("exacto_slots_to_coeffs", [_P, _P, _SZ, _SZ, _P], C.c_int),
    ("exacto_slots_to_coeffs_dev", [_P, _P, _SZ, _SZ, _P], C.c_int),
    ("exacto_lagrange_interpolate", [_P, _SZ, _U64, _P], C.c_int),
    ("exacto_compute_rounding_poly", [_U64, _U64, _U64, _P], C.c_int),
    ("exacto_trivial_encrypt", [_P, _P, _P, _SZ], C.c_int),
    ("exacto_trivial_encrypt_dev", [_P, _P, _P, _SZ], C.c_int),
    ("exacto_eval_poly", [_P, _P, _P, _SZ, _P, _SZ], C.c_int),
    ("exacto_eval_poly_dev", [_P, _P, _P, _SZ, _P, _SZ], C.c_int),
    ("exacto_bootstrap_key_material", [_P, _P, _P, _P, _P], C.c_int),
    ("exacto_bootstrap_key_material_dev", [_P, _P, _P, _P, _P], C.c_int),
    ("exacto_bfv_bootstrap", [_P, _P, _P, _SZ, _P, _P, _SZ, _U64, _P, _SZ, _P, _SZ, _P, _SZ], C.c_int),
    ("exacto_bfv_bootstrap_dev", [_P, _P, _P, _SZ, _P, _P, _SZ, _U64, _P, _SZ, _P, _SZ, _P, _SZ], C.c_int),
    ("exacto_rccl_unique_id", [_P], C.c_int),
    ("exacto_rccl_comm_init", [C.POINTER(_P), C.c_int, _P, C.c_int, C.c_int], C.c_int),
    ("exacto_rccl_comm_destroy", [_P], C.c_int),
    ("exacto_rccl_comm_count", [_P, C.POINTER(C.c_int)], C.c_int),
    ("exacto_ctx_broadcast_relin_key", [_P, _P, C.c_int, _SZ], C.c_int),
    ("exacto_broadcast_galois_key", [_P, _P, C.c_int, _P, _SZ], C.c_int),
    ("exacto_rccl_allgather_u64", [_P, _P, _P, _P, _SZ], C.c_int),
    ("exacto_rccl_sync", [_P, _P], C.c_int),
    ("exacto_galois_ntt_permutation", [_SZ, _U64, _P], C.c_int),
    ("exacto_galois_keyset_create", [_P, _P, _SZ, _P, _SZ, C.POINTER(_P)], C.c_int),
    ("exacto_galois_keyset_create_dev", [_P, _P, _SZ, _P, _SZ, C.POINTER(_P)], C.c_int),
    ("exacto_galois_keyset_destroy", [_P], None),
    ("exacto_galois_keyset_info", [_P, C.POINTER(_SZ), C.POINTER(_SZ), C.POINTER(C.c_int)], C.c_int),
    ("exacto_bfv_rotate_hoisted", [_P, _P, _P, _P, _SZ], C.c_int),
    ("exacto_bfv_rotate_hoisted_dev", [_P, _P, _P, _P, _SZ], C.c_int),
    ("exacto_bfv_linear_transform", [_P, _P, _P, _P, _P, _SZ], C.c_int),
    ("exacto_bfv_linear_transform_dev", [_P, _P, _P, _P, _P, _SZ], C.c_int),
    ("exacto_dbfv_rotate_hoisted", [_P, _P, _SZ, _P, _P, _SZ], C.c_int),
    ("exacto_dbfv_rotate_hoisted_dev", [_P, _P, _SZ, _P, _P, _SZ], C.c_int),
    ("exacto_dbfv_diagonals_create", [_P, _SZ, _SZ, _P, C.POINTER(_P)], C.c_int),
    ("exacto_dbfv_diagonals_create_dev", [_P, _SZ, _SZ, _P, C.POINTER(_P)], C.c_int),
    ("exacto_dbfv_diagonals_destroy", [_P], None),
    ("exacto_ctx_set_dbfv_lt_fused", [_P, C.c_int], C.c_int),
    ("exacto_dbfv_diagonals_info", [_P, C.POINTER(_SZ), C.POINTER(_SZ), C.POINTER(C.c_int)], C.c_int),
    *[(f"exacto_dbfv_linear_transform{sfx}", [_P, _P, _SZ, _U64, _U64, _P, _P, _P, _SZ, _P, _P], C.c_int)
      for sfx in ("", "_dev", "_prepared", "_prepared_dev")],
    ("exacto_last_error", [C.c_char_p, _SZ], _SZ),
    ("exacto_prof_enable", [_P, C.c_int], C.c_int),
    ("exacto_prof_read", [_P, C.c_int, C.POINTER(_U64), C.POINTER(C.c_double),
                          C.POINTER(C.c_double), C.POINTER(_U64)], C.c_int),
    ("exacto_prof_kernels", [_P, C.c_int, C.c_char_p, _SZ], _SZ),
    ("exacto_version", [], C.c_char_p),
]

EXPORTED_SYMBOLS = [s[0] for s in _SIGS]


def lib_path() -> str:
    return _LIB_PATH


def load() -> C.CDLL:
    """Load libexacto_hip.so (raises if it has not been built: no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise RuntimeError(f"{_LIB_PATH} not built; run `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = C.CDLL(_LIB_PATH)
        for name, args, res in _SIGS:
            f = getattr(lib, name)
            f.argtypes = args
            f.restype = res
        _lib = lib
    return _lib


def last_error() -> str:
    lib = load()
    buf = C.create_string_buffer(4096)
    lib.exacto_last_error(buf, 4096)
    return buf.value.decode("utf-8", "replace")


def check(rc: int):
    if rc != 0:
        raise ExactoError(rc, last_error())


def lagrange_interpolate(values, p: int) -> list[int]:
    """digit_extract.rs:37-90 (host-only entry point)."""
    v = np.ascontiguousarray(np.asarray(values, dtype=np.uint64))
    out = np.zeros(max(v.size, 1), dtype=np.uint64)
    check(load().exacto_lagrange_interpolate(v.ctypes.data, v.size, p, out.ctypes.data))
    return [int(x) for x in out[:v.size]]


def compute_rounding_poly(t_orig: int, q_prime: int, t_boot: int) -> list[int]:
    """digit_extract.rs:19-30 (host-only entry point)."""
    out = np.zeros(max(t_boot, 1), dtype=np.uint64)
    check(load().exacto_compute_rounding_poly(t_orig, q_prime, t_boot, out.ctypes.data))
    return [int(x) for x in out[:t_boot]]


def bootstrap_key_material(orig: "HipContext", boot: "HipContext", sk):
    """bfv_host.rs:57-100, 289-330: (boot_sk [Lb][n] NTT domain, s_pt [n]) from sk [1][n]."""
    sk = _u64(sk)
    boot_sk = np.zeros((boot.L, boot.n), dtype=np.uint64)
    s_pt = np.zeros(boot.n, dtype=np.uint64)
    check(load().exacto_bootstrap_key_material(orig._h, boot._h, sk.ctypes.data, boot_sk.ctypes.data,
                                               s_pt.ctypes.data))
    return boot_sk, s_pt


def bfv_bootstrap_raw(orig: "HipContext", boot: "HipContext", ct, bsk, rpoly, q_prime, elements, gks):
    """bfv_host.rs:131-205 batched: ct [B][2][1][n] (orig) -> [B][2][Lb][n] (boot)."""
    ct, bsk, gks = _u64(ct), _u64(bsk), _u64(gks)
    rp = np.ascontiguousarray(np.asarray(rpoly, dtype=np.uint64))
    el = np.ascontiguousarray(np.asarray(elements, dtype=np.uint64))
    E = el.shape[0]
    out = np.zeros((ct.shape[0], 2, boot.L, boot.n), dtype=np.uint64)
    check(load().exacto_bfv_bootstrap(orig._h, boot._h, ct.ctypes.data, ct.shape[1], bsk.ctypes.data,
                                      rp.ctypes.data, rp.size, q_prime, el.ctypes.data if E else None, E,
                                      gks.ctypes.data if E else None, gks.shape[1] if E else 0, out.ctypes.data,
                                      ct.shape[0]))
    return out


def rccl_unique_id() -> bytes:
    """ncclGetUniqueId (128 bytes) through the library's RCCL (exacto_rccl_unique_id)."""
    buf = (C.c_uint8 * 128)()
    check(load().exacto_rccl_unique_id(buf))
    return bytes(buf)


class RcclComm:
    """An RCCL communicator (ncclComm_t) made by the library (exacto_rccl_comm_init) on `device`."""

    def __init__(self, nranks: int, uid: bytes, rank: int, device: int = 0):
        lib = load()
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        h = C.c_void_p()
        check(lib.exacto_rccl_comm_init(C.byref(h), nranks, buf, rank, device))
        self._h, self._lib, self.nranks, self.rank = h, lib, nranks, rank

    @property
    def handle(self):
        return self._h

    def count(self) -> int:
        """ncclCommCount of the library's communicator: the ranks RCCL itself spans."""
        v = C.c_int(0)
        check(self._lib.exacto_rccl_comm_count(self._h, C.byref(v)))
        return v.value

    def close(self):
        if self._h:
            check(self._lib.exacto_rccl_comm_destroy(self._h))
            self._h = None


def required_trace_elements(n: int) -> list[int]:
    """coeffs_to_slots.rs:168-183 (host-only entry point of the library; no GPU needed)."""
    lib = load()
    count = lib.exacto_required_trace_elements(n, None, 0)
    out = (C.c_uint64 * max(count, 1))()
    lib.exacto_required_trace_elements(n, out, count)
    return [int(v) for v in out[:count]]


def galois_element_rotate_rows(n: int, steps: int) -> int:
    """3^(steps mod n/2) mod 2n: the element whose automorphism rotates both slot rows left by `steps`
    (negative: right); host-only entry point."""
    el = C.c_uint64(0)
    check(load().exacto_galois_element_rotate_rows(n, steps, C.byref(el)))
    return int(el.value)


def galois_element_swap_rows(n: int) -> int:
    """2n - 1: the element whose automorphism exchanges the two slot rows; host-only entry point."""
    el = C.c_uint64(0)
    check(load().exacto_galois_element_swap_rows(n, C.byref(el)))
    return int(el.value)


def galois_ntt_permutation(n: int, element: int) -> np.ndarray:
    """perm [n] (uint32) with NTT(sigma_element(a))[p] = NTT(a)[perm[p]] in the library's NTT-domain order, the
    same for every prime; element odd (taken mod 2n); host-only entry point."""
    perm = np.zeros(max(int(n), 1), dtype=np.uint32)
    check(load().exacto_galois_ntt_permutation(n, int(element) % (1 << 64), perm.ctypes.data))
    return perm[:n]


class GaloisKeySet:
    """Galois keys prepared once for hoisted rotations (exacto_galois_keyset_create): the permutation tables
    and the keys in the form the context's key switch consumes.  Holds a reference to its HipContext, so the
    context outlives it; close() (or garbage collection) releases the device memory."""

    def __init__(self, ctx: "HipContext", elements, gks, num_keys: int | None = None, dev: bool = False):
        self.ctx = ctx
        self.elements = [int(e) for e in elements]
        els = _u64(self.elements) if self.elements else None
        if dev:
            gp, nk = ctx._p(gks), int(num_keys or 0)
        else:
            g = None if gks is None else _u64(gks)
            nk = 0 if g is None or g.ndim != 5 else g.shape[1]
            gp = g.ctypes.data if g is not None and g.size else None
        h = C.c_void_p()
        fn = ctx._lib.exacto_galois_keyset_create_dev if dev else ctx._lib.exacto_galois_keyset_create
        check(fn(ctx._h, els.ctypes.data if els is not None else None, len(self.elements), gp, nk, C.byref(h)))
        self._h = h
        r, used, s = C.c_size_t(), C.c_size_t(), C.c_int()
        check(ctx._lib.exacto_galois_keyset_info(h, C.byref(r), C.byref(used), C.byref(s)))
        self.R, self.num_keys_used, self.ks32_primes = int(r.value), int(used.value), int(s.value)

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            self.ctx._lib.exacto_galois_keyset_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DbfvDiagonals:
    """Wide public diagonals lifted once for dBFV linear transforms (exacto_dbfv_diagonals_create): pts
    [R][d][n] plaintext coefficients -> a device buffer [R][d][L][n].  Holds a reference to its HipContext, so
    the context outlives it; close() (or garbage collection) releases the device memory.  `fused`: the route
    a transform of d digits took on that context when the handle was made (False: the staged route, the default;
    True: the fused kernel, after set_dbfv_lt_fused(True))."""

    def __init__(self, ctx: "HipContext", d: int, pts, R: int | None = None, dev: bool = False):
        self.ctx = ctx
        if dev:
            pp, r = ctx._p(pts), int(R or 0)
        else:
            p = _u64(pts)
            if p.ndim != 3 or p.shape[1:] != (d, ctx.n):
                raise ValueError(f"pts must be a [R][{d}][{ctx.n}] array")
            pp, r = (p.ctypes.data if p.size else None), p.shape[0]
        h = C.c_void_p()
        fn = ctx._lib.exacto_dbfv_diagonals_create_dev if dev else ctx._lib.exacto_dbfv_diagonals_create
        check(fn(ctx._h, d, r, pp, C.byref(h)))
        self._h = h
        rr, dd, f = C.c_size_t(), C.c_size_t(), C.c_int()
        check(ctx._lib.exacto_dbfv_diagonals_info(h, C.byref(rr), C.byref(dd), C.byref(f)))
        self.R, self.d, self.fused = int(rr.value), int(dd.value), bool(f.value)

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            self.ctx._lib.exacto_dbfv_diagonals_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def dbfv_change_base_matrix(d: int, base: int, plain: int, new_base: int, new_d: int) -> np.ndarray:
    """advanced.rs:119-130 (host-only entry point): [new_d][d], column i = digits of base^i mod p."""
    out = np.zeros((max(new_d, 1), max(d, 1)), dtype=np.uint64)
    check(load().exacto_dbfv_change_base_matrix(d, base, plain, new_base, new_d, out.ctypes.data))
    return out[:new_d, :d]


def dbfv_mul_plan(d: int, base: int, plain: int, symmetric: bool = False):
    """The plan of dbfv_mul (or, symmetric, of dbfv_square) for the d output limbs, host only
    (exacto_dbfv_mul_plan): (pairs [(i, j)], limbs [[(pair index, coefficient)]])."""
    lib = load()
    np_, nt = C.c_size_t(), C.c_size_t()
    check(lib.exacto_dbfv_mul_plan(d, base, plain, int(symmetric), None, 0, C.byref(np_), None, None, 0, C.byref(nt)))
    pairs = np.zeros((max(np_.value, 1), 2), dtype=np.int32)
    start = np.zeros(d + 1, dtype=np.int32)
    terms = np.zeros((max(nt.value, 1), 2), dtype=np.int64)
    check(lib.exacto_dbfv_mul_plan(d, base, plain, int(symmetric), pairs.ctypes.data, np_.value, C.byref(np_),
                                   start.ctypes.data, terms.ctypes.data, nt.value, C.byref(nt)))
    limbs = [[(int(p), int(c)) for p, c in terms[start[k]:start[k + 1]]] for k in range(d)]
    return [(int(i), int(j)) for i, j in pairs[:np_.value]], limbs


def noise_budget_bits(noise: int, moduli, plain: int) -> int:
    """Bits left before the noise reaches floor(Delta / 2), Delta = floor(Q / p): max(0, bitlen(floor(Delta / 2))
    - bitlen(noise)), an exact integer."""
    Q = 1
    for q in moduli:
        Q *= int(q)
    return max(0, ((Q // int(plain)) // 2).bit_length() - int(noise).bit_length())


def _words_to_ints(words: np.ndarray) -> list[int]:
    """[B][L] little-endian 64-bit words -> B Python ints."""
    return [sum(int(w) << (64 * k) for k, w in enumerate(row)) for row in words]


def _ptr(a) -> int | None:
    """Pointer of a numpy array (host) or a torch tensor (device or host)."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"]
        return a.ctypes.data
    return a.data_ptr()  # torch.Tensor


def _u64(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64))


class HipContext:
    """One device context = BfvParams (+ RnsBasis/NTT plans) on a GPU (exacto_ctx_create)."""

    def __init__(self, ring_degree: int, ct_moduli, aux_moduli=(), plain_modulus: int = 65537,
                 gadget_base: int = 0, device: int = 0):
        lib = load()
        ct = _u64(list(ct_moduli))
        aux = _u64(list(aux_moduli)) if len(aux_moduli) else None
        h = C.c_void_p()
        check(lib.exacto_ctx_create(C.byref(h), ring_degree, ct.ctypes.data, len(ct),
                                    aux.ctypes.data if aux is not None else None,
                                    0 if aux is None else len(aux), plain_modulus, gadget_base,
                                    device))
        self._h = h
        self._lib = lib
        info = CtxInfo()
        check(lib.exacto_ctx_get_info(h, C.byref(info)))
        self.n = info.ring_degree
        self.L = info.num_ct_moduli
        self.G = info.gadget_digits
        self.gadget_base = info.gadget_base
        self.path = info.mul_path
        self.num_internal_aux = info.num_internal_aux
        self.ks32_primes = info.ks32_primes
        self.psum_max = info.psum_max
        self.ct_moduli = [int(q) for q in ct_moduli]
        self.plain_modulus = int(info.plain_modulus)
        # the NTT-domain storage order this binding was written for (exacto_hip.h EXACTO_NTT_ORDER): keys and
        # ciphertexts kept from a library of another order would give wrong results silently
        if info.ntt_order != NTT_ORDER:
            raise RuntimeError(f"libexacto_hip uses NTT-domain order {info.ntt_order}, this binding expects {NTT_ORDER}")

    @property
    def ks32_lazy(self) -> bool:
        """The resident relinearisation key runs in the lazy 31-bit basis (decided at its first use)."""
        info = CtxInfo()
        check(self._lib.exacto_ctx_get_info(self._h, C.byref(info)))
        return bool(info.ks32_lazy)

    @property
    def dbfv_key_switch(self) -> int:
        """The last dbfv_mul's key switch: 1 summed digits (primary 31-bit basis), 2 summed (wide basis),
        0 per product, -1 none yet (exacto_ctx_info.dbfv_key_switch)."""
        info = CtxInfo()
        check(self._lib.exacto_ctx_get_info(self._h, C.byref(info)))
        return int(info.dbfv_key_switch)

    @classmethod
    def from_params(cls, params, device=0):
        """Build from an oracle-style / exacto_amd.params BfvParams object."""
        aux = params.aux_basis.moduli if params.aux_basis is not None else []
        return cls(params.ring_degree, params.ct_basis.moduli, aux, params.plain_modulus,
                   params.gadget_base, device)

    def close(self):
        if self._h:
            self._lib.exacto_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    # ---- configuration
    def set_stream(self, stream_handle: int | None):
        """Enqueue on this hipStream_t handle (0/None = the default stream)."""
        check(self._lib.exacto_ctx_set_stream(self._h, stream_handle or None))

    def set_chunk(self, chunk: int):
        check(self._lib.exacto_ctx_set_chunk(self._h, chunk))

    def set_square_hook(self, on: bool):
        """eval_poly's even baby steps on the square path (default) or as two-operand products (A/B)."""
        check(self._lib.exacto_ctx_set_square_hook(self._h, 1 if on else 0))

    def synchronize(self):
        check(self._lib.exacto_synchronize(self._h))

    # ---- relinearisation key
    def load_relin_key(self, rlk: np.ndarray):
        rlk = _u64(rlk)
        nk = rlk.shape[0] if rlk.ndim == 4 else 0
        check(self._lib.exacto_ctx_load_relin_key(self._h, rlk.ctypes.data if nk else None, nk))

    def load_relin_key_dev(self, rlk_dev, num_keys: int):
        check(self._lib.exacto_ctx_load_relin_key_dev(self._h, _ptr(rlk_dev), num_keys))

    def relin_key_buffer(self, num_keys: int) -> int:
        p = self._lib.exacto_ctx_relin_key_buffer(self._h, num_keys)
        if not p:
            raise ExactoError(100, last_error())
        return p

    # ---- host-pointer API (synchronous, numpy uint64)
    def ntt_fwd(self, polys: np.ndarray, limb: int = 0) -> np.ndarray:
        a = _u64(polys).copy()
        check(self._lib.exacto_ntt_fwd(self._h, a.ctypes.data, a.size // self.n, limb))
        return a

    def ntt_inv(self, polys: np.ndarray, limb: int = 0) -> np.ndarray:
        a = _u64(polys).copy()
        check(self._lib.exacto_ntt_inv(self._h, a.ctypes.data, a.size // self.n, limb))
        return a

    def bfv_mul_no_relin(self, ct1: np.ndarray, ct2: np.ndarray) -> np.ndarray:
        ct1, ct2 = _u64(ct1), _u64(ct2)
        B = ct1.shape[0]
        out = np.zeros((B, 3, self.L, self.n), dtype=np.uint64)
        check(self._lib.exacto_bfv_mul_no_relin(self._h, ct1.ctypes.data, ct1.shape[1],
                                                ct2.ctypes.data, ct2.shape[1], out.ctypes.data, B))
        return out

    def relinearize(self, ct: np.ndarray) -> np.ndarray:
        ct = _u64(ct)
        B, polys = ct.shape[0], ct.shape[1]
        out = np.zeros((B, polys if polys < 3 else 2, self.L, self.n), dtype=np.uint64)
        check(self._lib.exacto_relinearize(self._h, ct.ctypes.data, polys, out.ctypes.data, B))
        return out

    def bfv_mul_and_relin(self, ct1: np.ndarray, ct2: np.ndarray) -> np.ndarray:
        ct1, ct2 = _u64(ct1), _u64(ct2)
        B = ct1.shape[0]
        out = np.zeros((B, 2, self.L, self.n), dtype=np.uint64)
        check(self._lib.exacto_bfv_mul_and_relin(self._h, ct1.ctypes.data, ct2.ctypes.data,
                                                 out.ctypes.data, B))
        return out

    def bfv_square_no_relin(self, ct: np.ndarray) -> np.ndarray:
        """ct [B][2][L][n] -> [B][3][L][n], bit for bit bfv_mul_no_relin(ct, ct)."""
        ct = _u64(ct)
        B = ct.shape[0]
        out = np.zeros((B, 3, self.L, self.n), dtype=np.uint64)
        check(self._lib.exacto_bfv_square_no_relin(self._h, ct.ctypes.data, ct.shape[1], out.ctypes.data, B))
        return out

    def bfv_square_and_relin(self, ct: np.ndarray) -> np.ndarray:
        """ct [B][2][L][n] -> [B][2][L][n], bit for bit bfv_mul_and_relin(ct, ct)."""
        ct = _u64(ct)
        B = ct.shape[0]
        out = np.zeros((B, 2, self.L, self.n), dtype=np.uint64)
        check(self._lib.exacto_bfv_square_and_relin(self._h, ct.ctypes.data, out.ctypes.data, B))
        return out

    def _addsub(self, fn, ct1, ct2):
        ct1, ct2 = _u64(ct1), _u64(ct2)
        B = ct1.shape[0]
        out = np.zeros((B, max(ct1.shape[1], ct2.shape[1]), self.L, self.n), dtype=np.uint64)
        check(fn(self._h, ct1.ctypes.data, ct1.shape[1], ct2.ctypes.data, ct2.shape[1], out.ctypes.data, B))
        return out

    def bfv_add(self, ct1: np.ndarray, ct2: np.ndarray) -> np.ndarray:
        """eval.rs:14-31 batched: ct1 [B][p1][L][n] + ct2 [B][p2][L][n] -> [B][max][L][n]."""
        return self._addsub(self._lib.exacto_bfv_add, ct1, ct2)

    def bfv_sub(self, ct1: np.ndarray, ct2: np.ndarray) -> np.ndarray:
        """eval.rs:34-51 batched (ct2's extra components negated)."""
        return self._addsub(self._lib.exacto_bfv_sub, ct1, ct2)

    def bfv_neg(self, ct: np.ndarray) -> np.ndarray:
        """eval.rs:54-60 batched."""
        ct = _u64(ct)
        out = np.zeros_like(ct)
        check(self._lib.exacto_bfv_neg(self._h, ct.ctypes.data, ct.shape[1], out.ctypes.data, ct.shape[0]))
        return out

    def dbfv_mul(self, d, base, plain, a: np.ndarray, b: np.ndarray, depth_a=None, depth_b=None):
        a, b = _u64(a), _u64(b)
        B = a.shape[0]
        out = np.zeros_like(a)
        da = np.ascontiguousarray(depth_a, dtype=np.uint32) if depth_a is not None else None
        db = np.ascontiguousarray(depth_b, dtype=np.uint32) if depth_b is not None else None
        dout = np.zeros(B, dtype=np.uint32)
        check(self._lib.exacto_dbfv_mul(self._h, d, base, plain, a.ctypes.data, b.ctypes.data,
                                        out.ctypes.data, B, _ptr(da), _ptr(db), dout.ctypes.data))
        return out, dout

    def dbfv_square(self, d, base, plain, a: np.ndarray, depth_a=None):
        """a [B][d][2][L][n] -> (out, depth_out), bit for bit dbfv_mul(a, a, depth_a, depth_a)."""
        a = _u64(a)
        B = a.shape[0]
        out = np.zeros_like(a)
        da = np.ascontiguousarray(depth_a, dtype=np.uint32) if depth_a is not None else None
        dout = np.zeros(B, dtype=np.uint32)
        check(self._lib.exacto_dbfv_square(self._h, d, base, plain, a.ctypes.data, out.ctypes.data, B, _ptr(da),
                                           dout.ctypes.data))
        return out, dout

    def dbfv_mul_chain(self, d, base, plain, x: np.ndarray, y: np.ndarray, depth: int):
        """paper_repro.rs:203-236 chain: x * y^depth, mul_depth reset before every step."""
        x, y = _u64(x), _u64(y)
        out = np.zeros_like(x)
        check(self._lib.exacto_dbfv_mul_chain(self._h, d, base, plain, x.ctypes.data, y.ctypes.data,
                                              out.ctypes.data, x.shape[0], depth))
        return out

    def bfv_decrypt(self, ct: np.ndarray, sk: np.ndarray) -> np.ndarray:
        """encrypt.rs:111-178 batched: ct [B][polys][L][n], sk [L][n] (NTT) -> [B][n] mod p."""
        ct, sk = _u64(ct), _u64(sk)
        out = np.zeros((ct.shape[0], ct.shape[-1]), dtype=np.uint64)
        check(self._lib.exacto_bfv_decrypt(self._h, ct.ctypes.data, ct.shape[1], sk.ctypes.data,
                                           out.ctypes.data, ct.shape[0]))
        return out

    def dbfv_decrypt(self, d, base, plain, ct: np.ndarray, sk: np.ndarray) -> np.ndarray:
        """dbfv/decrypt.rs:20-43: ct [B][d][2][L][n] -> [B] scalars."""
        ct, sk = _u64(ct), _u64(sk)
        out = np.zeros(ct.shape[0], dtype=np.uint64)
        check(self._lib.exacto_dbfv_decrypt(self._h, d, base, plain, ct.ctypes.data, sk.ctypes.data,
                                            out.ctypes.data, ct.shape[0]))
        return out

    def dbfv_decrypt_poly(self, d, base, plain, ct: np.ndarray, sk: np.ndarray) -> np.ndarray:
        """dbfv/decrypt.rs:48-79: ct [B][d][2][L][n] -> [B][n] mod p."""
        ct, sk = _u64(ct), _u64(sk)
        out = np.zeros((ct.shape[0], ct.shape[-1]), dtype=np.uint64)
        check(self._lib.exacto_dbfv_decrypt_poly(self._h, d, base, plain, ct.ctypes.data, sk.ctypes.data,
                                                 out.ctypes.data, ct.shape[0]))
        return out

    def bfv_noise(self, ct: np.ndarray, sk: np.ndarray, expected=None, return_plain: bool = False):
        """paper_repro.rs:249-281 bfv_noise_inf, exact over the full Q, batched: ct [B][polys][L][n] -> B Python
        ints max |phase - Delta m| (centred mod Q); m is the decrypted coefficient, or expected [B][n] mod p.
        return_plain: also the decrypted plaintexts [B][n] (bfv_decrypt's), as (noise, plain)."""
        ct, sk = _u64(ct), _u64(sk)
        B = ct.shape[0]
        exp = _u64(expected).reshape(B, self.n) if expected is not None else None
        plain = np.zeros((B, self.n), dtype=np.uint64) if return_plain else None
        words = np.zeros((B, self.L), dtype=np.uint64)
        check(self._lib.exacto_bfv_noise(self._h, ct.ctypes.data, ct.shape[1], sk.ctypes.data, _ptr(exp), _ptr(plain),
                                         words.ctypes.data, B))
        noise = _words_to_ints(words)
        return (noise, plain) if return_plain else noise

    def dbfv_noise(self, d, ct: np.ndarray, sk: np.ndarray) -> list[int]:
        """paper_repro.rs:238-247 max_limb_noise batched: ct [B][d][2][L][n] -> B Python ints."""
        ct, sk = _u64(ct), _u64(sk)
        B = ct.shape[0]
        words = np.zeros((B, self.L), dtype=np.uint64)
        check(self._lib.exacto_dbfv_noise(self._h, d, ct.ctypes.data, sk.ctypes.data, words.ctypes.data, B))
        return _words_to_ints(words)

    # ---- dBFV beyond the product (dbfv/encrypt.rs, eval.rs:11-71, keyswitch.rs, advanced.rs)
    @staticmethod
    def _depths(depth, B):
        return np.ascontiguousarray(depth, dtype=np.uint32).reshape(B) if depth is not None else None

    def _dbfv_encrypt(self, name, d, base, plain, src, keypoly, key, stream, sigma):
        k, src, keypoly = self._key(key), _u64(src), _u64(keypoly)
        B = src.shape[0]
        ct = np.zeros((B, d, 2, self.L, self.n), dtype=np.uint64)
        check(getattr(self._lib, name)(self._h, d, base, plain, src.ctypes.data, keypoly.ctypes.data, sigma,
                                       k.ctypes.data, stream, ct.ctypes.data, B))
        return ct

    def dbfv_encrypt_sk(self, d, base, plain, values, sk, key, stream=0, sigma=3.2) -> np.ndarray:
        """dbfv/encrypt.rs:73-81: values [B] scalars -> [B][d][2][L][n]."""
        return self._dbfv_encrypt("exacto_dbfv_encrypt_sk", d, base, plain, _u64(values).reshape(-1), sk, key,
                                  stream, sigma)

    def dbfv_encrypt_pk(self, d, base, plain, values, pk, key, stream=0, sigma=3.2) -> np.ndarray:
        """dbfv/encrypt.rs:27-35."""
        return self._dbfv_encrypt("exacto_dbfv_encrypt_pk", d, base, plain, _u64(values).reshape(-1), pk, key,
                                  stream, sigma)

    def dbfv_encrypt_poly_sk(self, d, base, plain, pt, sk, key, stream=0, sigma=3.2) -> np.ndarray:
        """dbfv/encrypt.rs:94-103: pt [B][n] mod p -> [B][d][2][L][n]."""
        return self._dbfv_encrypt("exacto_dbfv_encrypt_poly_sk", d, base, plain, _u64(pt).reshape(-1, self.n), sk,
                                  key, stream, sigma)

    def dbfv_encrypt_poly_pk(self, d, base, plain, pt, pk, key, stream=0, sigma=3.2) -> np.ndarray:
        """dbfv/encrypt.rs:51-60."""
        return self._dbfv_encrypt("exacto_dbfv_encrypt_poly_pk", d, base, plain, _u64(pt).reshape(-1, self.n), pk,
                                  key, stream, sigma)

    def _dbfv_addsub(self, fn, a, b, depth_a, depth_b):
        a, b = _u64(a), _u64(b)
        B = a.shape[0]
        out = np.zeros((B, a.shape[1], max(a.shape[2], b.shape[2]), self.L, self.n), dtype=np.uint64)
        dout = np.zeros(B, dtype=np.uint32)
        da, db = self._depths(depth_a, B), self._depths(depth_b, B)
        check(fn(self._h, a.ctypes.data, a.shape[1], a.shape[2], b.ctypes.data, b.shape[1], b.shape[2],
                 out.ctypes.data, B, _ptr(da), _ptr(db), dout.ctypes.data))
        return out, dout

    def dbfv_add(self, a, b, depth_a=None, depth_b=None):
        """dbfv/eval.rs:11-33: a [B][d][p1][L][n] + b [B][d][p2][L][n] -> ([B][d][max][L][n], mul_depth [B])."""
        return self._dbfv_addsub(self._lib.exacto_dbfv_add, a, b, depth_a, depth_b)

    def dbfv_sub(self, a, b, depth_a=None, depth_b=None):
        """dbfv/eval.rs:36-58."""
        return self._dbfv_addsub(self._lib.exacto_dbfv_sub, a, b, depth_a, depth_b)

    def dbfv_neg(self, ct) -> np.ndarray:
        """dbfv/eval.rs:61-71."""
        ct = _u64(ct)
        out = np.zeros_like(ct)
        check(self._lib.exacto_dbfv_neg(self._h, ct.ctypes.data, ct.shape[1], ct.shape[2], out.ctypes.data,
                                        ct.shape[0]))
        return out

    def dbfv_relinearize(self, ct) -> np.ndarray:
        """dbfv/keyswitch.rs:9-23 with the resident key: [B][d][3][L][n] -> [B][d][2][L][n]."""
        ct = _u64(ct)
        B, d, polys = ct.shape[:3]
        out = np.zeros((B, d, polys if polys < 3 else 2, self.L, self.n), dtype=np.uint64)
        check(self._lib.exacto_dbfv_relinearize(self._h, ct.ctypes.data, d, polys, out.ctypes.data, B))
        return out

    def dbfv_apply_automorphism(self, ct, element, gk) -> np.ndarray:
        """dbfv/advanced.rs:15-29: ct [B][d][2][L][n], gk [K][2][L][n]."""
        ct, gk = _u64(ct), _u64(gk)
        out = np.zeros_like(ct)
        check(self._lib.exacto_dbfv_apply_automorphism(self._h, ct.ctypes.data, ct.shape[1], ct.shape[2], element,
                                                       gk.ctypes.data if gk.size else None, gk.shape[0],
                                                       out.ctypes.data, ct.shape[0]))
        return out

    def dbfv_linear_map(self, matrix, ct) -> np.ndarray:
        """out[b][j] = sum_i ((matrix[j][i] mod t) mod q_l) in[b][i]: ct [B][d_in][polys][L][n], matrix
        [d_out][d_in] -> [B][d_out][polys][L][n] (exacto_dbfv_linear_map)."""
        ct = _u64(ct)
        m = np.ascontiguousarray(np.array([[int(x) for x in row] for row in matrix], dtype=np.uint64))
        d_out, d_in = m.shape
        if d_in != ct.shape[1]:
            raise ValueError(f"matrix has {d_in} columns, ciphertext {ct.shape[1]} limbs")
        out = np.zeros((ct.shape[0], d_out) + ct.shape[2:], dtype=np.uint64)
        check(self._lib.exacto_dbfv_linear_map(self._h, d_in, d_out, ct.shape[2], m.ctypes.data, ct.ctypes.data,
                                               out.ctypes.data, ct.shape[0]))
        return out

    def dbfv_change_base(self, d, base, plain, new_base, new_d, ct) -> np.ndarray:
        """dbfv/advanced.rs:99-160: ct [B][d][2][L][n] -> [B][new_d][2][L][n]."""
        ct = _u64(ct)
        out = np.zeros((ct.shape[0], max(new_d, 1), 2, self.L, self.n), dtype=np.uint64)
        check(self._lib.exacto_dbfv_change_base(self._h, d, base, plain, new_base, new_d, ct.ctypes.data,
                                                out.ctypes.data, ct.shape[0]))
        return out[:, :new_d]

    def dbfv_div_by_base(self, d, base, plain, ct):
        """dbfv/advanced.rs:36-93: (ct' [B][d][2][L][n], new plain modulus p / base)."""
        ct = _u64(ct)
        out = np.zeros_like(ct)
        new_plain = C.c_uint64(0)
        check(self._lib.exacto_dbfv_div_by_base(self._h, d, base, plain, ct.ctypes.data, out.ctypes.data,
                                                ct.shape[0], C.byref(new_plain)))
        return out, int(new_plain.value)

    # ---- key generation / encryption (keygen.rs:64-162, encrypt.rs:29-106); key = 4 u64 words
    @staticmethod
    def _key(key):
        k = _u64(key).reshape(-1)
        if k.size != 4:
            raise ValueError("key must be 4 64-bit words")
        return k

    def gen_secret_key(self, key, stream=0) -> np.ndarray:
        k = self._key(key)
        sk = np.zeros((self.L, self.n), dtype=np.uint64)
        check(self._lib.exacto_gen_secret_key(self._h, k.ctypes.data, stream, sk.ctypes.data))
        return sk

    def gen_public_key(self, sk, key, stream=0, sigma=3.2) -> np.ndarray:
        k, sk = self._key(key), _u64(sk)
        pk = np.zeros((2, self.L, self.n), dtype=np.uint64)
        check(self._lib.exacto_gen_public_key(self._h, sk.ctypes.data, sigma, k.ctypes.data, stream, pk.ctypes.data))
        return pk

    def gen_relin_key(self, sk, key, stream=0, sigma=3.2, num_keys=None, resident=False):
        """resident=True: generate into the context's resident key (returns None)."""
        k, sk = self._key(key), _u64(sk)
        nk = self.G if num_keys is None else num_keys
        if resident:
            check(self._lib.exacto_gen_relin_key(self._h, sk.ctypes.data, sigma, k.ctypes.data, stream, nk, None))
            return None
        rlk = np.zeros((nk, 2, self.L, self.n), dtype=np.uint64)
        check(self._lib.exacto_gen_relin_key(self._h, sk.ctypes.data, sigma, k.ctypes.data, stream, nk,
                                             rlk.ctypes.data))
        return rlk

    def encrypt_sk(self, pt, sk, key, stream=0, sigma=3.2) -> np.ndarray:
        """pt [B][n] plaintext coefficients -> ct [B][2][L][n]."""
        k, pt, sk = self._key(key), _u64(pt), _u64(sk)
        ct = np.zeros((pt.shape[0], 2, self.L, self.n), dtype=np.uint64)
        check(self._lib.exacto_encrypt_sk(self._h, pt.ctypes.data, sk.ctypes.data, sigma, k.ctypes.data, stream,
                                          ct.ctypes.data, pt.shape[0]))
        return ct

    def encrypt_pk(self, pt, pk, key, stream=0, sigma=3.2) -> np.ndarray:
        k, pt, pk = self._key(key), _u64(pt), _u64(pk)
        ct = np.zeros((pt.shape[0], 2, self.L, self.n), dtype=np.uint64)
        check(self._lib.exacto_encrypt_pk(self._h, pt.ctypes.data, pk.ctypes.data, sigma, k.ctypes.data, stream,
                                          ct.ctypes.data, pt.shape[0]))
        return ct

    def gen_galois_key(self, sk, element, key, stream=0, sigma=3.2, num_keys=None) -> np.ndarray:
        """keygen.rs:171-209 -> [num_keys][2][L][n]."""
        k, sk = self._key(key), _u64(sk)
        nk = self.G if num_keys is None else num_keys
        gk = np.zeros((nk, 2, self.L, self.n), dtype=np.uint64)
        check(self._lib.exacto_gen_galois_key(self._h, sk.ctypes.data, element, sigma, k.ctypes.data, stream, nk,
                                              gk.ctypes.data))
        return gk

    def bfv_apply_automorphism(self, ct, element, gk) -> np.ndarray:
        """eval.rs:512-561 batched: ct [B][2][L][n], gk [K][2][L][n] -> [B][2][L][n]."""
        ct, gk = _u64(ct), _u64(gk)
        out = np.zeros((ct.shape[0], 2, self.L, self.n), dtype=np.uint64)
        check(self._lib.exacto_bfv_apply_automorphism(self._h, ct.ctypes.data, ct.shape[1], element,
                                                      gk.ctypes.data if gk.size else None, gk.shape[0],
                                                      out.ctypes.data, ct.shape[0]))
        return out

    def required_trace_elements(self, n=None) -> list[int]:
        return required_trace_elements(self.n if n is None else n)

    # ---- SIMD batching (exacto_batch_*): slot vectors [B][n] as 2 x n/2 matrices, exacto_hip.h
    def batch_info(self) -> int:
        """zeta of the slot encoding; raises the context's batching error when it cannot batch."""
        root = C.c_uint64(0)
        check(self._lib.exacto_batch_info(self._h, C.byref(root)))
        return int(root.value)

    def _batch_rows(self, a, what):
        a = _u64(a)
        if a.ndim != 2 or a.shape[1] != self.n:
            raise ValueError(f"{what} must be a [B][{self.n}] array")
        return a

    def batch_encode(self, values) -> np.ndarray:
        """values [B][n] (each below t, else InvalidParam) -> plaintext coefficients [B][n]."""
        v = self._batch_rows(values, "values")
        pt = np.zeros_like(v)
        check(self._lib.exacto_batch_encode(self._h, v.ctypes.data, pt.ctypes.data, v.shape[0]))
        return pt

    def batch_decode(self, pt) -> np.ndarray:
        """plaintext coefficients [B][n] (reduced mod t) -> values [B][n]."""
        p = self._batch_rows(pt, "pt")
        v = np.zeros_like(p)
        check(self._lib.exacto_batch_decode(self._h, p.ctypes.data, v.ctypes.data, p.shape[0]))
        return v

    def rotate_rows(self, ct, steps, gk=None) -> np.ndarray:
        """Both slot rows left by `steps`: bfv_apply_automorphism with 3^steps mod 2n and its key gk
        (None allowed when steps == 0 mod n/2)."""
        ct = _u64(ct)
        gk = None if gk is None else _u64(gk)
        out = np.zeros((ct.shape[0], ct.shape[1], self.L, self.n), dtype=np.uint64)
        check(self._lib.exacto_bfv_rotate_rows(self._h, ct.ctypes.data, ct.shape[1], int(steps),
                                               gk.ctypes.data if gk is not None and gk.size else None,
                                               0 if gk is None else gk.shape[0], out.ctypes.data, ct.shape[0]))
        return out

    def swap_rows(self, ct, gk) -> np.ndarray:
        """The two slot rows exchanged: bfv_apply_automorphism with 2n - 1 and its key gk."""
        ct, gk = _u64(ct), _u64(gk)
        out = np.zeros((ct.shape[0], ct.shape[1], self.L, self.n), dtype=np.uint64)
        check(self._lib.exacto_bfv_swap_rows(self._h, ct.ctypes.data, ct.shape[1], gk.ctypes.data if gk.size else None,
                                             gk.shape[0], out.ctypes.data, ct.shape[0]))
        return out

    # ---- hoisted rotations and slot linear transforms (exacto_galois_keyset_*, exacto_hip.h)
    def galois_keyset(self, elements, gks) -> "GaloisKeySet":
        """elements [R], gks [R][num_keys][2][L][n] (host) -> a prepared key set; element 1 needs no key."""
        return GaloisKeySet(self, elements, gks)

    def galois_keyset_dev(self, elements, gks, num_keys) -> "GaloisKeySet":
        """The same from device memory gks [R][num_keys][2][L][n] (may be released afterwards)."""
        return GaloisKeySet(self, elements, gks, num_keys, dev=True)

    def bfv_rotate_hoisted(self, ct, keyset: "GaloisKeySet") -> np.ndarray:
        """ct [B][2][L][n] -> [B][R][2][L][n]: every automorphism of the set on the shared digits of c1 (the
        same plaintexts as bfv_apply_automorphism, not its bits)."""
        ct = _u64(ct)
        out = np.zeros((ct.shape[0], keyset.R, 2, self.L, self.n), dtype=np.uint64)
        check(self._lib.exacto_bfv_rotate_hoisted(self._h, keyset.handle, ct.ctypes.data if ct.size else None,
                                                  out.ctypes.data if out.size else None, ct.shape[0]))
        return out

    def bfv_linear_transform(self, ct, keyset: "GaloisKeySet", pts) -> np.ndarray:
        """ct [B][2][L][n], pts [R][n] plaintext coefficients -> sum_r pts[r] * rotation r, [B][2][L][n]."""
        ct, pts = _u64(ct), _u64(pts)
        if pts.shape != (keyset.R, self.n):
            raise ValueError(f"pts must be a [{keyset.R}][{self.n}] array")
        out = np.zeros((ct.shape[0], 2, self.L, self.n), dtype=np.uint64)
        check(self._lib.exacto_bfv_linear_transform(self._h, keyset.handle, ct.ctypes.data if ct.size else None,
                                                    pts.ctypes.data, out.ctypes.data if out.size else None,
                                                    ct.shape[0]))
        return out

    def bfv_rotate_hoisted_dev(self, ct, keyset: "GaloisKeySet", out, batch):
        check(self._lib.exacto_bfv_rotate_hoisted_dev(self._h, keyset.handle, self._p(ct), self._p(out), batch))

    def bfv_linear_transform_dev(self, ct, keyset: "GaloisKeySet", pts, out, batch):
        check(self._lib.exacto_bfv_linear_transform_dev(self._h, keyset.handle, self._p(ct), self._p(pts),
                                                        self._p(out), batch))

    def rotate_rows_keyset(self, steps, gks) -> "GaloisKeySet":
        """A key set for row rotations by `steps` (gks[r] the key of 3^steps[r] mod 2n; ignored for steps == 0
        mod n/2), for rotate_rows_many / batch_linear_transform."""
        return self.galois_keyset([galois_element_rotate_rows(self.n, int(s)) for s in steps], gks)

    def rotate_rows_many(self, ct, steps, keyset: "GaloisKeySet") -> np.ndarray:
        """Both slot rows left by every steps[r] at once: ct [B][2][L][n] -> [B][R][2][L][n]; keyset holds the
        elements 3^steps[r] mod 2n in this order (rotate_rows_keyset)."""
        want = [galois_element_rotate_rows(self.n, int(s)) for s in steps]
        if [e % (2 * self.n) for e in keyset.elements] != want:
            raise ValueError("keyset does not hold the elements of these steps in this order")
        return self.bfv_rotate_hoisted(ct, keyset)

    def batch_linear_transform(self, ct, keyset: "GaloisKeySet", slot_diagonals) -> np.ndarray:
        """sum_r w_r (.) rot_r(x) on slots: slot_diagonals [R][n] (values below t) are batch_encoded and
        multiplied into the set's rotations of ct [B][2][L][n]."""
        return self.bfv_linear_transform(ct, keyset, self.batch_encode(slot_diagonals))

    def batch_encrypt_sk(self, values, sk, key, stream=0, sigma=3.2) -> np.ndarray:
        """batch_encode then encrypt_sk on the device: values [B][n] -> ct [B][2][L][n]."""
        k, v, sk = self._key(key), self._batch_rows(values, "values"), _u64(sk)
        ct = np.zeros((v.shape[0], 2, self.L, self.n), dtype=np.uint64)
        check(self._lib.exacto_batch_encrypt_sk(self._h, v.ctypes.data, sk.ctypes.data, sigma, k.ctypes.data, stream,
                                                ct.ctypes.data, v.shape[0]))
        return ct

    def batch_encrypt_pk(self, values, pk, key, stream=0, sigma=3.2) -> np.ndarray:
        k, v, pk = self._key(key), self._batch_rows(values, "values"), _u64(pk)
        ct = np.zeros((v.shape[0], 2, self.L, self.n), dtype=np.uint64)
        check(self._lib.exacto_batch_encrypt_pk(self._h, v.ctypes.data, pk.ctypes.data, sigma, k.ctypes.data, stream,
                                                ct.ctypes.data, v.shape[0]))
        return ct

    def batch_decrypt(self, ct, sk) -> np.ndarray:
        """bfv_decrypt then batch_decode on the device: ct [B][polys][L][n] -> values [B][n]."""
        ct, sk = _u64(ct), _u64(sk)
        out = np.zeros((ct.shape[0], self.n), dtype=np.uint64)
        check(self._lib.exacto_batch_decrypt(self._h, ct.ctypes.data, ct.shape[1], sk.ctypes.data, out.ctypes.data,
                                             ct.shape[0]))
        return out

    def batch_encode_dev(self, values, pt, batch):
        """Device form: every value is reduced mod t (no range error); pt may be values (in place)."""
        check(self._lib.exacto_batch_encode_dev(self._h, self._p(values), self._p(pt), batch))

    def batch_decode_dev(self, pt, values, batch):
        check(self._lib.exacto_batch_decode_dev(self._h, self._p(pt), self._p(values), batch))

    def rotate_rows_dev(self, ct, steps, gk, num_keys, out, batch):
        check(self._lib.exacto_bfv_rotate_rows_dev(self._h, self._p(ct), 2, int(steps), self._p(gk), num_keys,
                                                   self._p(out), batch))

    def swap_rows_dev(self, ct, gk, num_keys, out, batch):
        check(self._lib.exacto_bfv_swap_rows_dev(self._h, self._p(ct), 2, self._p(gk), num_keys, self._p(out), batch))

    def batch_encrypt_sk_dev(self, values, sk, key, stream, ct, batch, sigma=3.2):
        k = self._key(key)
        check(self._lib.exacto_batch_encrypt_sk_dev(self._h, self._p(values), self._p(sk), sigma, k.ctypes.data, stream,
                                                    self._p(ct), batch))

    def batch_encrypt_pk_dev(self, values, pk, key, stream, ct, batch, sigma=3.2):
        k = self._key(key)
        check(self._lib.exacto_batch_encrypt_pk_dev(self._h, self._p(values), self._p(pk), sigma, k.ctypes.data, stream,
                                                    self._p(ct), batch))

    def batch_decrypt_dev(self, ct, polys, sk, values, batch):
        check(self._lib.exacto_batch_decrypt_dev(self._h, self._p(ct), polys, self._p(sk), self._p(values), batch))

    # ---- slot-packed dBFV (exacto_dbfv_batch_*): n integers mod p per dBFV ciphertext, exacto_hip.h
    def dbfv_batch_encode(self, d, base, plain, values) -> np.ndarray:
        """values [B][n] (reduced mod p; as they are for p = 0) -> pt [B][d][n], row k the slot encoding of the
        k-th base-b digits."""
        v = self._batch_rows(values, "values")
        pt = np.zeros((v.shape[0], d, self.n), dtype=np.uint64)
        check(self._lib.exacto_dbfv_batch_encode(self._h, d, base, plain, v.ctypes.data, pt.ctypes.data, v.shape[0]))
        return pt

    def dbfv_batch_decode(self, d, base, plain, pt) -> np.ndarray:
        """pt [B][d][n] (reduced mod t) -> values [B][n]: slot decode, centre at t/2, recompose mod p."""
        p = _u64(pt)
        if p.ndim != 3 or p.shape[1:] != (d, self.n):
            raise ValueError(f"pt must be a [B][{d}][{self.n}] array")
        v = np.zeros((p.shape[0], self.n), dtype=np.uint64)
        check(self._lib.exacto_dbfv_batch_decode(self._h, d, base, plain, p.ctypes.data, v.ctypes.data, p.shape[0]))
        return v

    def _dbfv_batch_encrypt(self, name, d, base, plain, values, keypoly, key, stream, sigma):
        k, v, keypoly = self._key(key), self._batch_rows(values, "values"), _u64(keypoly)
        ct = np.zeros((v.shape[0], d, 2, self.L, self.n), dtype=np.uint64)
        check(getattr(self._lib, name)(self._h, d, base, plain, v.ctypes.data, keypoly.ctypes.data, sigma,
                                       k.ctypes.data, stream, ct.ctypes.data, v.shape[0]))
        return ct

    def dbfv_batch_encrypt_sk(self, d, base, plain, values, sk, key, stream=0, sigma=3.2) -> np.ndarray:
        """dbfv_batch_encode then encrypt_sk of the B * d plaintexts on the device: values [B][n] ->
        ct [B][d][2][L][n]."""
        return self._dbfv_batch_encrypt("exacto_dbfv_batch_encrypt_sk", d, base, plain, values, sk, key, stream, sigma)

    def dbfv_batch_encrypt_pk(self, d, base, plain, values, pk, key, stream=0, sigma=3.2) -> np.ndarray:
        return self._dbfv_batch_encrypt("exacto_dbfv_batch_encrypt_pk", d, base, plain, values, pk, key, stream, sigma)

    def dbfv_batch_decrypt(self, d, base, plain, ct, sk) -> np.ndarray:
        """bfv_decrypt of the B * d limbs then dbfv_batch_decode on the device: ct [B][d][2][L][n] -> [B][n]."""
        ct, sk = _u64(ct), _u64(sk)
        out = np.zeros((ct.shape[0], self.n), dtype=np.uint64)
        check(self._lib.exacto_dbfv_batch_decrypt(self._h, d, base, plain, ct.ctypes.data, sk.ctypes.data,
                                                  out.ctypes.data, ct.shape[0]))
        return out

    # ---- dBFV plaintext products (exacto_dbfv_plain_*): public wide operands times dBFV ciphertexts, exacto_hip.h
    def set_plain_terms(self, terms: int):
        """Terms of a dBFV plaintext product lifted at a time (0: the default); no result depends on it."""
        check(self._lib.exacto_ctx_set_plain_terms(self._h, terms))

    def dbfv_plain_limits(self) -> tuple[int, int]:
        """(products one accumulator of the product kernel takes between two reductions, term chunk)."""
        f, t = _SZ(0), _SZ(0)
        check(self._lib.exacto_dbfv_plain_limits(self._h, C.byref(f), C.byref(t)))
        return int(f.value), int(t.value)

    def dbfv_plain_mul_sum(self, d, base, plain, cts, pts, depth_ct=None):
        """cts [B][K][d][polys][L][n], pts [B or 1][K][d][n] -> (out [B][d][polys][L][n], mul_depth [B]):
        reduce(sum_k pts[k] * cts[k]) over the digit vectors."""
        cts, pts = _u64(cts), _u64(pts)
        if cts.ndim != 6 or pts.ndim != 4:
            raise ValueError("cts must be [B][K][d][polys][L][n] and pts [B or 1][K][d][n]")
        B, K, polys = cts.shape[0], cts.shape[1], cts.shape[3]
        out = np.zeros((B, d) + cts.shape[3:], dtype=np.uint64)
        dc = np.ascontiguousarray(depth_ct, dtype=np.uint32).reshape(B, K) if depth_ct is not None else None
        dout = np.zeros(B, dtype=np.uint32)
        check(self._lib.exacto_dbfv_plain_mul_sum(self._h, d, base, plain, cts.ctypes.data, K, polys, pts.ctypes.data,
                                                  pts.shape[0], out.ctypes.data, B, _ptr(dc), dout.ctypes.data))
        return out, dout

    def dbfv_plain_mul(self, d, base, plain, ct, pt, depth_ct=None):
        """ct [B][d][polys][L][n], pt [B or 1][d][n] -> (out, mul_depth [B]): dbfv_plain_mul_sum with K = 1."""
        ct, pt = _u64(ct), _u64(pt)
        if ct.ndim != 5 or pt.ndim != 3:
            raise ValueError("ct must be [B][d][polys][L][n] and pt [B or 1][d][n]")
        B = ct.shape[0]
        out = np.zeros_like(ct)
        dc = self._depths(depth_ct, B)
        dout = np.zeros(B, dtype=np.uint32)
        check(self._lib.exacto_dbfv_plain_mul(self._h, d, base, plain, ct.ctypes.data, ct.shape[2], pt.ctypes.data,
                                              pt.shape[0], out.ctypes.data, B, _ptr(dc), dout.ctypes.data))
        return out, dout

    def _dbfv_plain_addsub(self, fn, ct, pt):
        ct, pt = _u64(ct), _u64(pt)
        if ct.ndim != 5 or pt.ndim != 3:
            raise ValueError("ct must be [B][d][polys][L][n] and pt [B or 1][d][n]")
        out = np.zeros_like(ct)
        check(fn(self._h, ct.shape[1], ct.ctypes.data, ct.shape[2], pt.ctypes.data, pt.shape[0], out.ctypes.data,
                 ct.shape[0]))
        return out

    def dbfv_plain_add(self, ct, pt) -> np.ndarray:
        """ct [B][d][polys][L][n] + pt [B or 1][d][n]: bfv_plain_add limb by limb (c0 + Delta m)."""
        return self._dbfv_plain_addsub(self._lib.exacto_dbfv_plain_add, ct, pt)

    def dbfv_plain_sub(self, ct, pt) -> np.ndarray:
        """ct - pt limb by limb (c0 - Delta m)."""
        return self._dbfv_plain_addsub(self._lib.exacto_dbfv_plain_sub, ct, pt)

    def dbfv_batch_plain_mul(self, d, base, plain, ct, values, depth_ct=None):
        """Slot-wise ct * values mod p: values [B or 1][n] slot-encoded on the device (dbfv_batch_encode), then
        dbfv_plain_mul.  Returns (out, mul_depth [B])."""
        return self.dbfv_plain_mul(d, base, plain, ct, self.dbfv_batch_encode(d, base, plain, values), depth_ct)

    def dbfv_batch_plain_dot(self, d, base, plain, cts, values, depth_ct=None):
        """Slot-wise sum_k cts[k] * values[k] mod p: cts [B][K][d][polys][L][n], values [B or 1][K][n]."""
        v = _u64(values)
        if v.ndim != 3 or v.shape[2] != self.n:
            raise ValueError(f"values must be a [B or 1][K][{self.n}] array")
        pts = self.dbfv_batch_encode(d, base, plain, v.reshape(-1, self.n)).reshape(v.shape[0], v.shape[1], d, self.n)
        return self.dbfv_plain_mul_sum(d, base, plain, cts, pts, depth_ct)

    def dbfv_batch_plain_add(self, d, base, plain, ct, values) -> np.ndarray:
        """Slot-wise ct + values mod p (values [B or 1][n])."""
        return self.dbfv_plain_add(ct, self.dbfv_batch_encode(d, base, plain, values))

    def dbfv_batch_plain_sub(self, d, base, plain, ct, values) -> np.ndarray:
        """Slot-wise ct - values mod p (values [B or 1][n])."""
        return self.dbfv_plain_sub(ct, self.dbfv_batch_encode(d, base, plain, values))

    def dbfv_plain_mul_sum_dev(self, d, base, plain, cts, K, polys, pts, pt_batch, out, batch, depth_ct=None):
        dc = np.ascontiguousarray(depth_ct, dtype=np.uint32) if depth_ct is not None else None    # [batch][K]
        check(self._lib.exacto_dbfv_plain_mul_sum_dev(self._h, d, base, plain, self._p(cts), K, polys, self._p(pts),
                                                      pt_batch, self._p(out), batch, _ptr(dc), None))

    def dbfv_plain_mul_dev(self, d, base, plain, ct, polys, pt, pt_batch, out, batch, depth_ct=None):
        dc = self._depths(depth_ct, batch)
        check(self._lib.exacto_dbfv_plain_mul_dev(self._h, d, base, plain, self._p(ct), polys, self._p(pt), pt_batch,
                                                  self._p(out), batch, _ptr(dc), None))

    def dbfv_plain_add_dev(self, d, ct, polys, pt, pt_batch, out, batch):
        check(self._lib.exacto_dbfv_plain_add_dev(self._h, d, self._p(ct), polys, self._p(pt), pt_batch, self._p(out),
                                                  batch))

    def dbfv_plain_sub_dev(self, d, ct, polys, pt, pt_batch, out, batch):
        check(self._lib.exacto_dbfv_plain_sub_dev(self._h, d, self._p(ct), polys, self._p(pt), pt_batch, self._p(out),
                                                  batch))

    def dbfv_batch_plain_mul_dev(self, d, base, plain, ct, polys, values, pt_batch, pt, out, batch):
        """values [pt_batch][n] -> pt [pt_batch][d][n] (dbfv_batch_encode_dev), then dbfv_plain_mul_dev into out."""
        self.dbfv_batch_encode_dev(d, base, plain, values, pt, pt_batch)
        self.dbfv_plain_mul_dev(d, base, plain, ct, polys, pt, pt_batch, out, batch)

    def dbfv_batch_plain_dot_dev(self, d, base, plain, cts, K, polys, values, pt_batch, pts, out, batch):
        """values [pt_batch][K][n] -> pts [pt_batch][K][d][n], then dbfv_plain_mul_sum_dev into out."""
        self.dbfv_batch_encode_dev(d, base, plain, values, pts, pt_batch * K)
        self.dbfv_plain_mul_sum_dev(d, base, plain, cts, K, polys, pts, pt_batch, out, batch)

    def dbfv_batch_plain_add_dev(self, d, base, plain, ct, polys, values, pt_batch, pt, out, batch, sub=False):
        self.dbfv_batch_encode_dev(d, base, plain, values, pt, pt_batch)
        (self.dbfv_plain_sub_dev if sub else self.dbfv_plain_add_dev)(d, ct, polys, pt, pt_batch, out, batch)

    def dbfv_batch_plain_sub_dev(self, d, base, plain, ct, polys, values, pt_batch, pt, out, batch):
        self.dbfv_batch_plain_add_dev(d, base, plain, ct, polys, values, pt_batch, pt, out, batch, sub=True)

    def dbfv_batch_encode_dev(self, d, base, plain, values, pt, batch):
        check(self._lib.exacto_dbfv_batch_encode_dev(self._h, d, base, plain, self._p(values), self._p(pt), batch))

    def dbfv_batch_decode_dev(self, d, base, plain, pt, values, batch):
        check(self._lib.exacto_dbfv_batch_decode_dev(self._h, d, base, plain, self._p(pt), self._p(values), batch))

    def dbfv_batch_encrypt_sk_dev(self, d, base, plain, values, sk, key, stream, ct, batch, sigma=3.2):
        k = self._key(key)
        check(self._lib.exacto_dbfv_batch_encrypt_sk_dev(self._h, d, base, plain, self._p(values), self._p(sk), sigma,
                                                         k.ctypes.data, stream, self._p(ct), batch))

    def dbfv_batch_encrypt_pk_dev(self, d, base, plain, values, pk, key, stream, ct, batch, sigma=3.2):
        k = self._key(key)
        check(self._lib.exacto_dbfv_batch_encrypt_pk_dev(self._h, d, base, plain, self._p(values), self._p(pk), sigma,
                                                         k.ctypes.data, stream, self._p(ct), batch))

    def dbfv_batch_decrypt_dev(self, d, base, plain, ct, sk, values, batch):
        check(self._lib.exacto_dbfv_batch_decrypt_dev(self._h, d, base, plain, self._p(ct), self._p(sk),
                                                      self._p(values), batch))

    def dbfv_rotate_rows(self, ct, steps, gk) -> np.ndarray:
        """Both rows of the wide slots left by `steps`: dbfv_apply_automorphism with 3^steps mod 2n and its key."""
        return self.dbfv_apply_automorphism(ct, galois_element_rotate_rows(self.n, int(steps)), gk)

    def dbfv_swap_rows(self, ct, gk) -> np.ndarray:
        """The two rows of the wide slots exchanged: dbfv_apply_automorphism with 2n - 1 and its key."""
        return self.dbfv_apply_automorphism(ct, galois_element_swap_rows(self.n), gk)

    # ---- dBFV hoisted rotations and slot linear transforms with wide diagonals (exacto_dbfv_linear_transform*)
    def dbfv_rotate_hoisted(self, ct, keyset: "GaloisKeySet") -> np.ndarray:
        """ct [B][d][2][L][n] -> [B][R][d][2][L][n]: limb j of out[b][r] is bfv_rotate_hoisted's [b*d + j][r]."""
        ct = _u64(ct)
        if ct.ndim != 5:
            raise ValueError("ct must be [B][d][2][L][n]")
        B, d = ct.shape[:2]
        out = np.zeros((B, keyset.R, d, 2, self.L, self.n), dtype=np.uint64)
        check(self._lib.exacto_dbfv_rotate_hoisted(self._h, keyset.handle, d, ct.ctypes.data if ct.size else None,
                                                   out.ctypes.data if out.size else None, B))
        return out

    def dbfv_rotate_hoisted_dev(self, d, ct, keyset: "GaloisKeySet", out, batch):
        check(self._lib.exacto_dbfv_rotate_hoisted_dev(self._h, keyset.handle, d, self._p(ct), self._p(out), batch))

    def dbfv_rotate_rows_many(self, ct, steps, keyset: "GaloisKeySet") -> np.ndarray:
        """Both rows of the wide slots left by every steps[r] at once: ct [B][d][2][L][n] -> [B][R][d][2][L][n];
        keyset holds the elements 3^steps[r] mod 2n in this order (rotate_rows_keyset)."""
        want = [galois_element_rotate_rows(self.n, int(s)) for s in steps]
        if [e % (2 * self.n) for e in keyset.elements] != want:
            raise ValueError("keyset does not hold the elements of these steps in this order")
        return self.dbfv_rotate_hoisted(ct, keyset)

    def set_dbfv_lt_fused(self, on: bool):
        """True: dBFV linear transforms on the limb-wise key switch with d <= 8 take the fused kernel instead of
        the staged route, the default (tests and measurements); no result depends on it."""
        check(self._lib.exacto_ctx_set_dbfv_lt_fused(self._h, 1 if on else 0))

    def dbfv_diagonals(self, d, pts) -> "DbfvDiagonals":
        """pts [R][d][n] plaintext coefficients (host) -> diagonals lifted once for dbfv_linear_transform."""
        return DbfvDiagonals(self, d, pts)

    def dbfv_diagonals_dev(self, d, pts, R) -> "DbfvDiagonals":
        """The same from device memory pts [R][d][n] (may be released afterwards)."""
        return DbfvDiagonals(self, d, pts, R, dev=True)

    def dbfv_linear_transform(self, d, base, plain, ct, keyset: "GaloisKeySet", pts, depth_ct=None):
        """ct [B][d][2][L][n]; pts [R][d][n] plaintext coefficients or a DbfvDiagonals -> (out [B][d][2][L][n],
        mul_depth [B]): reduce(sum_r pts[r] * rotation r), dbfv_plain_mul_sum over the hoisted rotations."""
        ct = _u64(ct)
        if ct.ndim != 5 or ct.shape[1] != d:
            raise ValueError(f"ct must be [B][{d}][2][L][n]")
        B = ct.shape[0]
        out = np.zeros_like(ct)
        dc = self._depths(depth_ct, B)
        dout = np.zeros(B, dtype=np.uint32)
        if isinstance(pts, DbfvDiagonals):
            fn, pp = self._lib.exacto_dbfv_linear_transform_prepared, pts.handle
        else:
            pts = _u64(pts)
            if pts.shape != (keyset.R, d, self.n):
                raise ValueError(f"pts must be a [{keyset.R}][{d}][{self.n}] array")
            fn, pp = self._lib.exacto_dbfv_linear_transform, pts.ctypes.data
        check(fn(self._h, keyset.handle, d, base, plain, ct.ctypes.data, pp, out.ctypes.data, B, _ptr(dc),
                 dout.ctypes.data))
        return out, dout

    def dbfv_linear_transform_dev(self, d, base, plain, ct, keyset: "GaloisKeySet", pts, out, batch, depth_ct=None):
        """pts: a device buffer [R][d][n] or a DbfvDiagonals."""
        dc = self._depths(depth_ct, batch)
        if isinstance(pts, DbfvDiagonals):
            fn, pp = self._lib.exacto_dbfv_linear_transform_prepared_dev, pts.handle
        else:
            fn, pp = self._lib.exacto_dbfv_linear_transform_dev, self._p(pts)
        check(fn(self._h, keyset.handle, d, base, plain, self._p(ct), pp, self._p(out), batch, _ptr(dc), None))

    def dbfv_batch_linear_transform(self, d, base, plain, ct, keyset: "GaloisKeySet", wide_diagonals, depth_ct=None):
        """Slot-wise sum_r W_r[s] * x[rot_r(s)] mod p: wide_diagonals [R][n] slot-encoded on the device
        (dbfv_batch_encode), then dbfv_linear_transform.  Returns (out, mul_depth [B])."""
        pts = self.dbfv_batch_encode(d, base, plain, wide_diagonals)
        return self.dbfv_linear_transform(d, base, plain, ct, keyset, pts, depth_ct)

    def gen_trace_galois_keys(self, sk, key, stream=0, elements=None, sigma=3.2):
        """gen_trace_galois_keys / gen_all_galois_keys (coeffs_to_slots.rs:151-197): one key per element,
        element e on ChaCha stream `stream + e`.  Returns (elements, gks [E][G][2][L][n])."""
        els = self.required_trace_elements() if elements is None else list(elements)
        gks = np.stack([self.gen_galois_key(sk, k, key, stream=stream + e, sigma=sigma) for e, k in enumerate(els)])
        return els, gks

    def extract_coefficients(self, ct, j0, count, elements, gks) -> np.ndarray:
        """coeffs_to_slots.rs:21-49 for j0 .. j0+count-1: ct [2][L][n] -> [count][2][L][n]."""
        ct = _u64(ct)
        el = np.ascontiguousarray(np.asarray(elements, dtype=np.uint64))
        gks = _u64(gks)
        E = el.shape[0]
        out = np.zeros((count, 2, self.L, self.n), dtype=np.uint64)
        check(self._lib.exacto_extract_coefficients(self._h, ct.ctypes.data, j0, count, el.ctypes.data if E else None,
                                                    E, gks.ctypes.data if E else None, gks.shape[1] if E else 0,
                                                    out.ctypes.data))
        return out

    def extract_coefficient(self, ct, j, elements, gks) -> np.ndarray:
        return self.extract_coefficients(ct, j, 1, elements, gks)[0]

    def coeffs_to_slots(self, ct, elements, gks) -> np.ndarray:
        """coeffs_to_slots.rs:103-115: all n coefficients, the n shifted copies traced together."""
        return self.extract_coefficients(ct, 0, self.n, elements, gks)

    def slots_to_coeffs(self, slots) -> np.ndarray:
        """coeffs_to_slots.rs:121-145: slots [S][polys][L][n] -> [polys][L][n]."""
        slots = _u64(slots)
        S = slots.shape[0]
        polys = slots.shape[1] if S else 2
        out = np.zeros((polys, self.L, self.n), dtype=np.uint64)
        check(self._lib.exacto_slots_to_coeffs(self._h, slots.ctypes.data, S, polys, out.ctypes.data))
        return out

    def trivial_encrypt_poly(self, pt) -> np.ndarray:
        """digit_extract.rs:179-189 batched: pt [B][n] -> (Delta m, 0) [B][2][L][n]."""
        pt = _u64(pt)
        pt = pt.reshape(-1, self.n)
        out = np.zeros((pt.shape[0], 2, self.L, self.n), dtype=np.uint64)
        check(self._lib.exacto_trivial_encrypt(self._h, pt.ctypes.data, out.ctypes.data, pt.shape[0]))
        return out

    def trivial_encrypt(self, values) -> np.ndarray:
        """digit_extract.rs:160-176 for each scalar m of `values`: (Delta (m mod t), 0)."""
        vals = [int(v) for v in np.atleast_1d(values)]
        pt = np.zeros((len(vals), self.n), dtype=np.uint64)
        pt[:, 0] = [v % self.plain_modulus for v in vals]
        return self.trivial_encrypt_poly(pt)

    def eval_poly(self, ct, coeffs) -> np.ndarray:
        """digit_extract.rs:101-157 on a batch ct [B][2][L][n]; needs the resident relin key."""
        ct = _u64(ct)
        cf = np.ascontiguousarray(np.asarray(coeffs, dtype=np.uint64))
        out = np.zeros_like(ct)
        check(self._lib.exacto_eval_poly(self._h, ct.ctypes.data, cf.ctypes.data if cf.size else None, cf.size,
                                         out.ctypes.data, ct.shape[0]))
        return out

    def eval_poly_dev(self, ct, coeffs, out, batch):
        """The same on device buffers (coeffs on the host); asynchronous on the context's stream."""
        cf = np.ascontiguousarray(np.asarray(coeffs, dtype=np.uint64))
        check(self._lib.exacto_eval_poly_dev(self._h, self._p(ct), cf.ctypes.data if cf.size else None, cf.size,
                                             self._p(out), batch))

    def _pt(self, pt, rows):
        pt = _u64(pt).reshape(rows, self.n)
        return pt

    def bfv_plain_mul(self, ct, pt) -> np.ndarray:
        """eval.rs:468-486 batched: ct [B][polys][L][n], pt [B][n] -> [B][polys][L][n]."""
        ct = _u64(ct)
        pt = self._pt(pt, ct.shape[0])
        out = np.zeros_like(ct)
        check(self._lib.exacto_bfv_plain_mul(self._h, ct.ctypes.data, ct.shape[1], pt.ctypes.data, out.ctypes.data,
                                             ct.shape[0]))
        return out

    def bfv_plain_add(self, ct, pt) -> np.ndarray:
        """eval.rs:489-503 batched: c0 + Delta m."""
        ct = _u64(ct)
        pt = self._pt(pt, ct.shape[0])
        out = np.zeros_like(ct)
        check(self._lib.exacto_bfv_plain_add(self._h, ct.ctypes.data, ct.shape[1], pt.ctypes.data, out.ctypes.data,
                                             ct.shape[0]))
        return out

    def bfv_inner_product(self, cts, pts) -> np.ndarray:
        """eval.rs:588-606: cts [K][polys][L][n], pts [K][n] -> [polys][L][n]."""
        cts = _u64(cts)
        K = cts.shape[0]
        pts = _u64(pts).reshape(K, self.n) if K else _u64(pts)
        polys = cts.shape[1] if K else 2
        out = np.zeros((polys, self.L, self.n), dtype=np.uint64)
        check(self._lib.exacto_bfv_inner_product(self._h, cts.ctypes.data, pts.ctypes.data, K, polys,
                                                 out.ctypes.data))
        return out

    def bfv_monomial_mul(self, ct, j) -> np.ndarray:
        """eval.rs:613-652 batched: X^j * ct."""
        ct = _u64(ct)
        out = np.zeros_like(ct)
        check(self._lib.exacto_bfv_monomial_mul(self._h, ct.ctypes.data, ct.shape[1], j, out.ctypes.data,
                                                ct.shape[0]))
        return out

    def bfv_trace(self, ct, elements, gks) -> np.ndarray:
        """eval.rs:572-586 batched: elements [E], gks [E][K][2][L][n] (the key of elements[e] at e)."""
        ct = _u64(ct)
        el = np.ascontiguousarray(np.asarray(elements, dtype=np.uint64))
        gks = _u64(gks)
        E = el.shape[0]
        nk = gks.shape[1] if E else 0
        out = np.zeros_like(ct)
        check(self._lib.exacto_bfv_trace(self._h, ct.ctypes.data, ct.shape[1], el.ctypes.data if E else None, E,
                                         gks.ctypes.data if E else None, nk, out.ctypes.data, ct.shape[0]))
        return out

    def gen_relin_key_dev(self, sk, key, stream, num_keys, rlk=None, sigma=3.2):
        k = self._key(key)
        check(self._lib.exacto_gen_relin_key_dev(self._h, self._p(sk), sigma, k.ctypes.data, stream, num_keys,
                                                 None if rlk is None else self._p(rlk)))

    def encrypt_sk_dev(self, pt, sk, key, stream, ct, batch, sigma=3.2):
        k = self._key(key)
        check(self._lib.exacto_encrypt_sk_dev(self._h, self._p(pt), self._p(sk), sigma, k.ctypes.data, stream,
                                              self._p(ct), batch))

    # ---- device-pointer API (asynchronous; torch tensors or raw ints)
    def _p(self, x):
        return x if isinstance(x, int) else _ptr(x)

    def ntt_fwd_dev(self, polys, count, limb=0):
        check(self._lib.exacto_ntt_fwd_dev(self._h, self._p(polys), count, limb))

    def ntt_inv_dev(self, polys, count, limb=0):
        check(self._lib.exacto_ntt_inv_dev(self._h, self._p(polys), count, limb))

    def rns_fwd_dev(self, polys, count):
        check(self._lib.exacto_rns_fwd_dev(self._h, self._p(polys), count))

    def rns_inv_dev(self, polys, count):
        check(self._lib.exacto_rns_inv_dev(self._h, self._p(polys), count))

    def rns_add_dev(self, a, b, out, count):
        check(self._lib.exacto_rns_add_dev(self._h, self._p(a), self._p(b), self._p(out), count))

    def rns_sub_dev(self, a, b, out, count):
        check(self._lib.exacto_rns_sub_dev(self._h, self._p(a), self._p(b), self._p(out), count))

    def rns_neg_dev(self, a, out, count):
        check(self._lib.exacto_rns_neg_dev(self._h, self._p(a), self._p(out), count))

    def rns_mul_dev(self, a, b, out, count):
        check(self._lib.exacto_rns_mul_dev(self._h, self._p(a), self._p(b), self._p(out), count))

    def rns_mul_inv_dev(self, a, b, out, count):
        """INTT(a (.) b) per limb, fused (exacto_rns_mul_inv_dev)."""
        check(self._lib.exacto_rns_mul_inv_dev(self._h, self._p(a), self._p(b), self._p(out), count))

    def rns_polymul_dev(self, a, b, out, count):
        """Negacyclic products of coefficient-domain polys (exacto_rns_polymul_dev)."""
        check(self._lib.exacto_rns_polymul_dev(self._h, self._p(a), self._p(b), self._p(out), count))

    def rns_scalar_mul_dev(self, a, scalar, out, count):
        check(self._lib.exacto_rns_scalar_mul_dev(self._h, self._p(a), scalar, self._p(out), count))

    def bfv_add_dev(self, a, polys1, b, polys2, out, batch):
        check(self._lib.exacto_bfv_add_dev(self._h, self._p(a), polys1, self._p(b), polys2, self._p(out), batch))

    def bfv_plain_mul_dev(self, ct, polys, pt, out, batch):
        """ct [batch][polys][L][n] times pt [batch][n] plaintext coefficients, item by item."""
        check(self._lib.exacto_bfv_plain_mul_dev(self._h, self._p(ct), polys, self._p(pt), self._p(out), batch))

    def bfv_sub_dev(self, a, polys1, b, polys2, out, batch):
        check(self._lib.exacto_bfv_sub_dev(self._h, self._p(a), polys1, self._p(b), polys2, self._p(out), batch))

    def bfv_neg_dev(self, a, polys, out, batch):
        check(self._lib.exacto_bfv_neg_dev(self._h, self._p(a), polys, self._p(out), batch))

    def bfv_mul_no_relin_dev(self, ct1, ct2, out, batch):
        check(self._lib.exacto_bfv_mul_no_relin_dev(self._h, self._p(ct1), 2, self._p(ct2), 2,
                                                    self._p(out), batch))

    def relinearize_dev(self, ct, polys, out, batch):
        check(self._lib.exacto_relinearize_dev(self._h, self._p(ct), polys, self._p(out), batch))

    def bfv_mul_and_relin_dev(self, ct1, ct2, out, batch):
        check(self._lib.exacto_bfv_mul_and_relin_dev(self._h, self._p(ct1), self._p(ct2),
                                                     self._p(out), batch))

    def bfv_square_no_relin_dev(self, ct, out, batch, polys=2):
        check(self._lib.exacto_bfv_square_no_relin_dev(self._h, self._p(ct), polys, self._p(out), batch))

    def bfv_square_and_relin_dev(self, ct, out, batch):
        check(self._lib.exacto_bfv_square_and_relin_dev(self._h, self._p(ct), self._p(out), batch))

    def bfv_apply_automorphism_dev(self, ct, element, gk, num_keys, out, batch):
        check(self._lib.exacto_bfv_apply_automorphism_dev(self._h, self._p(ct), 2, element, self._p(gk), num_keys,
                                                          self._p(out), batch))

    def gadget_decompose_dev(self, coeffs, digits, batch, num_digits):
        check(self._lib.exacto_gadget_decompose_dev(self._h, self._p(coeffs), self._p(digits),
                                                    batch, num_digits))

    def dbfv_mul_dev(self, d, base, plain, a, b, out, batch, depth_a=None, depth_b=None):
        da = np.ascontiguousarray(depth_a, dtype=np.uint32) if depth_a is not None else None
        db = np.ascontiguousarray(depth_b, dtype=np.uint32) if depth_b is not None else None
        check(self._lib.exacto_dbfv_mul_dev(self._h, d, base, plain, self._p(a), self._p(b),
                                            self._p(out), batch, _ptr(da), _ptr(db), None))

    def dbfv_square_dev(self, d, base, plain, a, out, batch, depth_a=None):
        da = np.ascontiguousarray(depth_a, dtype=np.uint32) if depth_a is not None else None
        check(self._lib.exacto_dbfv_square_dev(self._h, d, base, plain, self._p(a), self._p(out), batch, _ptr(da),
                                               None))

    def dbfv_encrypt_sk_dev(self, d, base, plain, values, sk, key, stream, ct, batch, sigma=3.2, poly=False):
        """values [B] (poly: pt [B][n]) on the device -> ct [B][d][2][L][n]."""
        fn = self._lib.exacto_dbfv_encrypt_poly_sk_dev if poly else self._lib.exacto_dbfv_encrypt_sk_dev
        k = self._key(key)
        check(fn(self._h, d, base, plain, self._p(values), self._p(sk), sigma, k.ctypes.data, stream, self._p(ct),
                 batch))

    def dbfv_encrypt_pk_dev(self, d, base, plain, values, pk, key, stream, ct, batch, sigma=3.2, poly=False):
        fn = self._lib.exacto_dbfv_encrypt_poly_pk_dev if poly else self._lib.exacto_dbfv_encrypt_pk_dev
        k = self._key(key)
        check(fn(self._h, d, base, plain, self._p(values), self._p(pk), sigma, k.ctypes.data, stream, self._p(ct),
                 batch))

    def dbfv_add_dev(self, a, d1, polys1, b, d2, polys2, out, batch, depth_a=None, depth_b=None, sub=False):
        """Returns mul_depth [B] of the results (exacto_dbfv_add_dev / exacto_dbfv_sub_dev)."""
        fn = self._lib.exacto_dbfv_sub_dev if sub else self._lib.exacto_dbfv_add_dev
        dout = np.zeros(batch, dtype=np.uint32)
        da, db = self._depths(depth_a, batch), self._depths(depth_b, batch)
        check(fn(self._h, self._p(a), d1, polys1, self._p(b), d2, polys2, self._p(out), batch, _ptr(da), _ptr(db),
                 dout.ctypes.data))
        return dout

    def dbfv_sub_dev(self, a, d1, polys1, b, d2, polys2, out, batch, depth_a=None, depth_b=None):
        return self.dbfv_add_dev(a, d1, polys1, b, d2, polys2, out, batch, depth_a, depth_b, sub=True)

    def dbfv_neg_dev(self, ct, d, polys, out, batch):
        check(self._lib.exacto_dbfv_neg_dev(self._h, self._p(ct), d, polys, self._p(out), batch))

    def dbfv_relinearize_dev(self, ct, d, polys, out, batch):
        check(self._lib.exacto_dbfv_relinearize_dev(self._h, self._p(ct), d, polys, self._p(out), batch))

    def dbfv_apply_automorphism_dev(self, ct, d, element, gk, num_keys, out, batch):
        check(self._lib.exacto_dbfv_apply_automorphism_dev(self._h, self._p(ct), d, 2, element, self._p(gk),
                                                           num_keys, self._p(out), batch))

    def dbfv_linear_map_dev(self, matrix, polys, ct, out, batch):
        """matrix [d_out][d_in] on the host; ct, out device buffers (16-byte aligned, disjoint)."""
        m = np.ascontiguousarray(np.array([[int(x) for x in row] for row in matrix], dtype=np.uint64))
        check(self._lib.exacto_dbfv_linear_map_dev(self._h, m.shape[1], m.shape[0], polys, m.ctypes.data,
                                                   self._p(ct), self._p(out), batch))

    def dbfv_change_base_dev(self, d, base, plain, new_base, new_d, ct, out, batch):
        check(self._lib.exacto_dbfv_change_base_dev(self._h, d, base, plain, new_base, new_d, self._p(ct),
                                                    self._p(out), batch))

    def dbfv_div_by_base_dev(self, d, base, plain, ct, out, batch) -> int:
        """Returns the new plain modulus p / base."""
        new_plain = C.c_uint64(0)
        check(self._lib.exacto_dbfv_div_by_base_dev(self._h, d, base, plain, self._p(ct), self._p(out), batch,
                                                    C.byref(new_plain)))
        return int(new_plain.value)

    def dbfv_mul_limbs(self, d, base, plain, a: np.ndarray, b: np.ndarray, limbs) -> np.ndarray:
        """One GPU's output limbs of a split dbfv_mul: [B][len(limbs)][2][L][n], slot s = limb limbs[s]."""
        a, b = _u64(a), _u64(b)
        ls = np.ascontiguousarray(np.asarray(limbs, dtype=np.uint32))
        out = np.zeros((a.shape[0], ls.size, 2, self.L, self.n), dtype=np.uint64)
        check(self._lib.exacto_dbfv_mul_limbs(self._h, d, base, plain, a.ctypes.data, b.ctypes.data, out.ctypes.data,
                                              a.shape[0], ls.ctypes.data if ls.size else None, ls.size))
        return out

    def dbfv_mul_limbs_dev(self, d, base, plain, a, b, out, batch, limbs):
        ls = np.ascontiguousarray(np.asarray(limbs, dtype=np.uint32))
        check(self._lib.exacto_dbfv_mul_limbs_dev(self._h, d, base, plain, self._p(a), self._p(b), self._p(out),
                                                  batch, ls.ctypes.data if ls.size else None, ls.size))

    # ---- sums of ciphertext products (exacto_bfv_mul_sum)
    @staticmethod
    def _mul_sum_terms(terms, nslots):
        """terms: [(ia, ib, slot)] -> three uint32 arrays; malformed lists are rejected here, before any
        library call (the library checks the indices against na / nb)."""
        terms = list(terms)
        ia, ib, sl = [], [], []
        for k, t in enumerate(terms):
            try:
                x, y, s = t
            except (TypeError, ValueError):
                raise ValueError(f"bfv_mul_sum: term {k} is not an (ia, ib, slot) triple: {t!r}") from None
            for name, v in (("ia", x), ("ib", y), ("slot", s)):
                if int(v) != v or not 0 <= int(v) < 1 << 32:
                    raise ValueError(f"bfv_mul_sum: term {k} has {name} = {v!r} (need an index in [0, 2^32))")
            if int(s) >= nslots:
                raise ValueError(f"bfv_mul_sum: term {k} has slot {int(s)} >= nslots = {nslots}")
            ia.append(int(x)); ib.append(int(y)); sl.append(int(s))
        if int(nslots) != nslots or nslots < 0:
            raise ValueError(f"bfv_mul_sum: nslots = {nslots!r}")
        return tuple(np.array(v, dtype=np.uint32) for v in (ia, ib, sl))

    def bfv_mul_sum(self, a: np.ndarray, b: np.ndarray, terms, nslots: int) -> np.ndarray:
        """out[i][s] = sum over terms (ia, ib, s) of bfv_mul_and_relin(a[i][ia], b[i][ib]), one key switch
        per sum: a [B][na][2][L][n], b [B][nb][2][L][n] -> [B][nslots][2][L][n]."""
        ia, ib, sl = self._mul_sum_terms(terms, nslots)
        a, b = _u64(a), _u64(b)
        B = a.shape[0]
        out = np.zeros((B, nslots, 2, self.L, self.n), dtype=np.uint64)
        check(self._lib.exacto_bfv_mul_sum(self._h, a.ctypes.data, a.shape[1], b.ctypes.data, b.shape[1],
                                           _ptr(ia), _ptr(ib), _ptr(sl), ia.size, nslots, out.ctypes.data, B))
        return out

    def bfv_mul_sum_dev(self, a, na, b, nb, terms, nslots, out, batch):
        """Device buffers a [B][na][2][L][n], b [B][nb][2][L][n] (may be the same), out [B][nslots][2][L][n];
        terms on the host.  Asynchronous on the context's stream."""
        ia, ib, sl = self._mul_sum_terms(terms, nslots)
        check(self._lib.exacto_bfv_mul_sum_dev(self._h, self._p(a), na, self._p(b), nb, _ptr(ia), _ptr(ib), _ptr(sl),
                                               ia.size, nslots, self._p(out), batch))

    def set_mul_sum_group(self, max_products: int):
        """At most this many products of one output key-switched as one sum (0: the context's own limit)."""
        check(self._lib.exacto_ctx_set_mul_sum_group(self._h, max_products))

    def mul_sum_info(self) -> dict:
        """{"group_max", "last_mode"} (exacto_bfv_mul_sum_info)."""
        gm, md = _SZ(0), C.c_int(-1)
        check(self._lib.exacto_bfv_mul_sum_info(self._h, C.byref(gm), C.byref(md)))
        return {"group_max": int(gm.value), "last_mode": int(md.value)}

    # ---- modulus switching (exacto_bfv_mod_switch)
    MOD_SWITCH_MODES = {"round": 0, "reference": 1}

    @classmethod
    def _mod_switch_args(cls, polys, limbs_in, limbs_out, mode, batch):
        """Malformed arguments are rejected here, before any library call (the library checks limbs_in
        against the context's L, and the buffers)."""
        if mode not in cls.MOD_SWITCH_MODES:
            raise ValueError(f"bfv_mod_switch: mode = {mode!r} (need one of {sorted(cls.MOD_SWITCH_MODES)})")
        for name, v in (("polys", polys), ("limbs_in", limbs_in), ("limbs_out", limbs_out), ("batch", batch)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
                raise ValueError(f"bfv_mod_switch: {name} = {v!r} (need a non-negative integer)")
        if polys < 1:
            raise ValueError("bfv_mod_switch: the ciphertext has no polynomials")
        if limbs_in < 2:
            raise ValueError(f"bfv_mod_switch: limbs_in = {limbs_in}: cannot drop prime: only one modulus remaining")
        if not 1 <= limbs_out < limbs_in:
            raise ValueError(f"bfv_mod_switch: limbs_out = {limbs_out} (need 1 <= limbs_out < limbs_in = {limbs_in})")
        return cls.MOD_SWITCH_MODES[mode]

    def bfv_mod_switch(self, ct: np.ndarray, limbs_out=None, mode="round") -> np.ndarray:
        """Drop the top primes of ct [B][polys][limbs_in][n] (over the context's first limbs_in primes) down to
        limbs_out (default: one drop) -> [B][polys][limbs_out][n], a ciphertext of a context created with
        moduli[:limbs_out].  mode "round": exact rounding division by each dropped prime; "reference": the
        reference's drop_last_rns_prime literally (unscaled)."""
        if not isinstance(ct, np.ndarray) or ct.ndim != 4:
            raise ValueError("bfv_mod_switch: ct must be a [B][polys][limbs_in][n] array")
        B, polys, lin, n = ct.shape
        if n != self.n:
            raise ValueError(f"bfv_mod_switch: ct has rows of {n} coefficients, the context n = {self.n}")
        lout = lin - 1 if limbs_out is None else limbs_out
        m = self._mod_switch_args(polys, lin, lout, mode, B)
        ct = _u64(ct)
        out = np.zeros((B, polys, int(lout), n), dtype=np.uint64)
        check(self._lib.exacto_bfv_mod_switch(self._h, ct.ctypes.data, polys, lin, int(lout), m, out.ctypes.data, B))
        return out

    def bfv_mod_switch_dev(self, ct, polys, limbs_in, limbs_out, out, batch, mode="round"):
        """Device buffers ct [batch][polys][limbs_in][n] -> out [batch][polys][limbs_out][n] (disjoint, 16-byte
        aligned).  Asynchronous on the context's stream."""
        m = self._mod_switch_args(polys, limbs_in, limbs_out, mode, batch)
        check(self._lib.exacto_bfv_mod_switch_dev(self._h, self._p(ct), int(polys), int(limbs_in), int(limbs_out), m,
                                                  self._p(out), int(batch)))

    # ---- RCCL collectives (exacto_hip.h; comm = RcclComm)
    def broadcast_relin_key(self, comm: "RcclComm", root: int, num_keys: int):
        """Root's resident relinearisation key -> this context's resident key (ncclBroadcast, in place)."""
        check(self._lib.exacto_ctx_broadcast_relin_key(self._h, comm.handle, root, num_keys))

    def broadcast_galois_key(self, comm: "RcclComm", root: int, gk_dev, num_keys: int):
        check(self._lib.exacto_broadcast_galois_key(self._h, comm.handle, root, self._p(gk_dev), num_keys))

    def allgather_u64(self, comm: "RcclComm", send, recv, count: int):
        """recv = [nranks][count] u64 (ncclAllGather on the context stream)."""
        check(self._lib.exacto_rccl_allgather_u64(self._h, comm.handle, self._p(send), self._p(recv), count))

    def rccl_sync(self, comm: "RcclComm"):
        """Wait for the collectives on the context stream, at most $EXACTO_RCCL_TIMEOUT_S seconds
        (exacto_rccl_sync); raises ExactoError on expiry (the communicator is then aborted)."""
        check(self._lib.exacto_rccl_sync(self._h, comm.handle))

    def dbfv_mul_chain_dev(self, d, base, plain, x, y, out, batch, depth):
        check(self._lib.exacto_dbfv_mul_chain_dev(self._h, d, base, plain, self._p(x), self._p(y),
                                                  self._p(out), batch, depth))

    def bfv_decrypt_dev(self, ct, polys, sk, out, batch):
        check(self._lib.exacto_bfv_decrypt_dev(self._h, self._p(ct), polys, self._p(sk), self._p(out), batch))

    def bfv_noise_dev(self, ct, polys, sk, noise_out, batch, expected=None, plain_out=None):
        """noise_out: [batch][L] uint64 words on the device (exacto_bfv_noise_dev)."""
        check(self._lib.exacto_bfv_noise_dev(self._h, self._p(ct), polys, self._p(sk), self._p(expected),
                                             self._p(plain_out), self._p(noise_out), batch))

    def dbfv_noise_dev(self, d, ct, sk, noise_out, batch):
        check(self._lib.exacto_dbfv_noise_dev(self._h, d, self._p(ct), self._p(sk), self._p(noise_out), batch))

    def dbfv_decrypt_dev(self, d, base, plain, ct, sk, out, batch, poly=False):
        fn = self._lib.exacto_dbfv_decrypt_poly_dev if poly else self._lib.exacto_dbfv_decrypt_dev
        check(fn(self._h, d, base, plain, self._p(ct), self._p(sk), self._p(out), batch))

    # ---- profiling
    def prof_enable(self, on=True):
        check(self._lib.exacto_prof_enable(self._h, 1 if on else 0))

    def prof_read(self, kind: int):
        nl, pl = C.c_uint64(), C.c_uint64()
        ms, by = C.c_double(), C.c_double()
        check(self._lib.exacto_prof_read(self._h, kind, C.byref(nl), C.byref(ms), C.byref(by),
                                         C.byref(pl)))
        return {"launches": nl.value, "ms": ms.value, "bytes": by.value, "polys": pl.value}

    def prof_kernels(self, kind: int) -> list[tuple[str, int, float]]:
        """The kernels that ran for family `kind` in the records prof_read consumed, as rocprofv3 names
        them, by descending time: [(name, launches, ms)] (exacto_prof_kernels)."""
        n = self._lib.exacto_prof_kernels(self._h, kind, None, 0)
        buf = C.create_string_buffer(n + 1)
        self._lib.exacto_prof_kernels(self._h, kind, buf, n + 1)
        out = []
        for part in filter(None, buf.value.decode().split("; ")):
            name, _, tail = part.rpartition(" (")
            cnt, ms = tail.rstrip(")").split(", ")
            out.append((name, int(cnt), float(ms.split()[0])))
        return out

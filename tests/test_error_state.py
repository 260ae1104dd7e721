"""CPU: the library has ONE last-error state, whichever host module raises the failure.

The host runtime is more than one source file (context.hip, api_decrypt.hip and rccl.hip behind
csrc/runtime.hpp).  Every module reports through fail() in context.hip, and
exacto_last_error reads that one thread-local string.  A copy of the string per source file would still
build; exacto_last_error would then answer with stale or empty text for every failure raised outside
context.hip.  So, for one entry point of each API family: a context-free call of ANOTHER family fails
first with a different message, then the entry point is called with a null context, and the code and the
text must be that call's own."""

import ctypes as C

import pytest

from exacto_amd import _ffi

EXACTO_ERR_INVALID_PARAM = 1
EXACTO_ERR_INVALID_RING_DEGREE = 4


def _rotate_rows_bad_degree(lib):      # SIMD batching
    element = C.c_uint64(0)
    assert lib.exacto_galois_element_rotate_rows(48, 1, C.byref(element)) == EXACTO_ERR_INVALID_RING_DEGREE
    return "ring degree must be a power of 2, got 48"


def _change_base_bad_base(lib):        # dBFV maps between digit vectors
    out = (C.c_uint64 * 4)()
    assert lib.exacto_dbfv_change_base_matrix(2, 16, 256, 1, 2, out) == EXACTO_ERR_INVALID_PARAM
    return "invalid parameter: new base must be >= 2"


def _lagrange_nine_points_mod_7(lib):  # digit extraction
    values = (C.c_uint64 * 9)(*([1] * 9))
    out = (C.c_uint64 * 9)()
    assert lib.exacto_lagrange_interpolate(values, 9, 7, out) == EXACTO_ERR_INVALID_PARAM
    return "invalid parameter: points must be distinct mod p"


DECOYS = (_rotate_rows_bad_degree, _change_base_bad_base, _lagrange_nine_points_mod_7)

# (entry point, its API family); with the decoys taken in rotation no entry follows a decoy of its own family
ENTRIES = [
    ("exacto_ctx_set_chunk", "context"),
    ("exacto_bfv_mul_and_relin", "BFV products"),
    ("exacto_dbfv_mul", "dBFV products"),
    ("exacto_bfv_decrypt", "decryption (api_decrypt.hip)"),
    ("exacto_gen_secret_key", "keygen"),
    ("exacto_bfv_plain_mul", "plaintext operations"),
    ("exacto_eval_poly", "digit extraction"),
    ("exacto_batch_encode", "SIMD batching"),
    ("exacto_bfv_rotate_hoisted", "hoisted rotations"),
    ("exacto_dbfv_neg", "dBFV limb-wise operations"),
    ("exacto_rccl_sync", "RCCL (rccl.hip)"),
]


def _null_args(fn):
    """Every pointer null (the context first of all), every count and scalar zero."""
    return [0.0 if t is C.c_double else 0 if t in (C.c_size_t, C.c_uint64, C.c_int64, C.c_int, C.c_uint32) else None
            for t in fn.argtypes]


@pytest.mark.parametrize("i", range(len(ENTRIES)), ids=[e[0] for e in ENTRIES])
def test_null_context_message_after_a_failure_elsewhere(i):
    lib = _ffi.load()
    name, _family = ENTRIES[i]
    decoy_text = DECOYS[i % len(DECOYS)](lib)
    assert _ffi.last_error() == decoy_text
    fn = getattr(lib, name)
    assert fn.argtypes[0] is C.c_void_p
    assert fn(*_null_args(fn)) == EXACTO_ERR_INVALID_PARAM
    assert _ffi.last_error() == "invalid parameter: null context"

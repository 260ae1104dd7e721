"""The slot convention of SIMD batching on the CPU (tests/batch_ref.py), the Galois-element helpers of the
library (host only) and the header's wording of the batching errors.

The convention (include/exacto_hip.h): m(zeta^(3^i)) = values[i], m(zeta^(2n - 3^i)) = values[n/2 + i].
Checked here in Python integers: decode through NttPlan equals evaluation by Horner's rule; the negacyclic
product is the slot-wise product; sigma_{3^k} rotates both rows left by k; sigma_{2n-1} swaps the rows; the
relative-trace chain of required_trace_elements(n) leaves the sum of all slots in every slot.
"""

import os
import random

import numpy as np
import pytest

import batch_ref as R
from exacto_amd import _ffi
from oracle import bootstrap as ob
from oracle.ring import find_psi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(16, 97), (32, 193), (64, 65537)]


def _values(n, t, seed):
    rng = random.Random(seed)
    return [rng.randrange(t) for _ in range(n)]


@pytest.mark.parametrize("n,t", SHAPES)
def test_decode_is_evaluation_at_the_slot_roots(n, t):
    m = _values(n, t, 1)
    assert R.decode_direct(m, n, t) == R.decode(m, n, t)
    v = _values(n, t, 2)
    assert R.decode_direct(R.encode(v, n, t), n, t) == v
    assert R.encode(R.decode(m, n, t), n, t) == m
    # zeta is the library's root rule applied to t
    zeta = find_psi(n, t)
    assert pow(zeta, n, t) == t - 1
    assert sorted(R.slot_exponents(n)) == list(range(1, 2 * n, 2))


@pytest.mark.parametrize("n,t", SHAPES)
def test_single_slots_and_constants(n, t):
    assert R.encode([5] * n, n, t) == [5] + [0] * (n - 1)          # a constant polynomial is 5 in every slot
    for s in (0, 1, n // 2 - 1, n // 2, n - 1):
        e = [0] * n
        e[s] = 1
        m = R.encode(e, n, t)
        assert R.decode_direct(m, n, t) == e


@pytest.mark.parametrize("n,t", SHAPES)
def test_product_is_slotwise(n, t):
    a, b = _values(n, t, 3), _values(n, t, 4)
    ma, mb = R.encode(a, n, t), R.encode(b, n, t)
    prod = R.negacyclic_mul(ma, mb, n, t)
    assert prod == R.negacyclic_mul_naive(ma, mb, n, t)
    assert R.decode(prod, n, t) == [x * y % t for x, y in zip(a, b)]


@pytest.mark.parametrize("n,t", SHAPES)
def test_rotation_and_swap(n, t):
    v = _values(n, t, 5)
    m = R.encode(v, n, t)
    for k in (0, 1, 2, n // 2 - 1, n // 2, n // 2 + 3):
        got = R.decode(R.automorphism(m, pow(3, k, 2 * n), n, t), n, t)
        assert got == R.rotate_rows(v, k, n), k
    # right rotations: 3^-k
    got = R.decode(R.automorphism(m, pow(3, -1, 2 * n), n, t), n, t)
    assert got == R.rotate_rows(v, -1, n)
    assert R.decode(R.automorphism(m, 2 * n - 1, n, t), n, t) == R.swap_rows(v, n)
    assert R.rotate_rows(list(range(n)), 1, n)[:3] == [1, 2, 3] and R.rotate_rows(list(range(n)), 1, n)[n // 2 - 1] == 0


def test_trace_chain_sums_the_slots():
    n, t = 64, 65537
    v = _values(n, t, 6)
    m = R.encode(v, n, t)
    elements = ob.required_trace_elements(n)
    assert elements == [65, 33, 17, 9, 5, 3]
    for k in elements:                                   # bfv_trace: result <- result + sigma_k(result)
        m = [(x + y) % t for x, y in zip(m, R.automorphism(m, k, n, t))]
    assert R.decode(m, n, t) == [sum(v) % t] * n


@pytest.mark.parametrize("n,t", SHAPES + [(1024, 12289), (1024, 4294957057), (16, 4294966657)])
def test_vectorised_rows_equal_the_plan(n, t):
    rng = np.random.default_rng(n + t)
    v = rng.integers(0, t, size=(3, n), dtype=np.uint64)
    v[0] = t - 1
    enc = R.encode_many(v, n, t)
    assert enc.tolist() == [R.encode(row.tolist(), n, t) for row in v]
    dec = R.decode_many(v, n, t)
    assert dec.tolist() == [R.decode(row.tolist(), n, t) for row in v]
    assert np.array_equal(R.decode_many(enc, n, t), v)


def test_galois_element_helpers():
    for n in (16, 64, 4096):
        for k in (0, 1, -1, n // 2, n // 2 + 3, -(n // 2) - 1):
            assert _ffi.galois_element_rotate_rows(n, k) == pow(3, k % (n // 2), 2 * n), (n, k)
        assert _ffi.galois_element_rotate_rows(n, -1) == pow(3, -1, 2 * n)
        assert _ffi.galois_element_swap_rows(n) == 2 * n - 1
    with pytest.raises(_ffi.ExactoError) as e:
        _ffi.galois_element_rotate_rows(48, 1)
    assert e.value.variant == "InvalidRingDegree"


def test_header_states_the_errors():
    with open(os.path.join(ROOT, "include", "exacto_hip.h"), encoding="utf-8") as f:
        header = " ".join(f.read().replace("*", " ").split())
    for text in ("batching requires a prime plaintext modulus t ≡ 1 (mod 2n), got t={t}, n={n}",
                 "batching for plaintext moduli >= 2^32",
                 "plaintext {v} >= plain_modulus {t}",
                 "REDUCES every value mod t"):
        assert text in header, text
    for name in ("exacto_batch_info", "exacto_batch_encode_dev", "exacto_batch_decode_dev", "exacto_bfv_rotate_rows_dev",
                 "exacto_bfv_swap_rows_dev", "exacto_batch_encrypt_sk_dev", "exacto_batch_encrypt_pk_dev",
                 "exacto_batch_decrypt_dev", "exacto_galois_element_rotate_rows", "exacto_galois_element_swap_rows"):
        assert name in header and name in _ffi.EXPORTED_SYMBOLS, name

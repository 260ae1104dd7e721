"""Slot-packed dBFV on the CPU (tests/dbfv_batch_ref.py): n integers mod p per dBFV plaintext.

Slot encoding is a ring isomorphism and every dBFV operation is a Z-linear combination of limb products, so
the operations act slot by slot, with the digit growth of the SCALAR case.  Checked here in Python integers
at the plaintext level (digits -> slot encoding -> limb convolutions -> small_reps fold -> decode -> signed
recomposition): products, sums and differences are slot-wise mod p, sigma_{3^k} rotates the wide slots and
sigma_{2n-1} swaps their rows.  t = 1153 with p = 251 is the documented failure: the folded digits reach
100 + 5 * 225 = 1225 > t / 2.  One run per n = 16 shape goes through the oracle's own ciphertext-level
dbfv_mul: the shapes of tests/test_gpu_dbfv_batch.py decrypt under the oracle alone.
"""

import os
import random

import pytest

import batch_ref as R
import dbfv_batch_ref as D
from exacto_amd import _ffi
from oracle import bfv as obfv, dbfv as odbfv, params as P
from oracle.ring import CoeffPoly, NttPlan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, t, base, d, p); p = 0 is 2^64
SETS = [(16, 1153, 16, 2, 256), (16, 1040449, 256, 8, 0), (16, 2753, 16, 2, 251), (32, 33423041, 256, 2, 65521)]
CT_SHAPES = SETS[:2]          # the n = 16 shapes of the GPU end-to-end tests


def _values(n, p, seed):
    """Slots 0 .. 3 hold p - 1, 0, 1, p - 1; the rest are uniform."""
    m = D.modulus(p)
    rng = random.Random(seed)
    v = [rng.randrange(m) for _ in range(n)]
    v[:4] = [m - 1, 0, 1, m - 1]
    return v


@pytest.mark.parametrize("n,t,base,d,p", SETS)
def test_parameter_sets(n, t, base, d, p):
    assert NttPlan.try_new(n, t) is not None and t < 1 << 32
    assert base <= t and base ** d >= D.modulus(p)
    assert D.min_digits(base, p) <= d


def test_the_nonzero_small_representative():
    assert odbfv.small_reps(16, 2, 251) == [[5, 0]]
    assert odbfv.small_reps(256, 2, 65521) == [[15, 0]]


@pytest.mark.parametrize("n,t,base,d,p", SETS)
def test_round_trip_and_reduction(n, t, base, d, p):
    m = D.modulus(p)
    v = _values(n, p, 1)
    pt = D.encode(v, n, t, d, base, p)
    assert len(pt) == d and all(len(row) == n and max(row) < t for row in pt)
    assert D.decode(pt, n, t, d, base, p) == v
    big = [x + m * (i % 3) for i, x in enumerate(v)]
    if p:                                                    # values >= p are reduced
        assert D.encode(big, n, t, d, base, p) == pt
    assert D.decode([[c + t * 5 for c in row] for row in pt], n, t, d, base, p) == v    # coefficients mod t
    # a constant is "all slots equal": every limb is the constant polynomial of the digit
    const = D.encode([m - 1] * n, n, t, d, base, p)
    assert const == [[dg] + [0] * (n - 1) for dg in odbfv.digit_decompose(m - 1, base, d)]
    assert D.encode_many([v, big], n, t, d, base, p).tolist() == [pt, D.encode(big, n, t, d, base, p)]
    assert D.decode_many([pt, const], n, t, d, base, p).tolist() == [v, [m - 1] * n]


@pytest.mark.parametrize("n,t,base,d,p", SETS)
def test_product_sum_and_difference_are_slotwise(n, t, base, d, p):
    m = D.modulus(p)
    a, b = _values(n, p, 2), _values(n, p, 3)
    b[3], b[4] = m - 1, m - 2                                # (p - 1)^2 in slot 3
    x, y = D.encode(a, n, t, d, base, p), D.encode(b, n, t, d, base, p)
    dec = lambda pt: D.decode(pt, n, t, d, base, p)
    assert dec(D.limb_mul(x, y, n, t, d, base, p)) == [u * w % m for u, w in zip(a, b)]
    assert dec(D.limb_mul(x, x, n, t, d, base, p)) == [u * u % m for u in a]
    assert dec(D.limb_add(x, y, t)) == [(u + w) % m for u, w in zip(a, b)]
    assert dec(D.limb_add(x, y, t, -1)) == [(u - w) % m for u, w in zip(a, b)]


def test_t_too_small_for_the_folded_digits():
    """t = 1153 serves p = 256 (limb 1 reaches 2 * 15^2 = 450 < 576) but not p = 251, whose fold adds 5 times
    limb 2 to limb 0: (p - 1)^2 has limb 0 = 10 * 10 + 5 * 15 * 15 = 1225 > t / 2."""
    n, t, base, d, p = 16, 1153, 16, 2, 251
    a = [p - 1] * n
    x = D.encode(a, n, t, d, base, p)
    got = D.decode(D.limb_mul(x, x, n, t, d, base, p), n, t, d, base, p)
    assert got != [1] * n                                    # (p - 1)^2 = 1 mod p
    t_ok = 2753
    x = D.encode(a, n, t_ok, d, base, p)
    assert D.decode(D.limb_mul(x, x, n, t_ok, d, base, p), n, t_ok, d, base, p) == [1] * n


@pytest.mark.parametrize("n,t,base,d,p", SETS)
def test_rotation_and_swap_move_the_wide_slots(n, t, base, d, p):
    v = _values(n, p, 4)
    pt = D.encode(v, n, t, d, base, p)
    for k in (1, 2, n // 2 - 1):
        got = D.decode(D.automorphism(pt, pow(3, k, 2 * n), n, t), n, t, d, base, p)
        assert got == R.rotate_rows(v, k, n), k
    got = D.decode(D.automorphism(pt, pow(3, -1, 2 * n), n, t), n, t, d, base, p)
    assert got == R.rotate_rows(v, -1, n)
    assert D.decode(D.automorphism(pt, 2 * n - 1, n, t), n, t, d, base, p) == R.swap_rows(v, n)


def oracle_params(n, t, base, d, p):
    """The BFV parameters of the GPU end-to-end tests: cfg3's three 60-bit primes, gadget base 2^16."""
    bfv = P.BfvParamsBuilder().ring_degree(n).plain_modulus(t).ct_moduli(P.Q3).build()
    return P.DbfvParams(bfv, base, d, p)


@pytest.mark.parametrize("n,t,base,d,p", CT_SHAPES)
def test_the_oracles_dbfv_mul_on_slot_encoded_digits(n, t, base, d, p):
    dp = oracle_params(n, t, base, d, p)
    prm, m = dp.bfv_params, D.modulus(p)
    rng = random.Random(n + d)
    sk = obfv.gen_secret_key(prm, rng)
    rlk = obfv.gen_relin_key(sk, rng)
    a, b = _values(n, p, 5), _values(n, p, 6)
    b[3] = m - 1

    def encrypt(values):
        limbs = [obfv.encrypt_sk(CoeffPoly(row, t), sk, rng) for row in D.encode(values, n, t, d, base, p)]
        return odbfv.DbfvCiphertext(limbs, d, 0, dp)

    prod = odbfv.dbfv_mul(encrypt(a), encrypt(b), rlk)
    assert prod.num_limbs() == d
    pt = [obfv.decrypt(limb, sk).coeffs for limb in prod.limbs]
    assert D.decode(pt, n, t, d, base, p) == [u * w % m for u, w in zip(a, b)]


def test_header_states_the_convention_and_the_errors():
    with open(os.path.join(ROOT, "include", "exacto_hip.h"), encoding="utf-8") as f:
        header = " ".join(f.read().replace("*", " ").split())
    for text in ("dBFV base {b} must be <= BFV plaintext modulus {t}",
                 "dbfv_plain_modulus = 0 (p = 2^64) is ALLOWED in all of these calls",
                 "every slot is a scalar of its own",
                 "any overlap of values and pt",
                 "that of the SCALAR dBFV case",
                 "t > 2 d (b - 1)^2 = 1040400",
                 "item b d + k of exacto_encrypt_sk / exacto_encrypt_pk",
                 "batch == 0 returns 0"):
        assert text in header, text
    for op in ("encode", "decode", "encrypt_sk", "encrypt_pk", "decrypt"):
        for sfx in ("", "_dev"):
            name = f"exacto_dbfv_batch_{op}{sfx}"
            assert name in header and name in _ffi.EXPORTED_SYMBOLS, name

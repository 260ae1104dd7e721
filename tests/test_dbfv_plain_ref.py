"""dBFV plaintext products on the CPU (tests/dbfv_plain_ref.py): public digit vectors times dBFV ciphertexts.

  1. the helper's two forms (the literal composition on oracle objects, the direct NTT-domain sums) agree;
  2. encryptions made by the oracle and multiplied by the reference decrypt, slot by slot, to sum_k w_k a_k
     mod p, with the extremes in slots 0 .. 3 of every operand: the ciphertext-level margin (noise about
     fresh * n * t * d * K against Delta about 2^150) is confirmed here, not assumed;
  3. the bound on t binds: three shapes whose digits outgrow t / 2 do not decode;
  4. plain_add / plain_sub are slot-wise too;
  5. the new symbols are exported, bound and declared.
"""

import os
import random

import numpy as np
import pytest

import dbfv_batch_ref as D
import dbfv_plain_ref as PR
from bridge import ct_to_np, np_to_ct, uniform_residues
from exacto_amd import _ffi
from oracle import bfv as obfv
from oracle.ring import CoeffPoly
from test_dbfv_batch_ref import oracle_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = 1 << 64
P64 = U64 - 59

# (n, t, base, d, p, K); p = 0 is 2^64
DECODES = [
    (16, 1153, 16, 2, 256, 1),
    (16, 12289, 16, 2, 256, 3),
    (64, 12289, 16, 2, 251, 3),                 # a non-zero fold
    (16, 1040449, 256, 8, 0, 1),
    (16, 1073750017, 256, 8, 0, 3),
    (16, 1073750017, 256, 8, P64, 3),           # large fold digits
]
# the same operands with t too small for the digits of the sum
DOES_NOT_DECODE = [
    (16, 1153, 16, 2, 256, 2),
    (64, 1153, 16, 2, 251, 1),
    (16, 1040449, 256, 8, 0, 2),
]

NEW_SYMBOLS = [f"exacto_dbfv_plain_{op}{sfx}" for op in ("mul_sum", "mul", "add", "sub") for sfx in ("", "_dev")]
NEW_SYMBOLS += ["exacto_ctx_set_plain_terms", "exacto_dbfv_plain_limits"]


def operands(n, p, K, seed):
    """a, w [K][n] below p: slots 0 .. 3 of every a are 0, 1, p - 1, p - 1, of every w p - 1, p - 1, p - 1, p - 2."""
    m = D.modulus(p)
    rng = random.Random(seed)
    a = [[rng.randrange(m) for _ in range(n)] for _ in range(K)]
    w = [[rng.randrange(m) for _ in range(n)] for _ in range(K)]
    for k in range(K):
        a[k][:4] = [0, 1, m - 1, m - 1]
        w[k][:4] = [m - 1, m - 1, m - 1, m - 2]
    return a, w


def slotwise_dot(a, w, p):
    m = D.modulus(p)
    return [sum(x[s] * y[s] for x, y in zip(a, w)) % m for s in range(len(a[0]))]


@pytest.mark.parametrize("base,d,p", [(16, 2, 251), (256, 8, 0), (256, 8, P64), (3, D.min_digits(3, 10 ** 9 + 7), 10 ** 9 + 7),
                                      (16, 2, 256), (2, 1, 2)])
@pytest.mark.parametrize("K,polys", [(1, 2), (3, 3)])
def test_the_two_forms_agree(base, d, p, K, polys):
    n, B = 16, 2
    dp = oracle_params(n, 1073750017, base, d, p)
    prm = dp.bfv_params
    q = prm.ct_basis.moduli
    rng = np.random.default_rng(d * 100 + K)
    cts = uniform_residues(rng, (B, K, d, polys), q, n)
    pts = rng.integers(0, U64, size=(B, K, d, n), dtype=np.uint64)
    pts[0, 0, 0, :2] = [U64 - 1, 0]
    for pb in (B, 1):
        direct = PR.mul_sum_direct(cts, pts[:pb], q, base, d, p)
        for b in range(B):
            lit = PR.mul_sum_literal([[np_to_ct(cts[b, k, j], prm) for j in range(d)] for k in range(K)],
                                     pts[b if pb == B else 0].tolist(), dp)
            assert lit.num_limbs() == d and lit.mul_depth == 1
            assert np.array_equal(np.stack([ct_to_np(limb) for limb in lit.limbs]), direct[b]), (pb, b)


def _encrypt_decrypt_dot(n, t, base, d, p, K):
    dp = oracle_params(n, t, base, d, p)
    prm = dp.bfv_params
    rng = random.Random(n + d + K)
    sk = obfv.gen_secret_key(prm, rng)
    a, w = operands(n, p, K, 17 * K + d)
    cts = [[obfv.encrypt_sk(CoeffPoly(row, t), sk, rng) for row in D.encode(a[k], n, t, d, base, p)] for k in range(K)]
    pts = [D.encode(w[k], n, t, d, base, p) for k in range(K)]
    out = PR.mul_sum_literal(cts, pts, dp)
    got = D.decode([obfv.decrypt(limb, sk).coeffs for limb in out.limbs], n, t, d, base, p)
    return got, slotwise_dot(a, w, p), (cts, pts, a, w, sk, dp)


@pytest.mark.parametrize("n,t,base,d,p,K", DECODES)
def test_oracle_encryptions_decrypt_to_the_slotwise_dot_product(n, t, base, d, p, K):
    got, want, _ = _encrypt_decrypt_dot(n, t, base, d, p, K)
    assert got == want


@pytest.mark.parametrize("n,t,base,d,p,K", DOES_NOT_DECODE)
def test_the_bound_on_t_binds(n, t, base, d, p, K):
    got, want, _ = _encrypt_decrypt_dot(n, t, base, d, p, K)
    assert got != want


@pytest.mark.parametrize("n,t,base,d,p", [(16, 1153, 16, 2, 256), (16, 1040449, 256, 8, 0), (16, 1040449, 256, 8, P64)])
def test_plain_add_and_sub_are_slotwise(n, t, base, d, p):
    dp = oracle_params(n, t, base, d, p)
    prm, m = dp.bfv_params, D.modulus(p)
    q = prm.ct_basis.moduli
    rng = random.Random(d)
    sk = obfv.gen_secret_key(prm, rng)
    (a,), (w,) = operands(n, p, 1, 3)
    limbs = [obfv.encrypt_sk(CoeffPoly(row, t), sk, rng) for row in D.encode(a, n, t, d, base, p)]
    pt = D.encode(w, n, t, d, base, p)
    ct = np.stack([ct_to_np(limb) for limb in limbs])[None]
    for sub in (False, True):
        out = PR.addsub_direct(ct, np.array([pt], dtype=np.uint64), q, t, sub)
        if not sub:                                           # the literal bfv_plain_add, limb by limb
            lit = [ct_to_np(obfv.bfv_plain_add(limb, CoeffPoly(row, t))) for limb, row in zip(limbs, pt)]
            assert np.array_equal(out[0], np.stack(lit))
        dec = [obfv.decrypt(np_to_ct(out[0, k], prm), sk).coeffs for k in range(d)]
        sign = -1 if sub else 1
        assert D.decode(dec, n, t, d, base, p) == [(x + sign * y) % m for x, y in zip(a, w)], sub


def test_symbols_exported_and_bound():
    lib = _ffi.load()
    with open(os.path.join(ROOT, "include", "exacto_hip.rs")) as f:
        rs = f.read()
    with open(os.path.join(ROOT, "include", "exacto_hip.h")) as f:
        hdr = f.read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _ffi.EXPORTED_SYMBOLS
        assert f"pub fn {name}(" in rs, name
        assert f"{name}(" in hdr, name
    for method in ("dbfv_plain_mul", "dbfv_plain_mul_sum", "dbfv_plain_add", "dbfv_plain_sub", "dbfv_batch_plain_mul",
                   "dbfv_batch_plain_dot", "dbfv_batch_plain_add", "dbfv_batch_plain_sub"):
        assert hasattr(_ffi.HipContext, method) and hasattr(_ffi.HipContext, method + "_dev"), method


def test_header_states_the_definition_and_the_errors():
    with open(os.path.join(ROOT, "include", "exacto_hip.h"), encoding="utf-8") as f:
        header = " ".join(f.read().replace("*", " ").split())
    for text in ("cts [B][K][d][polys][L][n]", "pts [pt_batch][K][d][n]", "out[i] = wide[i] + sum_{m >= d} rep[m-d][i] wide[m]",
                 "mismatched ct/pt lengths", "pt_batch not in {1, B}", "A batching context is NOT required",
                 "batch == 0 returns 0"):
        assert text in header, text

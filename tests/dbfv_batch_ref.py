"""Slot-packed dBFV in Python integers (test helper): n integers mod p per dBFV plaintext.

The convention of include/exacto_hip.h (exacto_dbfv_batch_*): every slot value is reduced mod p (p = 0 means
2^64: taken as it is), decomposed into d base-b digits (oracle.dbfv.digit_decompose), and row k of the
plaintext is batch_ref's slot encoding mod t of the vector of k-th digits.  decode slot-decodes every row and
recomposes each slot with oracle.dbfv.digit_recompose_signed (digits centred at t // 2, then mod p).

limb_mul is dBFV's product at the plaintext level: the d x d negacyclic limb products mod t summed by
i + j, then folded with oracle.dbfv.small_reps exactly as oracle.dbfv.reduce folds ciphertext limbs.
"""

from __future__ import annotations

import batch_ref as R
from oracle.dbfv import digit_decompose, digit_recompose_signed, small_reps


def modulus(p: int) -> int:
    return 1 << 64 if p == 0 else p


def min_digits(base: int, p: int) -> int:
    """The smallest d with base^d >= p."""
    d = 1
    while base ** d < modulus(p):
        d += 1
    return d


def digits(values, d: int, base: int, p: int) -> list[list[int]]:
    """values[n] -> [d][n]: row k holds every slot's k-th digit."""
    cols = [digit_decompose(int(v) % modulus(p), base, d) for v in values]
    return [[c[k] for c in cols] for k in range(d)]


def encode(values, n: int, t: int, d: int, base: int, p: int) -> list[list[int]]:
    """values[n] -> pt [d][n]."""
    assert base <= t
    return [R.encode(row, n, t) for row in digits(values, d, base, p)]


def decode(pt, n: int, t: int, d: int, base: int, p: int) -> list[int]:
    """pt [d][n] (any integers, taken mod t) -> values[n]."""
    assert len(pt) == d
    rows = [R.decode(row, n, t) for row in pt]
    return [digit_recompose_signed([rows[k][s] for k in range(d)], base, p, t) for s in range(n)]


def encode_many(values, n: int, t: int, d: int, base: int, p: int):
    """encode on values [B][n] at once -> uint64 [B][d][n] (batch_ref.encode_many on the digit rows)."""
    import numpy as np
    v = [[int(x) for x in row] for row in values]
    dig = np.array([digits(row, d, base, p) for row in v], dtype=np.uint64).reshape(len(v) * d, n)
    return R.encode_many(dig, n, t).reshape(len(v), d, n)


def decode_many(pt, n: int, t: int, d: int, base: int, p: int):
    """decode on pt [B][d][n] at once -> uint64 [B][n]."""
    import numpy as np
    pt = np.asarray(pt, dtype=np.uint64)
    B = pt.shape[0]
    rows = R.decode_many(pt.reshape(B * d, n), n, t).reshape(B, d, n).tolist()
    out = [[digit_recompose_signed([rows[b][k][s] for k in range(d)], base, p, t) for s in range(n)]
           for b in range(B)]
    return np.array(out, dtype=np.uint64)


def limb_add(x, y, t: int, sign: int = 1):
    """Limb-wise sum (sign = -1: difference) mod t of two plaintexts [d][n]."""
    return [[(a + sign * b) % t for a, b in zip(rx, ry)] for rx, ry in zip(x, y)]


def limb_mul(x, y, n: int, t: int, d: int, base: int, p: int):
    """dbfv_mul on plaintexts [d][n]: limb products by i + j, then the small_reps fold (oracle.dbfv.reduce)."""
    wide = [[0] * n for _ in range(2 * d - 1)]
    for i in range(d):
        for j in range(d):
            prod = R.negacyclic_mul(x[i], y[j], n, t)
            wide[i + j] = [(a + b) % t for a, b in zip(wide[i + j], prod)]
    res = wide[:d]
    for j, rep in enumerate(small_reps(base, d, p)):
        for i, coeff in enumerate(rep):
            if coeff:
                res[i] = [(a + coeff * b) % t for a, b in zip(res[i], wide[d + j])]
    return res


def automorphism(pt, k: int, n: int, t: int):
    """sigma_k on every limb of a plaintext [d][n]."""
    return [R.automorphism(row, k, n, t) for row in pt]

"""SIMD batching mod a plaintext prime t == 1 (mod 2n) in Python integers (test helper).

The convention of include/exacto_hip.h: zeta = oracle.ring.find_psi(n, t); a slot vector values[n] is a
2 x n/2 matrix (row 0 = values[:n/2], row 1 = values[n/2:]); with e_i = 3^i mod 2n the plaintext m(X)
mod t has m(zeta^e_i) = values[i] and m(zeta^(2n - e_i)) = values[n/2 + i].

encode / decode go through oracle.ring.NttPlan(n, t): in the library's evaluation numbering (evaluation
k = a(psi^(2 brv(k) + 1)), stored at storage_order()'s position) slot exponent e is evaluation
brv((e - 1) / 2), so encode places the values, inverse-transforms and normalises, and decode is the
mirror image.  decode_direct evaluates m at zeta^e by Horner's rule and knows nothing of the transform.
"""

from __future__ import annotations

import functools

from oracle.ring import NttPlan, bit_reverse, find_psi


def slot_exponents(n: int) -> list[int]:
    """Exponent e of slot i: 3^i mod 2n for row 0, 2n - 3^i mod 2n for row 1."""
    row0 = [pow(3, i, 2 * n) for i in range(n // 2)]
    return row0 + [2 * n - e for e in row0]


@functools.lru_cache(maxsize=None)
def _plan(n: int, t: int) -> NttPlan:
    plan = NttPlan.try_new(n, t)
    assert plan is not None, f"t = {t} is not a prime == 1 mod {2 * n}"
    return plan


@functools.lru_cache(maxsize=None)
def slot_positions(n: int, t: int) -> tuple[int, ...]:
    """slot -> position of its evaluation in NttPlan's storage (storage_order() is position -> evaluation)."""
    logn = n.bit_length() - 1
    pos_of_eval = [0] * n
    for p, k in enumerate(_plan(n, t).storage_order()):
        pos_of_eval[k] = p
    return tuple(pos_of_eval[bit_reverse((e - 1) // 2, logn)] for e in slot_exponents(n))


def encode(values, n: int, t: int) -> list[int]:
    """values[n] (any integers, taken mod t) -> coefficients of m(X) in [0, t)."""
    assert len(values) == n
    plan = _plan(n, t)
    a = [0] * n
    for v, p in zip(values, slot_positions(n, t)):
        a[p] = int(v) % t
    plan.inv(a)
    plan.normalize(a)
    return a


def decode(coeffs, n: int, t: int) -> list[int]:
    """coefficients (any integers, taken mod t) -> values[n]."""
    assert len(coeffs) == n
    plan = _plan(n, t)
    a = [int(c) % t for c in coeffs]
    plan.fwd(a)
    return [a[p] for p in slot_positions(n, t)]


def _tables(n: int, t: int):
    import numpy as np
    plan = _plan(n, t)
    return (np.array(plan.psi_rev, dtype=np.uint64), np.array(plan.psi_inv_rev, dtype=np.uint64),
            np.array(plan.storage_order(), dtype=np.int64), np.array(slot_positions(n, t), dtype=np.int64))


def encode_many(values, n: int, t: int):
    """encode on every row of values [B][n] at once: NttPlan.inv's loops (its tables, its stage order)
    on numpy uint64 rows.  t < 2^32, so no product leaves 64 bits.  tests/test_batch_ref.py holds it
    against encode."""
    import numpy as np
    assert t < 1 << 32
    _, tw, order, pos = _tables(n, t)
    q = np.uint64(t)
    v = np.asarray(values, dtype=np.uint64) % q
    B = v.shape[0]
    stored = np.zeros((B, n), dtype=np.uint64)
    stored[:, pos] = v
    a = np.zeros((B, n), dtype=np.uint64)
    a[:, order] = stored                                   # NttPlan.inv: a[k] = stored[p]
    tt, m = 1, n
    while m > 1:
        h = m >> 1
        x = a.reshape(B, h, 2, tt)
        u, w = x[:, :, 0, :].copy(), x[:, :, 1, :].copy()
        x[:, :, 0, :] = (u + w) % q
        x[:, :, 1, :] = (u + q - w) % q * tw[h:m, None] % q
        tt <<= 1
        m = h
    return a * np.uint64(_plan(n, t).n_inv) % q


def decode_many(coeffs, n: int, t: int):
    """decode on every row of coeffs [B][n] at once (NttPlan.fwd's loops, as encode_many)."""
    import numpy as np
    assert t < 1 << 32
    tw, _, order, pos = _tables(n, t)
    q = np.uint64(t)
    a = np.asarray(coeffs, dtype=np.uint64) % q
    B = a.shape[0]
    tt, m = n, 1
    while m < n:
        tt >>= 1
        x = a.reshape(B, m, 2, tt)
        u, w = x[:, :, 0, :].copy(), x[:, :, 1, :] * tw[m:2 * m, None] % q
        x[:, :, 0, :] = (u + w) % q
        x[:, :, 1, :] = (u + q - w) % q
        m <<= 1
    return a[:, order][:, pos]                             # stored[p] = std[order[p]], slot i at pos[i]


def decode_direct(coeffs, n: int, t: int) -> list[int]:
    """values[i] = m(zeta^e_i) by Horner's rule."""
    zeta = find_psi(n, t)
    out = []
    for e in slot_exponents(n):
        x = pow(zeta, e, t)
        acc = 0
        for c in reversed(coeffs):
            acc = (acc * x + int(c)) % t
        out.append(acc)
    return out


def automorphism(coeffs, k: int, n: int, t: int) -> list[int]:
    """sigma_k: m(X) -> m(X^k) mod (X^n + 1, t), k odd."""
    assert k % 2 == 1
    out = [0] * n
    for i, c in enumerate(coeffs):
        e = i * k % (2 * n)
        if e < n:
            out[e] = (out[e] + int(c)) % t
        else:
            out[e - n] = (out[e - n] - int(c)) % t
    return out


def negacyclic_mul(a, b, n: int, t: int) -> list[int]:
    """a(X) b(X) mod (X^n + 1, t), through the transform (the product of evaluations)."""
    plan = _plan(n, t)
    fa, fb = [int(x) % t for x in a], [int(x) % t for x in b]
    plan.fwd(fa)
    plan.fwd(fb)
    c = [x * y % t for x, y in zip(fa, fb)]
    plan.inv(c)
    plan.normalize(c)
    return c


def negacyclic_mul_naive(a, b, n: int, t: int) -> list[int]:
    """The schoolbook product, for the small sizes that check negacyclic_mul."""
    out = [0] * n
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            if i + j < n:
                out[i + j] = (out[i + j] + x * y) % t
            else:
                out[i + j - n] = (out[i + j - n] - x * y) % t
    return out


def rotate_rows(values, k: int, n: int) -> list[int]:
    """Both rows left by k."""
    h = n // 2
    return [values[(i + k) % h] for i in range(h)] + [values[h + (i + k) % h] for i in range(h)]


def swap_rows(values, n: int) -> list[int]:
    h = n // 2
    return list(values[h:]) + list(values[:h])

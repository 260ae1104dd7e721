"""bfv_apply_automorphism (eval.rs:512-561) on whole batches at any n (test helper).

The oracle's own steps (oracle/bfv.py bfv_apply_automorphism) with the transforms and the products in
oracle/c: inverse transforms, the coefficient permutation X^i -> X^(ik), the exact CRT and the balanced
gadget digits of c1 in Python integers (oracle.bfv.gadget_decompose_coeff itself), then
c0' = sigma(c0) + sum_g d_g k_g0 and c1' = sum_g d_g k_g1 per limb.  The products run in the coefficient
domain (cref.polymul of a digit with the key's inverse transform), which is the same residue as the
NTT-domain product the reference forms: the transform is linear and exact mod q_i.
tests/test_automorphism_ref.py holds this against the Python oracle at a small n.
"""

from __future__ import annotations

import math

import numpy as np

from oracle import bfv as obfv, cref


def _per_limb(fn, x, moduli):
    """x [...][L][n] -> fn(q_i, rows of limb i) stacked back."""
    L, n = x.shape[-2:]
    rows = np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, L, n)
    return np.stack([fn(q, np.ascontiguousarray(rows[:, i])) for i, q in enumerate(moduli)], axis=1).reshape(x.shape)


def apply_automorphism(prm, ct: np.ndarray, element: int, gk: np.ndarray, threads: int = 1) -> np.ndarray:
    """ct [B][2][L][n], gk [keys][2][L][n] (NTT domain, the library's order) -> [B][2][L][n]."""
    moduli = [int(q) for q in prm.ct_basis.moduli]
    n, L = prm.ring_degree, len(moduli)
    B = ct.shape[0]
    guse = min(prm.gadget_digits, gk.shape[0])
    assert guse > 0 and element % 2 == 1
    qcol = np.array(moduli, dtype=np.uint64)[:, None]
    coef = _per_limb(lambda q, r: cref.ntt(n, q, r, inverse=True, threads=threads), ct, moduli)
    key = _per_limb(lambda q, r: cref.ntt(n, q, r, inverse=True, threads=threads), gk[:guse], moduli)
    # X^i -> X^(i k): coefficient i moves to i k mod 2n, negated past n (k odd: a bijection)
    e = (np.arange(n, dtype=np.int64) * (element % (2 * n))) % (2 * n)
    dst, neg = np.where(e < n, e, e - n), e >= n
    sig = np.empty_like(coef)
    sig[..., dst] = np.where(neg, (qcol - coef) % qcol, coef)
    # the digits of sigma(c1): exact CRT to [0, Q), then the oracle's balanced decomposition, residues mod q_i
    Q = math.prod(moduli)
    terms = [(q, pow(Q // q, -1, q), Q // q) for q in moduli]
    out = np.empty_like(ct)
    for b in range(B):
        c1 = [[int(v) for v in sig[b, 1, i]] for i in range(L)]
        if L == 1:
            xs = c1[0]
        else:
            xs = [sum(c1[i][j] * inv % q * qs for i, (q, inv, qs) in enumerate(terms)) % Q for j in range(n)]
        cols = [obfv.gadget_decompose_coeff(x, Q, prm.gadget_base, prm.gadget_digits)[:guse] for x in xs]
        for i, q in enumerate(moduli):
            dig = np.array([[col[g] % q for col in cols] for g in range(guse)], dtype=np.uint64)   # [guse][n]
            acc = [sig[b, 0, i].copy(), np.zeros(n, dtype=np.uint64)]
            for k in range(2):
                prod = cref.polymul(n, q, dig, np.ascontiguousarray(key[:, k, i]), threads=threads)
                for g in range(guse):
                    acc[k] = (acc[k] + prod[g]) % np.uint64(q)       # both below 2^62: no wrap
                out[b, k, i] = cref.ntt(n, q, acc[k][None, :])[0]
    return out

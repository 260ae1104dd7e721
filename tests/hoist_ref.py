"""Hoisted rotations and slot linear transforms (exacto_bfv_rotate_hoisted / exacto_bfv_linear_transform) on
whole batches at any n (test helper, after automorphism_ref.py).

out[b][r] = (sigma_r(c0) + sum_g sigma_r(d_g) k_{r,g,0}, sum_g sigma_r(d_g) k_{r,g,1}) per limb, with d_g the
balanced gadget digits of the exact CRT of c1 ITSELF (oracle.bfv.gadget_decompose_coeff in Python integers):
the transforms run through oracle/c, sigma_r acts on each digit's residues in the coefficient domain (index
i -> i k mod 2n, negated past n), the products are cref.polymul of a permuted digit with the key's inverse
transform, and the result goes forward again.  Element 1 copies the input.  Not the bits of
bfv_apply_automorphism, which decomposes sigma(c1): tests/test_hoist_ref.py shows both that and the equal
decryptions.
"""

from __future__ import annotations

import math

import numpy as np

from oracle import bfv as obfv, cref

from automorphism_ref import _per_limb


def _brv(x: int, bits: int) -> int:
    return int(format(x, f"0{bits}b")[::-1], 2) if bits else 0


def ntt_permutation(n: int, k: int) -> np.ndarray:
    """perm[p] = storage position whose value lands at storage position p under sigma_k:
    NTT(sigma_k(a))[p] = NTT(a)[perm[p]].  Evaluation j sits at (j mod 16) n/16 + j // 16, and evaluation j of
    sigma_k(a) is evaluation j' of a with brv(j') = ((2 brv(j) + 1) k mod 2n - 1) / 2."""
    bits, m = n.bit_length() - 1, n // 16
    k %= 2 * n
    assert k % 2 == 1
    perm = np.empty(n, dtype=np.uint32)
    for p in range(n):
        j = (p % m) * 16 + p // m
        j2 = _brv((((2 * _brv(j, bits) + 1) * k) % (2 * n) - 1) // 2, bits)
        perm[p] = (j2 % 16) * m + j2 // 16
    return perm


def _sigma(coef: np.ndarray, element: int, qcol) -> np.ndarray:
    """X^i -> X^(i k) on [...][n] residues mod qcol (broadcast against [..., n])."""
    n = coef.shape[-1]
    e = (np.arange(n, dtype=np.int64) * (element % (2 * n))) % (2 * n)
    dst, neg = np.where(e < n, e, e - n), e >= n
    sig = np.empty_like(coef)
    sig[..., dst] = np.where(neg, (qcol - coef) % qcol, coef)
    return sig


def digit_columns(prm, c1_coef: np.ndarray, guse: int):
    """c1 [L][n] (coefficient domain) -> per coefficient the first guse balanced digits of its exact CRT."""
    moduli = [int(q) for q in prm.ct_basis.moduli]
    L, n = c1_coef.shape
    Q = math.prod(moduli)
    c1 = [[int(v) for v in c1_coef[i]] for i in range(L)]
    if L == 1:
        xs = c1[0]
    else:
        terms = [(q, pow(Q // q, -1, q), Q // q) for q in moduli]
        xs = [sum(c1[i][j] * inv % q * qs for i, (q, inv, qs) in enumerate(terms)) % Q for j in range(n)]
    return [obfv.gadget_decompose_coeff(x, Q, prm.gadget_base, prm.gadget_digits)[:guse] for x in xs]


def rotate_hoisted(prm, ct: np.ndarray, elements, gks: np.ndarray, threads: int = 1) -> np.ndarray:
    """ct [B][2][L][n], gks [R][keys][2][L][n] (NTT domain, the library's order) -> [B][R][2][L][n]."""
    moduli = [int(q) for q in prm.ct_basis.moduli]
    n, L = prm.ring_degree, len(moduli)
    B, R = ct.shape[0], len(elements)
    guse = min(prm.gadget_digits, gks.shape[1])
    coef = _per_limb(lambda q, r: cref.ntt(n, q, r, inverse=True, threads=threads), ct, moduli)
    key = _per_limb(lambda q, r: cref.ntt(n, q, r, inverse=True, threads=threads), gks[:, :guse], moduli)
    out = np.empty((B, R, 2, L, n), dtype=np.uint64)
    for b in range(B):
        cols = digit_columns(prm, coef[b, 1], guse)
        for i, q in enumerate(moduli):
            dig = np.array([[col[g] % q for col in cols] for g in range(guse)], dtype=np.uint64)   # [guse][n]
            for r, el in enumerate(elements):
                if el % (2 * n) == 1:
                    out[b, r, :, i] = ct[b, :, i]
                    continue
                sd = np.ascontiguousarray(_sigma(dig, el, np.uint64(q)))
                acc = [_sigma(coef[b, 0, i], el, np.uint64(q)), np.zeros(n, dtype=np.uint64)]
                for k in range(2):
                    prod = cref.polymul(n, q, sd, np.ascontiguousarray(key[r, :, k, i]), threads=threads)
                    for g in range(guse):
                        acc[k] = (acc[k] + prod[g]) % np.uint64(q)       # both below 2^62: no wrap
                    out[b, r, k, i] = cref.ntt(n, q, np.ascontiguousarray(acc[k])[None, :])[0]
    return out


def linear_transform(prm, hoisted: np.ndarray, pts: np.ndarray, threads: int = 1) -> np.ndarray:
    """hoisted [B][R][2][L][n] (NTT domain), pts [R][n] plaintext coefficients -> sum_r pt_r * hoisted[:, r]."""
    moduli = [int(q) for q in prm.ct_basis.moduli]
    n, L = prm.ring_degree, len(moduli)
    B, R = hoisted.shape[:2]
    coef = _per_limb(lambda q, r: cref.ntt(n, q, r, inverse=True, threads=threads), hoisted, moduli)
    out = np.empty((B, 2, L, n), dtype=np.uint64)
    for i, q in enumerate(moduli):
        ptq = np.ascontiguousarray(np.asarray(pts, dtype=np.uint64) % np.uint64(q))
        for b in range(B):
            for k in range(2):
                prod = cref.polymul(n, q, np.ascontiguousarray(coef[b, :, k, i]), ptq, threads=threads)
                acc = np.zeros(n, dtype=np.uint64)
                for r in range(R):
                    acc = (acc + prod[r]) % np.uint64(q)
                out[b, k, i] = cref.ntt(n, q, acc[None, :])[0]
    return out

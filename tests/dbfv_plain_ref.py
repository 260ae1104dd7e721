"""dBFV plaintext products in Python integers (test helper): public digit vectors times dBFV ciphertexts.

The definition of include/exacto_hip.h (exacto_dbfv_plain_mul_sum): with P[k][i] = NTT(pts[k][i] mod q_l) and
wide[m] the sum over k and over i + j = m of P[k][i] (.) cts[k][j], out[i] = wide[i] + sum_{m >= d}
rep[m - d][i] wide[m] with rep = oracle.dbfv.small_reps(base, d, p), canonical residues mod q_l.  Two forms:

  literal  the composition itself on oracle objects: oracle.bfv.bfv_plain_mul per digit pair, bfv_add by i + j
           and over k, oracle.dbfv.reduce on the DbfvCiphertext of degree 2d - 1;
  direct   the same sums in the NTT domain on numpy arrays of Python integers (the digit vectors multiplied as
           polynomials in a power of two, one reduction per output residue), for n = 1024.

tests/test_dbfv_plain_ref.py holds them against each other.
"""

from __future__ import annotations

import functools

import numpy as np

from oracle import bfv as obfv, dbfv as odbfv
from oracle.ring import CoeffPoly, make_plan

U64 = 1 << 64


def mul_sum_literal(cts, pts, dp):
    """cts[k][j]: BfvCiphertext (limb j of term k), pts[k][i]: n integers (any, reduced mod each q_l) ->
    the d limbs of reduce(sum_k pts[k] * cts[k]) as a DbfvCiphertext of depth 1."""
    d = dp.num_digits
    limbs = [None] * (2 * d - 1)
    for ct_k, pt_k in zip(cts, pts):
        assert len(ct_k) == d and len(pt_k) == d
        for i in range(d):
            for j in range(d):
                prod = obfv.bfv_plain_mul(ct_k[j], CoeffPoly([int(c) for c in pt_k[i]], U64))
                limbs[i + j] = prod if limbs[i + j] is None else obfv.bfv_add(limbs[i + j], prod)
    return odbfv.reduce(odbfv.DbfvCiphertext(limbs, 2 * d - 1, 1, dp))


@functools.lru_cache(maxsize=None)
def _plan(n, q):
    return make_plan(n, q)


def ntt_rows(a, n, q):
    """Forward transforms of the rows of a [rows][n] (Python integers below q), in the library's storage order:
    oracle.ring.NttPlan.fwd stage by stage on whole arrays."""
    plan = _plan(n, q)
    rows = a.shape[0]
    t, m = n, 1
    while m < n:
        t >>= 1
        v = a.reshape(rows, m, 2, t)
        s = np.array(plan.psi_rev[m:2 * m], dtype=object).reshape(1, m, 1)
        u, w = v[:, :, 0, :], v[:, :, 1, :] * s % q
        a = np.stack([(u + w) % q, (u - w) % q], axis=2).reshape(rows, n)
        m <<= 1
    return a[:, plan.storage_order()]


def lift(pts, moduli, n):
    """pts [...][n] (any u64) -> NTT(pts mod q_l) as Python integers [...][L][n]."""
    pts = np.asarray(pts, dtype=np.uint64)
    flat = pts.reshape(-1, n).astype(object)
    out = np.stack([ntt_rows(flat % q, n, q) for q in moduli], axis=1)
    return out.reshape(pts.shape[:-1] + (len(moduli), n))


def mul_sum_direct(cts, pts, moduli, base, d, p, lifted=None):
    """cts [B][K][d][polys][L][n], pts [B or 1][K][d][n] -> out [B][d][polys][L][n] (uint64); lifted:
    lift(pts, ...) when the caller already has it.

    The digit vectors are multiplied as polynomials in 2^S (Kronecker substitution): with S wider than any
    wide limb, one integer product per position and term holds all 2d - 1 sums over i + j = m in its S-bit
    fields, and one more product per high limb (by the integer whose 2^S2 fields are that limb's fold digits)
    holds its contribution to every output limb.  A wide limb with an all-zero representative contributes
    nothing, formed or not."""
    cts = np.asarray(cts, dtype=np.uint64)
    B, K, _, polys, L, n = cts.shape
    P = lift(pts, moduli, n) if lifted is None else lifted          # [pb][K][d][L][n]
    C = cts.astype(object)
    reps = odbfv.small_reps(base, d, p)
    S = 2 * max(moduli).bit_length() + (d * K).bit_length()         # a wide limb is below 2^S
    S2 = S + base.bit_length() + d.bit_length()                     # ... and a folded sum below 2^S2
    W = 0
    for k in range(K):
        pk = sum(P[:, k, i] * (1 << (i * S)) for i in range(d))
        ck = sum(C[:, k, j] * (1 << (j * S)) for j in range(d))
        W = W + pk[:, None] * ck                                    # [B][polys][L][n]
    wide = [(W >> (m * S)) & ((1 << S) - 1) for m in range(2 * d - 1)]
    F = 0
    for m in range(d, 2 * d - 1):
        r = sum(reps[m - d][i] << (i * S2) for i in range(d))
        if r:
            F = F + wide[m] * r
    q = np.array(moduli, dtype=object).reshape(1, 1, L, 1)
    out = np.zeros((B, d, polys, L, n), dtype=np.uint64)
    for i in range(d):
        out[:, i] = ((wide[i] + ((F >> (i * S2)) & ((1 << S2) - 1))) % q).astype(np.uint64)
    return out


def addsub_direct(ct, pt, moduli, plain, sub=False):
    """ct [B][d][polys][L][n], pt [B or 1][d][n] -> limb k: c0 +- NTT(Delta (pt mod q_l) mod q_l), Delta =
    floor(Q / t) (oracle.bfv.bfv_plain_add limb by limb)."""
    ct = np.asarray(ct, dtype=np.uint64)
    n, L = ct.shape[-1], ct.shape[-2]
    Q = 1
    for q in moduli:
        Q *= q
    delta = Q // plain
    pt = np.asarray(pt, dtype=np.uint64)
    flat = pt.reshape(-1, n).astype(object)
    dm = np.stack([ntt_rows(flat % q * (delta % q) % q, n, q) for q in moduli], axis=1)
    dm = dm.reshape(pt.shape[:-1] + (L, n))                          # [pb][d][L][n]
    q = np.array(moduli, dtype=object).reshape(1, 1, L, 1)
    out = ct.copy()
    c0 = ct[:, :, 0].astype(object)
    out[:, :, 0] = ((c0 - dm if sub else c0 + dm) % q).astype(np.uint64)
    return out

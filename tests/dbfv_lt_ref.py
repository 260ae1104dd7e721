"""Slot linear transforms on dBFV ciphertexts with wide public diagonals (test helper): the definition of
include/exacto_hip.h (exacto_dbfv_linear_transform) and nothing else.

    H [B*d][R][2][L][n] = hoist_ref.rotate_hoisted of the B*d limbs taken as BFV ciphertexts
    out [B][d][2][L][n] = dbfv_plain_ref.mul_sum_direct(cts[b][r][j] = H[b*d + j][r], pts [1][R][d][n])

No arithmetic of its own: the rotations are hoist_ref's, the sums and the fold dbfv_plain_ref's.
"""

from __future__ import annotations

import numpy as np

import dbfv_plain_ref as PR
import hoist_ref


def rotate_hoisted(prm, ct: np.ndarray, elements, gks: np.ndarray, threads: int = 1) -> np.ndarray:
    """ct [B][d][2][L][n] -> [B][R][d][2][L][n]: limb j of out[b][r] is hoist_ref's [b*d + j][r]."""
    ct = np.asarray(ct, dtype=np.uint64)
    B, d = ct.shape[:2]
    H = hoist_ref.rotate_hoisted(prm, ct.reshape((B * d,) + ct.shape[2:]), elements, gks, threads=threads)
    H = H.reshape((B, d, len(elements)) + ct.shape[2:])
    return np.ascontiguousarray(H.transpose(0, 2, 1, 3, 4, 5))


def linear_transform(prm, ct: np.ndarray, elements, gks: np.ndarray, pts: np.ndarray, base: int, d: int, p: int,
                     threads: int = 1, rotated: np.ndarray | None = None) -> np.ndarray:
    """ct [B][d][2][L][n], pts [R][d][n] plaintext coefficients (any u64) -> out [B][d][2][L][n]; rotated:
    rotate_hoisted(...) when the caller already has it."""
    moduli = [int(q) for q in prm.ct_basis.moduli]
    H = rotate_hoisted(prm, ct, elements, gks, threads) if rotated is None else rotated
    pts = np.asarray(pts, dtype=np.uint64)
    return PR.mul_sum_direct(H, pts[None], moduli, base, d, p)

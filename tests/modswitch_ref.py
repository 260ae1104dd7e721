"""Modulus switching (exacto_bfv_mod_switch) in Python integers (test helper).

One drop, level l -> l - 1 (include/exacto_hip.h): q = q_{l-1}, Q' = q_0 ... q_{l-2}, x in [0, Q' q) the
CRT value of a coefficient.
  "round":      y = floor((2 x + q) / (2 q)) mod Q'   (round(x / q); q odd, no ties)
                limb i = (c_i - delta) q^-1 mod q_i, delta the centred residue of x mod q
  "reference":  drop_last_rns_prime (modswitch.rs:37-87): limb i = c_i - (u mod q_i), u = x mod q in [0, q)
Both are linear per coefficient, so the per-limb forms hold in the NTT domain once delta (or u) has been
forward-transformed under q_i.  Several drops are single drops from the top.
"""

from __future__ import annotations

import math

import numpy as np

from oracle import bfv as obfv, cref
from oracle.params import BfvParamsBuilder
from oracle.ring import RnsBasis, RnsPoly, crt_exact

MODES = ("round", "reference")


def centred(r: int, q: int) -> int:
    """The residue of r mod q in [-(q-1)/2, (q-1)/2] (q odd)."""
    r %= q
    return r - q if r > (q - 1) // 2 else r


def round_div(x: int, q: int, Qp: int) -> int:
    """The division form of the exact mode on a CRT value x in [0, Q' q)."""
    return ((2 * x + q) // (2 * q)) % Qp


def drop_limbs(limbs, moduli, mode="round"):
    """limbs [l][n] residues of one polynomial's coefficients (any domain in which the map is applied
    coefficient by coefficient: here the coefficient domain) -> [l-1][n], per-limb formulas."""
    assert mode in MODES and len(limbs) == len(moduli) >= 2
    q = moduli[-1]
    last = limbs[-1]
    out = []
    for c, qi in zip(limbs[:-1], moduli[:-1]):
        if mode == "round":
            inv = pow(q % qi, -1, qi)
            out.append([(int(a) - centred(int(u), q)) * inv % qi for a, u in zip(c, last)])
        else:
            out.append([(int(a) - int(u) % qi) % qi for a, u in zip(c, last)])
    return out


def drop_np(ct: np.ndarray, moduli, n: int, mode="round", drops=1) -> np.ndarray:
    """ct [...][l][n] uint64, NTT domain, the library's storage order, over moduli (l of them) ->
    [...][l - drops][n]: inverse transforms, drop_limbs per polynomial, forward transforms."""
    moduli = list(moduli)
    l = ct.shape[-2]
    assert l == len(moduli) and ct.shape[-1] == n and 1 <= drops < l
    rows = np.ascontiguousarray(ct, dtype=np.uint64).reshape(-1, l, n)
    coef = np.stack([cref.ntt(n, q, rows[:, i], inverse=True) for i, q in enumerate(moduli)], axis=1)
    polys = [[[int(v) for v in coef[r, i]] for i in range(l)] for r in range(rows.shape[0])]
    for k in range(drops):
        polys = [drop_limbs(p, moduli[:l - k], mode) for p in polys]
    lo = l - drops
    res = np.array(polys, dtype=np.uint64).reshape(-1, lo, n)
    out = np.stack([cref.ntt(n, q, res[:, i]) for i, q in enumerate(moduli[:lo])], axis=1)
    return out.reshape(ct.shape[:-2] + (lo, n))


def lower_params(prm, limbs_out=None):
    """The parameters of the context a switched ciphertext lives in: moduli[:limbs_out] (one drop by
    default), same n, p, sigma and gadget base."""
    m = prm.ct_basis.moduli
    lo = len(m) - 1 if limbs_out is None else limbs_out
    return (BfvParamsBuilder().ring_degree(prm.ring_degree).plain_modulus(prm.plain_modulus)
            .ct_moduli(m[:lo]).sigma(prm.sigma).gadget_base(prm.gadget_base).build())


def lower_key(sk, lower):
    """sk restricted to the lower parameters' primes (the per-prime tables depend only on (n, q_i))."""
    lo = len(lower.ct_basis.moduli)
    return obfv.SecretKey(RnsPoly(sk.poly.components[:lo], sk.poly.ring_degree), lower, sk.signed)


def drop_ct(ct, mode="round"):
    """One drop of an oracle ciphertext; the result carries lower_params (also in reference mode, where
    the reference itself keeps the old params: its polys have L - 1 limbs either way)."""
    prm = ct.params
    moduli = prm.ct_basis.moduli
    lower = lower_params(prm)
    comps = [RnsPoly.from_limb_coeffs(drop_limbs(c.limb_coeffs(), moduli, mode), lower.ct_basis) for c in ct.c]
    return obfv.BfvCiphertext(comps, lower)


def drop_crt(xs, moduli, mode="round"):
    """CRT values x_j in [0, Q) -> y_j in [0, Q'), through the per-limb formulas."""
    limbs = drop_limbs([[x % q for x in xs] for q in moduli], moduli, mode)
    return crt_exact(limbs, RnsBasis(list(moduli[:-1]), len(xs)))


def noise_bound(noise_before: int, q: int, p: int, n: int) -> int:
    """Ternary secret, degree-1 ciphertext, one exact drop: Delta_Q / q = Delta_Q' + theta with |theta| < 1
    (so m Delta_Q / q is within p of m Delta_Q'), and the rounding term |delta_0 + delta_1 s| / q <=
    (n + 1) / 2."""
    return noise_before // q + p + n // 2 + 2


def product(moduli) -> int:
    return math.prod(moduli)


# ------------------------------------------------------------------ boundary inputs of the GPU tests

def boundary_positions(n: int) -> list[int]:
    """Coefficient positions at the edges of a thread's 16 values, of a wave and of the row."""
    return sorted({j for j in (0, 1, 15, 16, 63, 64, n // 16 - 1, n // 16, n // 2 + 5, n - 1) if 0 <= j < n})


def boundary_values(moduli, n, rnd):
    """x = k q + r over remainders r at the centring boundary and quotients k at both ends of [0, Q'):
    includes Q - (q + 1) / 2 (rounds to Q' - 1), Q - (q - 1) / 2 and Q - 1 (wrap to 0)."""
    q = moduli[-1]
    Qp = math.prod(moduli[:-1])
    h = (q - 1) // 2
    rs = [0, 1, h - 1, h, h + 1, h + 2, q - 1]
    ks = [0, 1, Qp - 1, None]
    xs = [(rnd.randrange(Qp) if k is None else k) * q + r for k in ks for r in rs]
    return xs, boundary_positions(n)


def boundary_batch(moduli, n, B, polys, seed=0):
    """(ct [B][polys][l][n] NTT domain, xs [B][polys][n] CRT values): the boundary values at the boundary
    positions, round robin over the polynomials (every slot filled), random values elsewhere.  Built from
    coefficient values, so each coefficient is an independent lane of the kernel."""
    import random
    from worstcase import to_ntt
    rnd = random.Random(seed)
    Q = math.prod(moduli)
    vals, pos = boundary_values(moduli, n, rnd)
    slots = B * polys * len(pos)
    assert slots >= len(vals), "every boundary value is placed at least once"
    xs = [[[rnd.randrange(Q) for _ in range(n)] for _ in range(polys)] for _ in range(B)]
    for s in range(slots):
        pi, j = divmod(s, len(pos))
        b, k = divmod(pi, polys)
        if s >= len(vals) and s % len(vals) == 0:
            vals, _ = boundary_values(moduli, n, rnd)   # fresh random quotients for the next pass
        xs[b][k][pos[j]] = vals[s % len(vals)]
    ct = np.stack([np.stack([to_ntt(p, moduli, n) for p in item]) for item in xs])
    return ct, xs

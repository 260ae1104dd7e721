"""Inputs that put s = [p T]_Q at the centring boundary of the float-sum scale paths (test helper).

kernels.hip fpq_y / fpq_acc centre s by beta = rint(f), f the float sum tests/test_fpq.py restates, and
send a lane to the Garner fallback where |f - beta| > 1/2 - 2^-40.  A uniform coefficient does that with
probability about 2^-39, so these inputs are built to do it in most lanes of a wave and not in the rest.

With ct2 = (1, 0) (c0 the constant polynomial 1, c1 = 0) the integer tensor of ct1 * ct2 is T0 = ct1.c0,
T1 = ct1.c1, T2 = 0 coefficient by coefficient: no convolution mixes the lanes, so a coefficient
x = s p^-1 mod Q (centred) of ct1 gives [p T]_Q = s in that lane.  With ct2 = (0, 1) it is T1 = ct1.c0,
T2 = ct1.c1: the boundary reaches the third component, whose rounding feeds the gadget digits and the key
switch.  The scaled result is then scale_round(x, p, Q, Q >> 1) per coefficient (`closed_form`), without
the oracle's tensor.

Boundary values of s (h = floor(Q/2)), in this order:
  h - k, h + 1 + k (k = 0..7) and h - (Q >> e), h + 1 + (Q >> e) for e = 45, 41: inside the band (Garner);
  the same for e = 39, 38: just outside it (fast path);
  0, 1, 2, Q - 1, Q - 2: f next to an integer from either side (fast path).
Lanes 0..63 cycle through the list (one wave mixing both paths); for n > 64, lane j >= 64 takes the next
value of the cycle when j % 7 == 0 and lane n - 1 always does, every other lane is a uniform residue.

Ciphertext components are centred integer coefficient vectors moved to the NTT domain with
tests/worstcase.py to_ntt (the C restatement's transform).

Special primes outside Q3 / Q4 are searched, not listed: the primes == 1 mod `step` in
(2^60 - 2^24, 2^60) from the bottom of the window upward, so d = 2^60 - q is about 2^23.9 (where the
special-prime bounds of reduce_near60, dot30_fold, mulmod_near60, the asm NTT rounds, fpq_flush and
ks32_crt are tight) and clear of the library's auxiliary primes, which are taken from the top.
"""

from __future__ import annotations

import hashlib
import math
import random

import numpy as np

from oracle import params as P
from oracle.bfv import scale_round
from bridge import uniform_residues
from test_fpc_crt import is_prime
from test_fpq import LIM, fpq
from worstcase import to_ntt

IN_BAND_E = (45, 41)      # |s -+ Q/2| <= Q >> 41: the lane must take Garner
FAST_E = (39, 38)         # Q >> 39 or further from +-Q/2: the lane must take the float sum
WINDOW_LO = (1 << 60) - (1 << 24)

# the bottom of the special window, as the search must return it
LOW_16384 = [1152921504590675969, 1152921504591020033, 1152921504591216641, 1152921504591265793]
LOW_2048 = [1152921504590110721, 1152921504590143489, 1152921504590346241, 1152921504590368769,
            1152921504590419969, 1152921504590493697]


def low_window_primes(step: int, count: int) -> list[int]:
    """The `count` smallest primes == 1 mod step in (2^60 - 2^24, 2^60)."""
    out = []
    cand = WINDOW_LO // step * step + 1
    while cand <= WINDOW_LO:
        cand += step
    while len(out) < count and cand < 1 << 60:
        if is_prime(cand):
            out.append(cand)
        cand += step
    assert len(out) == count, (step, count, out)
    want = {16384: LOW_16384, 2048: LOW_2048}.get(step)
    if want is not None:
        assert out == want[:count], (step, out)
    return out


def low_params(n: int, L: int, plain: int, base: int = 0):
    """BfvParams over the L lowest special primes usable at ring degree n (== 1 mod 16384 for n >= 4096,
    mod 2048 below)."""
    step = 16384 if n >= 4096 else 2048
    assert step % (2 * n) == 0
    return (P.BfvParamsBuilder().ring_degree(n).plain_modulus(plain).ct_moduli(low_window_primes(step, L))
            .gadget_base(base).build())


def boundary_values(Q: int) -> list[tuple[int, str]]:
    """[(s, kind)] with kind "band" (Garner expected) or "fast"."""
    h = Q // 2
    out = []
    for k in range(8):
        out += [(h - k, "band"), (h + 1 + k, "band")]
    for es, kind in ((IN_BAND_E, "band"), (FAST_E, "fast")):
        for e in es:
            out += [(h - (Q >> e), kind), (h + 1 + (Q >> e), kind)]
    out += [(s, "fast") for s in (0, 1, 2, Q - 1, Q - 2)]
    return out


def boundary_lane(j: int, n: int) -> bool:
    return j < 64 or j % 7 == 0 or j == n - 1


def centre(x: int, Q: int) -> int:
    return x - Q if x > Q // 2 else x


def boundary_poly(moduli, plain, n, seed):
    """Centred coefficients x_j with [p x_j]_Q on the boundary list in the lanes of `boundary_lane`, a
    uniform residue elsewhere."""
    Q = math.prod(moduli)
    vals = [s for s, _ in boundary_values(Q)]
    pinv = pow(plain, -1, Q)
    rng = random.Random(seed)
    out, nxt = [], 0
    for j in range(n):
        if boundary_lane(j, n):
            x = vals[nxt % len(vals)] * pinv % Q
            nxt += 1
        else:
            x = rng.randrange(Q)
        out.append(centre(x, Q))
    return out


def pz_consts(moduli, plain):
    """z_i = T_i pz_i mod q_i (context.hip fpq_pz): p (Q / q_i)^-1 mod q_i."""
    Q = math.prod(moduli)
    return [plain % q * pow((Q // q) % q, -1, q) % q for q in moduli]


def in_band(moduli, plain, coeffs) -> list[bool]:
    """Per coefficient: the model of the kernel's float sum (test_fpq.fpq) sends the lane to Garner."""
    pz = pz_consts(moduli, plain)
    out = []
    for x in coeffs:
        _, f, b = fpq([x % q for q in moduli], moduli, pz)
        out.append(abs(f - b) > LIM)
    return out


def const_poly(c: int, n: int) -> list[int]:
    return [c] + [0] * (n - 1)


def bfv_case(prm, which, seed=41):
    """(ct1, ct2, (a0, a1)): ct1 = (A, A reversed) [1][2][L][n], ct2 = (1, 0) for which = "c0c1" (T0, T1
    on the boundary) or (0, 1) for "c1c2" (T1, T2); a0, a1 the centred coefficients of ct1."""
    q, n, p = prm.ct_basis.moduli, prm.ring_degree, prm.plain_modulus
    a0 = boundary_poly(q, p, n, seed)
    a1 = a0[::-1]
    one, zero = to_ntt(const_poly(1, n), q, n), to_ntt(const_poly(0, n), q, n)
    ct1 = np.stack([to_ntt(a0, q, n), to_ntt(a1, q, n)])[None]
    ct2 = np.stack({"c0c1": [one, zero], "c1c2": [zero, one]}[which])[None]
    return ct1, ct2, (a0, a1)


def closed_form(prm, coeffs, which):
    """bfv_mul_no_relin of bfv_case's inputs without the oracle: [1][3][L][n], the two boundary
    components NTT(scale_round(x_j, p, Q, Q >> 1)), the third zero."""
    q, n, p = prm.ct_basis.moduli, prm.ring_degree, prm.plain_modulus
    Q = math.prod(q)
    r = [to_ntt([scale_round(x, p, Q, Q >> 1) for x in a], q, n) for a in coeffs]
    zero = to_ntt(const_poly(0, n), q, n)
    return np.stack({"c0c1": [r[0], r[1], zero], "c1c2": [zero, r[0], r[1]]}[which])[None]


def uniform_key(prm, seed=43):
    return uniform_residues(np.random.default_rng(seed), (prm.gadget_digits, 2), prm.ct_basis.moduli,
                            prm.ring_degree)


def dbfv_case(dp, seed=42):
    """(a, b, rlk) for dbfv_mul, a and b [1][d][2][L][n]: limb k of a is (A, A reversed) for even k and
    (A reversed, A) for odd k, every limb of b is (1, 0), the key uniform.  Every product's c0 / c1 tensor
    is then A or its reverse, so an output limb's psum row adds Garner-fallback products and float-sum
    products (flushed by fpq_flush) into the same carry."""
    prm = dp.bfv_params
    q, n, d = prm.ct_basis.moduli, prm.ring_degree, dp.num_digits
    A = boundary_poly(q, prm.plain_modulus, n, seed)
    fw, bw = to_ntt(A, q, n), to_ntt(A[::-1], q, n)
    one, zero = to_ntt(const_poly(1, n), q, n), to_ntt(const_poly(0, n), q, n)
    a = np.stack([np.stack([fw, bw] if k % 2 == 0 else [bw, fw]) for k in range(d)])[None]
    b = np.stack([np.stack([one, zero]) for _ in range(d)])[None]
    return a, b, uniform_key(prm, seed + 1)


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.uint64).tobytes()).hexdigest()


# ---------------------------------------------------------------- the two digest-pinned n = 8192 cases

def digest_inputs(name):
    """(params, x, y, rlk) of tests/golden/digests.json `name`: boundary_cfg5_dbfv (dbfv_mul at cfg5) or
    boundary_low4_bfv (bfv_mul_and_relin over the four lowest special primes == 1 mod 16384, "c1c2")."""
    if name == "boundary_cfg5_dbfv":
        dp = P.cfg5_params(8192)
        return (dp,) + dbfv_case(dp)
    if name == "boundary_low4_bfv":
        prm = low_params(8192, 4, 1040407, 256)
        ct1, ct2, _ = bfv_case(prm, "c1c2")
        return prm, ct1, ct2, uniform_key(prm)
    raise ValueError(name)

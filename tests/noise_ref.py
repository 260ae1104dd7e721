"""Noise of a BFV / dBFV ciphertext in Python big integers (test helper).

Definition (include/exacto_hip.h, exacto_bfv_noise): Q = prod q_i, p the plain modulus, Delta = floor(Q / p),
x_j = CRT(INTT(sum_k c_k s^k))_j in [0, Q) the phase oracle.bfv.decrypt rounds,
    m_j   = floor((x_j p + floor(Q/2)) / Q) mod p   (or expected[j] mod p),
    e_j   = (x_j - m_j Delta) mod Q,
    noise = max_j min(e_j, Q - e_j).
`bfv_noise_inf_u64` restates the reference's own u64 steps (paper_repro.rs:249-281), which exist for one
ciphertext prime only; the two agree there (tests/test_noise_ref.py).
"""

from __future__ import annotations

import math

from oracle.ring import crt_exact

U64 = (1 << 64) - 1


def phase_coeffs(ct, sk) -> list[int]:
    """x_j in [0, Q): the phase of oracle.bfv.decrypt (encrypt.rs:115-123), exact CRT."""
    phase = ct.c[0].clone()
    s_pow = sk.poly.clone()
    for i in range(1, len(ct.c)):
        phase = phase.add(ct.c[i].mul(s_pow))
        if i < len(ct.c) - 1:
            s_pow = s_pow.mul(sk.poly)
    return crt_exact(phase.limb_coeffs(), ct.params.ct_basis)


def decrypt_coeffs(xs, moduli, p) -> list[int]:
    Q = math.prod(moduli)
    return [((x * p + (Q >> 1)) // Q) % p for x in xs]


def noise_of_phase(xs, moduli, p, expected=None) -> int:
    """The definition, on phase coefficients x_j in [0, Q)."""
    Q = math.prod(moduli)
    delta = Q // p
    ms = decrypt_coeffs(xs, moduli, p) if expected is None else [int(v) % p for v in expected]
    worst = 0
    for x, m in zip(xs, ms):
        e = (x - m * delta) % Q
        worst = max(worst, min(e, Q - e))
    return worst


def bfv_noise(ct, sk, expected=None) -> int:
    prm = ct.params
    return noise_of_phase(phase_coeffs(ct, sk), prm.ct_basis.moduli, prm.plain_modulus, expected)


def dbfv_noise(limbs, sk) -> int:
    """max_limb_noise (paper_repro.rs:238-247) over oracle BfvCiphertext limbs."""
    return max(bfv_noise(l, sk) for l in limbs)


def bfv_noise_inf_u64(phase_coeffs_q, pt_coeffs, q: int, t: int) -> int:
    """paper_repro.rs:249-281 step by step in (checked) u64 / u128 arithmetic: phase_coeffs_q = the phase's
    coefficients mod q = moduli[0], pt_coeffs = bfv_decrypt's output."""
    delta = q // t
    max_abs = 0
    for x, m in zip(phase_coeffs_q, pt_coeffs):
        prod = m * delta
        assert prod < (1 << 128)
        target = prod % q
        raw = x - target if x >= target else x + q - target
        assert 0 <= raw <= U64
        centered = min(raw, q - raw)
        if centered > max_abs:
            max_abs = centered
    return max_abs


def noise_budget_bits(noise: int, moduli, p: int) -> int:
    half_delta = (math.prod(moduli) // p) // 2
    return max(0, half_delta.bit_length() - noise.bit_length())

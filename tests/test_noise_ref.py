"""The noise definition of exacto_bfv_noise / exacto_dbfv_noise, on the CPU.

tests/noise_ref.py states it twice: over the full Q in big integers, and as the reference's u64 steps
(paper_repro.rs:249-281) for one ciphertext prime.  Here the two are compared, the big-integer form is
checked against closed forms on trivial ciphertexts (c1 = 0, so the phase is c0), and the binding's
noise_budget_bits and symbol list are checked.
"""
import math
import os
import random
import re

import pytest

from oracle import bfv as obfv, params as P
from oracle.ring import CoeffPoly, RnsPoly
from exacto_amd import _ffi
import noise_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["exacto_bfv_noise", "exacto_bfv_noise_dev", "exacto_dbfv_noise", "exacto_dbfv_noise_dev"]


def _trivial(xs, prm):
    """(c0, c1) = (x, 0): the phase is x whatever the key."""
    basis = prm.ct_basis
    c0 = RnsPoly.from_coeff_poly(CoeffPoly([x % basis.product() for x in xs], basis.product()), basis)
    return obfv.BfvCiphertext([c0, RnsPoly.zero(basis)], prm)


def test_two_restatements_agree_at_compact_bfv():
    prm = P.compact_bfv()
    q, t = prm.ct_basis.moduli[0], prm.plain_modulus
    r = random.Random(31)
    sk = obfv.gen_secret_key(prm, r)
    cts = [obfv.encrypt_sk(obfv.encode_scalar(m, prm), sk, r) for m in (0, 5, t - 1)]
    # random ciphertexts: uniform residues in both components (already NTT-domain values)
    basis = prm.ct_basis
    for _ in range(2):
        comps = [RnsPoly.from_limb_coeffs([[r.randrange(q) for _ in range(prm.ring_degree)]], basis)
                 for _ in range(2)]
        cts.append(obfv.BfvCiphertext(comps, prm))
    for i, ct in enumerate(cts):
        xs = noise_ref.phase_coeffs(ct, sk)
        pt = obfv.decrypt(ct, sk).coeffs
        lit = noise_ref.bfv_noise_inf_u64(xs, pt, q, t)
        assert lit == noise_ref.noise_of_phase(xs, [q], t) == noise_ref.bfv_noise(ct, sk), i
        if i < 3:
            assert 0 < lit < 64, "a fresh encryption's noise is a few sigma"
        else:
            assert lit > (q // t) // 8, "a uniform phase leaves a residual of Delta's size"


@pytest.mark.parametrize("which", ["cfg3_n16", "compact"])
def test_trivial_ciphertexts_closed_form(which):
    prm = P.cfg3_params(16) if which == "cfg3_n16" else P.compact_bfv()
    moduli, p, n = prm.ct_basis.moduli, prm.plain_modulus, prm.ring_degree
    Q = math.prod(moduli)
    delta = Q // p
    sk = obfv.gen_secret_key(prm, random.Random(2))
    ks = [0, 1, -1, delta // 2 - 1, -(delta // 2 - 1)]
    if Q > 1 << 70:
        ks += [(1 << 64) - 1, -((1 << 64) - 1), 1 << 64, -(1 << 64)]
    for k in ks:
        # Q = p Delta + rho moves the rounding boundaries of m by m rho / p < p: a residual within p of
        # Delta / 2 decrypts to m only for small m
        for m in ((0, 1) if abs(k) == delta // 2 - 1 else (0, 1, p - 1)):
            xs = [delta * m] * n
            xs[n // 3] = delta * m + k
            ct = _trivial(xs, prm)
            assert noise_ref.bfv_noise(ct, sk) == abs(k), (k, m)
            assert obfv.decrypt(ct, sk).coeffs == [m] * n
            assert _ffi.noise_budget_bits(abs(k), moduli, p) == noise_ref.noise_budget_bits(abs(k), moduli, p) \
                == max(0, (delta // 2).bit_length() - abs(k).bit_length())
    # x = Q - 1: the rounding gives r = p, so m = 0 and the residual is -1
    xs = [0] * n
    xs[n - 1] = Q - 1
    ct = _trivial(xs, prm)
    assert obfv.decrypt(ct, sk).coeffs == [0] * n
    assert noise_ref.bfv_noise(ct, sk) == 1
    # with `expected`: residuals either side of Q / 2
    exp = [3] * n
    for e in (Q // 2, Q // 2 + 1):
        xs = [delta * 3] * n
        xs[1] = (delta * 3 + e) % Q
        assert noise_ref.bfv_noise(_trivial(xs, prm), sk, expected=exp) == Q // 2
    assert _ffi.noise_budget_bits(Q // 2, moduli, p) == 0
    assert _ffi.noise_budget_bits(0, moduli, p) == (delta // 2).bit_length()
    assert _ffi.noise_budget_bits(delta // 2, moduli, p) == 0
    assert _ffi.noise_budget_bits(delta // 4, moduli, p) == 1


def test_noise_symbols_are_declared_and_bound():
    with open(os.path.join(ROOT, "include", "exacto_hip.h")) as f:
        hdr = f.read()
    for s in SYMBOLS:
        assert s in _ffi.EXPORTED_SYMBOLS, s
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), s
    assert hasattr(_ffi.HipContext, "bfv_noise") and hasattr(_ffi.HipContext, "dbfv_noise")
    assert hasattr(_ffi.HipContext, "bfv_noise_dev") and hasattr(_ffi.HipContext, "dbfv_noise_dev")

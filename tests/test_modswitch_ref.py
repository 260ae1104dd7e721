"""Modulus switching (exacto_bfv_mod_switch), on the CPU: the definition of tests/modswitch_ref.py.

The rounding identity (division form == (x - delta) / q == the per-limb formula), the reference mode
against a line-by-line restatement of modswitch.rs:49-80, the noise bound of one exact drop on oracle
ciphertexts, the binding's symbols and argument checks, and what the GPU tests' boundary inputs tell apart.
"""
import inspect
import os
import random
import re

import numpy as np
import pytest

from oracle import bfv as obfv, params as P
from oracle.ring import CoeffPoly, NttPoly, RnsBasis, RnsPoly
from exacto_amd import _ffi
from exacto_amd._ffi import HipContext
import modswitch_ref as M
import noise_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["exacto_bfv_mod_switch", "exacto_bfv_mod_switch_dev"]


# ------------------------------------------------------------------ rounding identity

@pytest.mark.parametrize("moduli", [[13, 17], [17, 13], [11, 13, 17], [3, 257]])
def test_rounding_identity_exhaustive_toy(moduli):
    q = moduli[-1]
    Qp = M.product(moduli[:-1])
    invs = [pow(q % qi, -1, qi) for qi in moduli[:-1]]
    zeros = 0
    for x in range(Qp * q):
        d = M.centred(x, q)
        assert -(q - 1) // 2 <= d <= (q - 1) // 2 and (x - d) % q == 0
        y = M.round_div(x, q, Qp)
        assert y == ((x - d) // q) % Qp
        assert abs(2 * ((x - d) // q) * q - 2 * x) < q   # (x - d) / q is the nearest integer: |d| < q / 2
        for qi, inv in zip(moduli[:-1], invs):
            assert y % qi == (x % qi - d) * inv % qi
        (got,) = zip(*M.drop_limbs([[x % m] for m in moduli], moduli, "round"))
        assert [y % qi for qi in moduli[:-1]] == list(got)
        zeros += y == 0 and x > Qp * q // 2
    assert zeros == (q - 1) // 2, "the top (q - 1) / 2 values wrap to 0"


def test_rounding_identity_boundaries_cfg3():
    moduli = P.Q3
    q, Qp = moduli[-1], M.product(moduli[:-1])
    Q = Qp * q
    xs, _ = M.boundary_values(moduli, 64, random.Random(1))
    assert Q - (q + 1) // 2 in xs and Q - (q - 1) // 2 in xs and Q - 1 in xs and 0 in xs
    xs = (xs + [0] * 16)[:len(xs) // 16 * 16 + 16]
    for k in range(0, len(xs), 16):
        part = xs[k:k + 16]
        want = [M.round_div(x, q, Qp) for x in part]
        assert want == [((x - M.centred(x, q)) // q) % Qp for x in part]
        assert M.drop_crt(part, moduli, "round") == want
    assert M.round_div(Q - (q + 1) // 2, q, Qp) == Qp - 1
    assert M.round_div(Q - (q - 1) // 2, q, Qp) == 0 == M.round_div(Q - 1, q, Qp)


# ------------------------------------------------------------------ reference mode

def _drop_last_rns_prime(poly: RnsPoly, basis: RnsBasis) -> RnsPoly:
    """modswitch.rs:37-87, statement by statement."""
    num_primes = poly.num_components()
    last_idx = num_primes - 1
    last_coeffs = poly.components[last_idx].to_coeff_poly()
    new_components = []
    for i in range(last_idx):
        qi = basis.moduli[i]
        last_mod_qi = [c % qi for c in last_coeffs.coeffs]
        ci_coeffs = poly.components[i].to_coeff_poly()
        new_coeffs = []
        for j, c in enumerate(ci_coeffs.coeffs):
            diff = c - last_mod_qi[j] if c >= last_mod_qi[j] else qi - last_mod_qi[j] + c
            new_coeffs.append(diff)
        new_components.append(NttPoly.from_coeff_poly(CoeffPoly(new_coeffs, qi), basis.plans[i]))
    return RnsPoly(new_components, poly.ring_degree)


@pytest.mark.parametrize("moduli", [P.Q3, [1099509805057, 562949953443841], [562949953443841, 1099509805057]])
def test_reference_mode_is_the_reference_function(moduli):
    n = 16
    basis = RnsBasis(list(moduli), n)
    r = random.Random(4)
    for _ in range(3):
        poly = RnsPoly.from_limb_coeffs([[r.randrange(q) for _ in range(n)] for q in moduli], basis)
        want = _drop_last_rns_prime(poly, basis)
        got = M.drop_limbs(poly.limb_coeffs(), moduli, "reference")
        assert got == want.limb_coeffs()
        ct = np.array([c.evals for c in poly.components], dtype=np.uint64)
        assert np.array_equal(M.drop_np(ct, moduli, n, "reference"),
                              np.array([c.evals for c in want.components], dtype=np.uint64))
        assert got != M.drop_limbs(poly.limb_coeffs(), moduli, "round")


def test_several_drops_are_single_drops():
    n, moduli = 16, P.Q4
    rng = np.random.default_rng(3)
    ct = np.stack([rng.integers(0, q, size=(2, n), dtype=np.uint64) for q in moduli], axis=1)
    for mode in M.MODES:
        one = M.drop_np(ct, moduli, n, mode)
        two = M.drop_np(one, moduli[:3], n, mode)
        assert np.array_equal(M.drop_np(ct, moduli, n, mode, drops=2), two)
        assert np.array_equal(M.drop_np(ct, moduli, n, mode, drops=3), M.drop_np(two, moduli[:2], n, mode))


# ------------------------------------------------------------------ noise bound

@pytest.mark.parametrize("n", [16, 64])
def test_noise_after_one_exact_drop(n):
    prm = P.cfg3_params(n)
    moduli, p = prm.ct_basis.moduli, prm.plain_modulus
    q = moduli[-1]
    r = random.Random(100 + n)
    sk = obfv.gen_secret_key(prm, r)
    lower = M.lower_params(prm)
    sk_lo = M.lower_key(sk, lower)
    assert lower.ct_basis.moduli == moduli[:-1]

    def check(ct, want_pt, what):
        before = noise_ref.bfv_noise(ct, sk, expected=want_pt)
        out = M.drop_ct(ct, "round")
        assert len(out.c[0].components) == len(moduli) - 1
        assert obfv.decrypt(out, sk_lo).coeffs == want_pt, what
        after = noise_ref.bfv_noise(out, sk_lo, expected=want_pt)
        print(f"n={n} {what}: noise {before} -> {after}, bound {M.noise_bound(before, q, p, n)}")
        assert after <= M.noise_bound(before, q, p, n), what
        # the reference's "simplified" form is not a ciphertext of the smaller modulus
        assert obfv.decrypt(M.drop_ct(ct, "reference"), sk_lo).coeffs != want_pt

    msgs = [[r.randrange(p) for _ in range(n)] for _ in range(3)] + [[p - 1] * n]
    cts = [obfv.encrypt_sk(CoeffPoly(m, p), sk, r) for m in msgs]
    for i, (m, ct) in enumerate(zip(msgs, cts)):
        check(ct, m, f"encryption {i}")
    rlk = obfv.gen_relin_key(sk, r)
    a, b = 12345 % p, 54321 % p
    prod = obfv.bfv_mul_and_relin(obfv.encrypt_sk(obfv.encode_scalar(a, prm), sk, r),
                                  obfv.encrypt_sk(obfv.encode_scalar(b, prm), sk, r), rlk)
    check(prod, [a * b % p] + [0] * (n - 1), "product")


# ------------------------------------------------------------------ bindings

def test_symbols_are_declared_and_bound():
    with open(os.path.join(ROOT, "include", "exacto_hip.h")) as f:
        hdr = f.read()
    sigs = dict((s[0], s[1]) for s in _ffi._SIGS)
    for s in SYMBOLS:
        assert s in _ffi.EXPORTED_SYMBOLS, s
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), s
        assert len(sigs[s]) == 8
    assert sigs[SYMBOLS[0]] == sigs[SYMBOLS[1]]
    assert re.search(r"enum\s+exacto_mod_switch_mode\s*\{\s*EXACTO_MODSWITCH_ROUND\s*=\s*0\s*,\s*"
                     r"EXACTO_MODSWITCH_REFERENCE\s*=\s*1\s*\}", hdr)
    assert list(inspect.signature(HipContext.bfv_mod_switch).parameters) == ["self", "ct", "limbs_out", "mode"]
    assert list(inspect.signature(HipContext.bfv_mod_switch_dev).parameters) == \
        ["self", "ct", "polys", "limbs_in", "limbs_out", "out", "batch", "mode"]
    assert HipContext.MOD_SWITCH_MODES == {"round": 0, "reference": 1}
    with open(os.path.join(ROOT, "exacto_amd", "csrc", "exacto_internal.hpp")) as f:
        assert "launch_drop_prime" in f.read()


class _NoLibrary:
    """Stands in for the loaded library: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the arguments were checked")


def _bare_context():
    ctx = object.__new__(HipContext)
    ctx._lib = _NoLibrary()
    ctx._h = None
    ctx.L, ctx.n = 3, 16
    return ctx


@pytest.mark.parametrize("shape, kw, text", [
    ((1, 2, 1, 16), {}, "only one modulus remaining"),
    ((1, 0, 3, 16), {}, "no polynomials"),
    ((1, 2, 3, 16), {"limbs_out": 3}, "limbs_out = 3"),
    ((1, 2, 3, 16), {"limbs_out": 0}, "limbs_out = 0"),
    ((1, 2, 3, 16), {"limbs_out": -1}, "limbs_out = -1"),
    ((1, 2, 3, 16), {"limbs_out": 1.5}, "limbs_out = 1.5"),
    ((1, 2, 3, 16), {"mode": "exact"}, "mode = 'exact'"),
    ((1, 2, 3, 16), {"mode": 0}, "mode = 0"),
    ((1, 2, 3, 32), {}, "rows of 32 coefficients"),
    ((2, 3, 16), {}, "[B][polys][limbs_in][n]"),
])
def test_malformed_arguments_rejected_before_the_library(shape, kw, text):
    ctx = _bare_context()
    with pytest.raises(ValueError) as e:
        ctx.bfv_mod_switch(np.zeros(shape, dtype=np.uint64), **kw)
    assert text in str(e.value)
    if len(shape) == 4 and shape[3] == 16:
        with pytest.raises(ValueError) as e:
            ctx.bfv_mod_switch_dev(None, shape[1], shape[2], kw.get("limbs_out", shape[2] - 1), None, shape[0],
                                   mode=kw.get("mode", "round"))
        assert text in str(e.value)


# ------------------------------------------------------------------ what the GPU tests' inputs tell apart

def test_boundary_inputs_separate_the_wrong_formulas():
    """tests/test_gpu_modswitch.py compares the device with drop_np on boundary_batch's inputs.  Three wrong
    kernels, restated here on the same inputs, must differ from the definition (so those tests fail on them):
    the uncentred remainder in the exact mode; the inverse of the context's last prime for a drop below the
    top; no re-reduction of delta before the forward transform where q is not near q_i."""
    n = 16
    for moduli in ([1099509805057, 562949953443841], [562949953443841, 1099509805057], [65537, 1099509805057], P.Q3):
        ct, xs = M.boundary_batch(moduli, n, 3, 3, seed=2)
        q = moduli[-1]
        rows = [[[x % m for x in poly] for m in moduli] for item in xs for poly in item]
        good = [M.drop_limbs(r, moduli, "round") for r in rows]
        uncentred = [[[(a - u) * pow(q % qi, -1, qi) % qi for a, u in zip(c, r[-1])]
                      for c, qi in zip(r[:-1], moduli[:-1])] for r in rows]
        assert all(g != u for g, u in zip(good, uncentred)), "every polynomial has a remainder above q / 2"
        # delta as the kernel holds it (two's complement, 64 bits) is not a residue mod q_i
        for r in rows:
            ds = [M.centred(u, q) for u in r[-1]]
            assert any(d < 0 for d in ds)
            if q > 2 * moduli[0]:
                assert any(abs(d) >= moduli[0] for d in ds)
    # level 2 of an L = 3 context: q_1^-1 mod q_0 is not q_2^-1 mod q_0
    q0, q1, q2 = P.Q3
    assert pow(q1, -1, q0) != pow(q2 % q0, -1, q0)

"""tests/hoist_ref.py (the whole-batch reference of the hoisted-rotation GPU tests) and the host-only table
builder exacto_galois_ntt_permutation, on the CPU: the permutation against the oracle's transform, the
library's table against the helper's at every ring degree, and the helper's rotations at n = 16 against the
Python oracle: the same decryption as bfv_apply_automorphism, other bits where a digit sits at -B/2."""

import os
import random

import numpy as np
import pytest

import hoist_ref
from exacto_amd import _ffi
from oracle import bfv as obfv, cref, params as P
from oracle.ring import CoeffPoly, NttPlan, RnsPoly
from bridge import ct_to_np, np_to_ct, np_to_rlk, rns_to_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _elements(n):
    return [1, 3, 5, 2 * n - 1, pow(3, n // 2 - 1, 2 * n), 4 * n + 3]


def _sigma_coeffs(a, k, q):
    n = len(a)
    res = [0] * n
    for i, c in enumerate(a):
        e = (i * k) % (2 * n)
        if e < n:
            res[e] = c
        else:
            res[e - n] = (-c) % q
    return res


@pytest.mark.parametrize("n,moduli", [(16, [65537, 1099509805057]), (64, P.Q3[:2]), (1024, P.Q3[:2])])
def test_permutation_against_oracle_transform(n, moduli):
    rng = random.Random(n)
    for q in moduli:
        plan = NttPlan(n, int(q))
        a = [rng.randrange(int(q)) for _ in range(n)]
        fa = list(a)
        plan.fwd(fa)
        for k in (3, 5, 2 * n - 1, pow(3, 7, 2 * n)):
            fs = _sigma_coeffs(a, k, int(q))
            plan.fwd(fs)
            perm = hoist_ref.ntt_permutation(n, k)
            assert sorted(perm.tolist()) == list(range(n))
            assert fs == [fa[p] for p in perm], (n, q, k)


@pytest.mark.parametrize("logn", range(4, 15))
def test_library_table_matches_helper(logn):
    n = 1 << logn
    for k in _elements(n):
        got = _ffi.galois_ntt_permutation(n, k)
        assert got.dtype == np.uint32 and np.array_equal(got, hoist_ref.ntt_permutation(n, k)), (n, k)


def test_table_errors():
    with pytest.raises(_ffi.ExactoError) as e:
        _ffi.galois_ntt_permutation(64, 6)
    assert e.value.variant == "InvalidParam" and "hoisted automorphisms require odd Galois elements" in str(e.value)
    with pytest.raises(_ffi.ExactoError) as e:
        _ffi.galois_ntt_permutation(48, 3)
    assert e.value.variant == "InvalidRingDegree"
    for n in (8, 32768):
        with pytest.raises(_ffi.ExactoError) as e:
            _ffi.galois_ntt_permutation(n, 3)
        assert e.value.variant in ("InvalidRingDegree", "InvalidParam")


def _multiprime16():
    return P.BfvParamsBuilder().ring_degree(16).plain_modulus(257).ct_moduli([65537, 1099509805057]) \
        .gadget_base(8).build()


def _gen_galois_key(sk, k, rng):
    """keygen.rs:171-209 with the oracle's sampler: gk_i = (-(a_i s + e_i) + base^i s(X^k), a_i).  s(X^k) from
    the signed coefficients (the reference lifts limb 0's residues, which at q_0 = 65537 is not s(X^k))."""
    prm = sk.params
    basis = prm.ct_basis
    n = prm.ring_degree
    sig = [0] * n
    for i, c in enumerate(sk.signed):
        e = (i * k) % (2 * n)
        sig[e % n] = c if e < n else -c
    g = obfv._signed_to_rns(sig, basis)
    keys = []
    for i in range(prm.gadget_digits):
        a = obfv._uniform_rns(rng, basis)
        e = obfv._signed_to_rns(obfv._gaussian(rng, prm.ring_degree, prm.sigma), basis)
        keys.append((a.mul(sk.poly).add(e).neg().add(g), a))
        g = g.scalar_mul(prm.gadget_base)
    return obfv.GaloisKey(keys, k, prm)


def _keys_np(gk):
    return np.stack([np.stack([rns_to_np(k0), rns_to_np(k1)]) for k0, k1 in gk.keys])


def test_same_plaintext_as_oracle_automorphism():
    assert cref.available(), "oracle/c/liboracle.so is not built: run build() of __graft_entry__.py"
    prm = _multiprime16()
    n, p = prm.ring_degree, prm.plain_modulus
    rng = random.Random(5)
    sk = obfv.gen_secret_key(prm, rng)
    elements = [3, 2 * n - 1]
    gks = [_gen_galois_key(sk, k, rng) for k in elements]
    pts = [CoeffPoly([rng.randrange(p) for _ in range(n)], p) for _ in range(3)]
    cts = [obfv.encrypt_sk(pt, sk, rng) for pt in pts]
    ct = np.stack([ct_to_np(c) for c in cts])
    got = hoist_ref.rotate_hoisted(prm, ct, elements, np.stack([_keys_np(g) for g in gks]))
    assert got.shape == (3, 2, 2, 2, n)
    for b in range(3):
        for r, k in enumerate(elements):
            want = obfv.bfv_apply_automorphism(cts[b], gks[r])
            want_pt = obfv.decrypt(want, sk).coeffs
            assert want_pt == obfv.apply_automorphism(pts[b], k).coeffs
            assert obfv.decrypt(np_to_ct(got[b, r], prm), sk).coeffs == want_pt, (b, k)


def test_not_the_bits_of_the_oracle_automorphism():
    """A coefficient of c1 equal to -B/2 = -4 has the digits (-4, 0, ...); sigma moves it to another index
    with the sign flipped, and the digits of +4 are (-4, 1, 0, ...): not minus the digits of -4."""
    assert cref.available()
    prm = _multiprime16()
    n, q = prm.ring_degree, [int(v) for v in prm.ct_basis.moduli]
    Q = q[0] * q[1]
    assert obfv.gadget_decompose_coeff(Q - 4, Q, 8, prm.gadget_digits)[:2] == [Q - 4, 0]
    assert obfv.gadget_decompose_coeff(4, Q, 8, prm.gadget_digits)[:2] == [Q - 4, 1]
    rng = np.random.default_rng(3)
    from bridge import uniform_residues
    c1 = [0] * n
    c1[1] = Q - 4                     # sigma_{2n-1}: X -> -X^(n-1), so this coefficient becomes +4
    basis = prm.ct_basis
    c0 = np_to_ct(uniform_residues(rng, (2,), q, n), prm).c[0]
    ct = obfv.BfvCiphertext([c0, RnsPoly.from_coeff_poly(CoeffPoly(c1, Q), basis)], prm)
    k = 2 * n - 1
    gk = uniform_residues(rng, (prm.gadget_digits, 2), q, n)
    want = ct_to_np(obfv.bfv_apply_automorphism(ct, obfv.GaloisKey(np_to_rlk(gk, prm).keys, k, prm)))
    got = hoist_ref.rotate_hoisted(prm, ct_to_np(ct)[None], [k], gk[None])[0, 0]
    assert not np.array_equal(got, want)


def test_linear_transform_is_the_sum_of_plain_products():
    assert cref.available()
    prm = _multiprime16()
    n, q = prm.ring_degree, [int(v) for v in prm.ct_basis.moduli]
    rng = np.random.default_rng(9)
    from bridge import uniform_residues
    hoisted = uniform_residues(rng, (2, 3, 2), q, n)
    pts = rng.integers(0, prm.plain_modulus, size=(3, n), dtype=np.uint64)
    got = hoist_ref.linear_transform(prm, hoisted, pts)
    for b in range(2):
        acc = None
        for r in range(3):
            term = obfv.bfv_plain_mul(np_to_ct(hoisted[b, r], prm), CoeffPoly([int(v) for v in pts[r]], prm.plain_modulus))
            acc = term if acc is None else obfv.bfv_add(acc, term)
        assert np.array_equal(got[b], ct_to_np(acc))


NEW_SYMBOLS = ["exacto_galois_ntt_permutation", "exacto_galois_keyset_create", "exacto_galois_keyset_create_dev",
               "exacto_galois_keyset_destroy", "exacto_galois_keyset_info", "exacto_bfv_rotate_hoisted",
               "exacto_bfv_rotate_hoisted_dev", "exacto_bfv_linear_transform", "exacto_bfv_linear_transform_dev"]


def test_symbols_exported_and_bound():
    lib = _ffi.load()
    with open(os.path.join(ROOT, "include", "exacto_hip.rs")) as f:
        rs = f.read()
    with open(os.path.join(ROOT, "include", "exacto_hip.h")) as f:
        hdr = f.read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _ffi.EXPORTED_SYMBOLS
        assert f"pub fn {name}(" in rs, name
        assert f"{name}(" in hdr, name
    assert "pub struct ExactoGaloisKeyset" in rs

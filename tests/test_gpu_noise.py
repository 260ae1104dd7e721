"""Noise measurement on the GPU: exacto_bfv_noise / exacto_dbfv_noise (csrc/noise.hip).

Reference: paper_repro.rs:238-281 (max_limb_noise, bfv_noise_inf), restated over the full Q in
tests/noise_ref.py.  Every comparison is bit-exact.

Trivial ciphertexts (c1 = 0) make the phase equal to c0, so every coefficient is an independent lane of
the kernel and a residual can be placed at a chosen coefficient: c0_j = Delta m_j + k_j has residual k_j
as long as |k_j| stays clear of Delta / 2.
"""
import math
import os
import random
import re
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import bfv as obfv, params as P
from exacto_amd._ffi import HipContext, ExactoError, noise_budget_bits
from bridge import ct_to_np, np_to_ct, np_to_rns, rlk_to_np, rns_to_np, uniform_residues
from worstcase import to_ntt
import fp_boundary
import noise_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = [0x0123456789ABCDEF, 0x0FEDCBA987654321, 0x1111111122222222, 0x3333333344444444]
GENERIC2 = [1099509805057, 562949953443841]


def _launch_shape():
    """(threads per workgroup, coefficients per workgroup) of noise_kernel, read from the code under test."""
    with open(os.path.join(ROOT, "exacto_amd", "csrc", "noise.hip")) as f:
        src = f.read()
    tpb = int(re.search(r"NOISE_TPB = (\d+);", src).group(1))
    cpt = int(re.search(r"NOISE_CPT = (\d+);", src).group(1))
    assert re.search(r"NOISE_CHUNK = NOISE_TPB \* NOISE_CPT;", src)
    return tpb, tpb * cpt


def _generic2_params():
    return P.BfvParamsBuilder().ring_degree(1024).plain_modulus(257).ct_moduli(GENERIC2).build()


def _oracle_sk(sk_np, prm):
    return SimpleNamespace(poly=np_to_rns(sk_np, prm.ct_basis), params=prm)


def _setup(prm, seed):
    r = random.Random(seed)
    sk = obfv.gen_secret_key(prm, r)
    return HipContext.from_params(prm), sk, rns_to_np(sk.poly), r


def _trivial(xs_list, prm):
    """Phase coefficient vectors -> [B][2][L][n] with c1 = 0."""
    moduli, n = prm.ct_basis.moduli, prm.ring_degree
    out = np.zeros((len(xs_list), 2, len(moduli), n), dtype=np.uint64)
    for b, xs in enumerate(xs_list):
        out[b, 0] = to_ntt(xs, moduli, n)
    return out


def _some_sk(prm, seed=1):
    # c1 = 0: the key does not enter the phase; a uniform one exercises the product with zero all the same
    return uniform_residues(np.random.default_rng(seed), (), prm.ct_basis.moduli, prm.ring_degree)


# ------------------------------------------------------------------ argmax placement

@pytest.mark.parametrize("which", ["cfg3_n16", "cfg3_n64", "cfg3_n256", "cfg3_n1024", "compact"])
def test_argmax_placement(gpu_available, which):
    prm = P.compact_bfv() if which == "compact" else P.cfg3_params(int(which.split("_n")[1]))
    moduli, p, n = prm.ct_basis.moduli, prm.plain_modulus, prm.ring_degree
    L = len(moduli)
    Q = math.prod(moduli)
    delta = Q // p
    # noise_kernel: NOISE_TPB = 256 threads, NOISE_CHUNK = 512 coefficients per workgroup, a thread takes
    # coefficients t and t + 256 of its chunk; workgroup boundaries are the multiples of the chunk
    tpb, chunk = _launch_shape()
    pos = {0, n - 1, 63, 64, tpb - 1, tpb, (n // 2 + 5) % n, n // 3}
    for b in range(chunk, n, chunk):
        pos |= {b - 1, b}
    pos = sorted(j for j in pos if j < n)
    # the large residual: a quarter of Delta, every word live, clear of the rounding boundary for every m
    K = (delta // 4) | 1
    top = 1 << (64 * (L - 1)) if L > 1 else 1 << 20
    fillers = {"one_less": K - 1, "tie": K, "top_word": K - top, "bottom_word": K - 0x12345,
               "top_digit": K - math.prod(moduli[:-1]), "small": 7}
    if L > 1:
        # the kernel compares mixed-radix digits (digit i is mod q_i, the top one first): values below K whose
        # lower digits are above K's, so that a comparison starting from the low digit picks them
        U = math.prod(moduli[:-1])
        assert K % moduli[0] + 1 < moduli[0] and K > 2 * U
        fillers["low_digit_up"] = K - U + 1
        fillers["mid_digit_up"] = K - U + moduli[0] * (L > 2)
        fillers["all_low_digits_max"] = (K // U) * U - 1
    ms = [(j * 2654435761) % p for j in range(n)]
    cases, xs_list, want = [], [], []
    for j0 in pos:
        for name, f in fillers.items():
            for sign in (1, -1):
                # the large residual with `sign`; the others alternate sign coefficient by coefficient
                ks = [f if (j & 1) else -f for j in range(n)]
                ks[j0] = sign * K
                xs = [(delta * m + k) % Q for m, k in zip(ms, ks)]
                cases.append((j0, name, sign))
                xs_list.append(xs)
                want.append(K)
    xs_list.append([delta * m for m in ms])   # no noise at all
    cases.append(("zero", "", 0))
    want.append(0)
    # the closed form is what the big-integer definition gives (checked on a sample: it is the slow part)
    for i in (0, len(xs_list) // 2, len(xs_list) - 1):
        assert noise_ref.noise_of_phase(xs_list[i], moduli, p) == want[i], cases[i]
    ctx = HipContext.from_params(prm)
    got, plain = ctx.bfv_noise(_trivial(xs_list, prm), _some_sk(prm), return_plain=True)
    bad = [(c, hex(g)) for c, g, w in zip(cases, got, want) if g != w]
    assert not bad, (which, hex(K), bad[:6], len(bad))
    assert all([int(v) for v in row] == ms for row in plain)


# ------------------------------------------------------------------ item isolation

def test_items_do_not_see_each_other(gpu_available):
    prm = P.cfg3_params(1024)
    moduli, p, n = prm.ct_basis.moduli, prm.plain_modulus, prm.ring_degree
    Q = math.prod(moduli)
    delta = Q // p
    ctx = HipContext.from_params(prm)
    sk = _some_sk(prm)
    noises = [(1 << 160) + 12345, 5, (1 << 70) + 1]
    assert noises[0] < delta // 4
    for order in (noises, noises[::-1]):
        xs_list = []
        for b, k in enumerate(order):
            xs = [delta * (j % p) for j in range(n)]
            j0 = (300 * b + 700) % n
            xs[j0] = (xs[j0] - k) % Q
            xs_list.append(xs)
        assert ctx.bfv_noise(_trivial(xs_list, prm), sk) == list(order)


@pytest.mark.parametrize("d", [2, 8])
def test_dbfv_limb_maximum_and_isolation(gpu_available, d):
    prm = P.cfg3_params(1024)
    moduli, p, n = prm.ct_basis.moduli, prm.plain_modulus, prm.ring_degree
    Q = math.prod(moduli)
    delta = Q // p
    ctx = HipContext.from_params(prm)
    sk = _some_sk(prm)
    B = 3
    big = [(1 << 150) + 3, (1 << 66) + 1, (1 << 129) + 77]   # item b's maximum
    cache = {}

    def limb(k, j0):
        if (k, j0) not in cache:
            xs = [delta * ((3 * j) % p) for j in range(n)]
            xs[j0] = (xs[j0] + k) % Q
            c = np.zeros((2, len(moduli), n), dtype=np.uint64)
            c[0] = to_ntt(xs, moduli, n)
            cache[(k, j0)] = c
        return cache[(k, j0)]

    for l0 in range(d):
        ct = np.zeros((B, d, 2, len(moduli), n), dtype=np.uint64)
        for b in range(B):
            where = (l0 + b) % d      # neighbouring items carry their maximum in different limbs
            for l in range(d):
                # every other limb: one unit below the item's maximum, or tiny, at the far end of the row
                k = big[b] if l == where else (big[b] - 1 if (l + b) % 2 else 9)
                ct[b, l] = limb(-k if l % 2 else k, n - 1 if l == where else 600)
        assert ctx.dbfv_noise(d, ct, sk) == big, (d, l0)
        # per limb: the BFV form with batch B * d on the same memory
        per = ctx.bfv_noise(ct.reshape(B * d, 2, len(moduli), n), sk)
        assert [max(per[b * d:(b + 1) * d]) for b in range(B)] == big


# ------------------------------------------------------------------ uniform ciphertexts

UNIFORM = {
    "compact": (P.compact_bfv, 2),
    "small": (P.small_bfv, 1),
    "cfg3_n1024": (lambda: P.cfg3_params(1024), 2),
    "cfg3": (P.cfg3_params, 1),
    "cfg5": (lambda: P.cfg5_params().bfv_params, 2),
    "generic2": (_generic2_params, 2),
    "low_L2": (lambda: fp_boundary.low_params(1024, 2, 65537), 2),
    "low_L5": (lambda: fp_boundary.low_params(1024, 5, 65537), 2),
    "low_L6": (lambda: fp_boundary.low_params(1024, 6, 65537), 1),
}


@pytest.mark.parametrize("which", list(UNIFORM))
def test_uniform_ciphertexts_match_reference(gpu_available, which):
    make, B = UNIFORM[which]
    prm = make()
    ctx, sk, sk_np, _ = _setup(prm, 3)
    rng = np.random.default_rng(5)
    n, moduli, p = prm.ring_degree, prm.ct_basis.moduli, prm.plain_modulus
    half_delta = (math.prod(moduli) // p) // 2
    for polys, b in ((2, B), (3, 1)):
        ct = uniform_residues(rng, (b, polys), moduli, n)
        got, plain = ctx.bfv_noise(ct, sk_np, return_plain=True)
        assert got == ctx.bfv_noise(ct, sk_np)
        assert np.array_equal(plain, ctx.bfv_decrypt(ct, sk_np))
        for i in range(b):
            want = noise_ref.bfv_noise(np_to_ct(ct[i], prm), sk)
            assert got[i] == want, (which, polys, i, hex(got[i]), hex(want))
            # a uniform phase: the residual fills floor(Q / 2p), every word of the result is live
            assert got[i].bit_length() >= half_delta.bit_length() - 3


# ------------------------------------------------------------------ the `expected` form

@pytest.mark.parametrize("which", ["compact", "cfg3_n1024", "generic2"])
def test_expected_uniform(gpu_available, which):
    prm = UNIFORM[which][0]()
    ctx, sk, sk_np, _ = _setup(prm, 7)
    rng = np.random.default_rng(9)
    n, moduli, p = prm.ring_degree, prm.ct_basis.moduli, prm.plain_modulus
    ct = uniform_residues(rng, (2, 2), moduli, n)
    exp = rng.integers(0, 1 << 63, size=(2, n), dtype=np.uint64) * np.uint64(2) + np.uint64(1)  # any u64: taken mod p
    got, plain = ctx.bfv_noise(ct, sk_np, expected=exp, return_plain=True)
    assert got == ctx.bfv_noise(ct, sk_np, expected=exp)
    assert np.array_equal(plain, ctx.bfv_decrypt(ct, sk_np))
    Q = math.prod(moduli)
    for i in range(2):
        want = noise_ref.bfv_noise(np_to_ct(ct[i], prm), sk, expected=[int(v) for v in exp[i]])
        assert got[i] == want
        assert got[i] > Q // 4, "residuals against an unrelated plaintext reach Q / 2"


@pytest.mark.parametrize("which", ["cfg3_n64", "compact", "generic2"])
def test_expected_crafted_around_half_q(gpu_available, which):
    prm = P.cfg3_params(64) if which == "cfg3_n64" else UNIFORM[which][0]()
    moduli, p, n = prm.ct_basis.moduli, prm.plain_modulus, prm.ring_degree
    Q = math.prod(moduli)
    delta = Q // p
    h = Q // 2
    ctx = HipContext.from_params(prm)
    exp = [(5 * j + 1) % p for j in range(n)]
    es = [h - 1, h, h + 1, Q - 1, 0]
    want = [h - 1, h, h, 1, 0]
    xs_list = []
    for t, e in enumerate(es):
        xs = [delta * m % Q for m in exp]
        j0 = (17 * t + 3) % n
        xs[j0] = (xs[j0] + e) % Q
        xs_list.append(xs)
    for xs, w in zip(xs_list, want):
        assert noise_ref.noise_of_phase(xs, moduli, p, expected=exp) == w
    ct = _trivial(xs_list, prm)
    e_np = np.array([exp] * len(es), dtype=np.uint64)
    sk = _some_sk(prm)
    assert ctx.bfv_noise(ct, sk, expected=e_np) == want
    got, plain = ctx.bfv_noise(ct, sk, expected=e_np, return_plain=True)
    assert got == want
    assert np.array_equal(plain, ctx.bfv_decrypt(ct, sk))


# ------------------------------------------------------------------ genuine encryptions and products

@pytest.mark.parametrize("which", ["compact", "cfg3_n1024"])
def test_genuine_encryptions_and_products(gpu_available, which):
    prm = UNIFORM[which][0]()
    ctx, sk, sk_np, r = _setup(prm, 9)
    moduli, p = prm.ct_basis.moduli, prm.plain_modulus
    ctx.load_relin_key(rlk_to_np(obfv.gen_relin_key(sk, r)))
    msgs = [(3, 7), (p - 1, 2)]
    c1 = np.stack([ct_to_np(obfv.encrypt_sk(obfv.encode_scalar(a, prm), sk, r)) for a, _ in msgs])
    c2 = np.stack([ct_to_np(obfv.encrypt_sk(obfv.encode_scalar(b, prm), sk, r)) for _, b in msgs])
    fresh = ctx.bfv_noise(np.concatenate([c1, c2]), sk_np)
    for i, ct in enumerate(np.concatenate([c1, c2])):
        assert fresh[i] == noise_ref.bfv_noise(np_to_ct(ct, prm), sk)
        assert 0 < fresh[i] < 64
        assert noise_budget_bits(fresh[i], moduli, p) > 0
    for prod in (ctx.bfv_mul_and_relin(c1, c2), ctx.bfv_mul_no_relin(c1, c2)):
        got = ctx.bfv_noise(prod, sk_np)
        for i in range(len(msgs)):
            assert got[i] == noise_ref.bfv_noise(np_to_ct(prod[i], prm), sk), (which, prod.shape[1], i)
            assert got[i] > max(fresh[i], fresh[i + len(msgs)])
        assert [int(v[0]) for v in ctx.bfv_decrypt(prod, sk_np)] == [(a * b) % p for a, b in msgs]


@pytest.mark.parametrize("which", ["compact_dbfv", "u64_dbfv"])
def test_dbfv_mul_noise(gpu_available, which):
    dp = P.compact_dbfv() if which == "compact_dbfv" else P.u64_dbfv()
    prm = dp.bfv_params
    moduli, t = prm.ct_basis.moduli, prm.plain_modulus
    d, args = dp.num_digits, (dp.num_digits, dp.base, dp.plain_modulus)
    ctx = HipContext.from_params(prm)
    sk_np = ctx.gen_secret_key(KEY, stream=1)
    ctx.gen_relin_key(sk_np, KEY, stream=2, resident=True)
    sk = _oracle_sk(sk_np, prm)
    B = 2 if which == "compact_dbfv" else 1
    mask = (1 << 64) - 1 if dp.plain_modulus == 0 else dp.plain_modulus - 1
    xs = [0x9E3779B97F4A7C15 & mask, 0xC2B2AE3D27D4EB4F & mask][:B]
    ys = [0x165667B19E3779F9 & mask, 0x27D4EB2F165667C5 & mask][:B]
    a = ctx.dbfv_encrypt_sk(*args, xs, sk_np, KEY, stream=3)
    b = ctx.dbfv_encrypt_sk(*args, ys, sk_np, KEY, stream=4)
    na, nb = ctx.dbfv_noise(d, a, sk_np), ctx.dbfv_noise(d, b, sk_np)
    out, _ = ctx.dbfv_mul(*args, a, b)
    no = ctx.dbfv_noise(d, out, sk_np)
    for i in range(B):
        assert na[i] == noise_ref.dbfv_noise([np_to_ct(l, prm) for l in a[i]], sk)
        assert no[i] == noise_ref.dbfv_noise([np_to_ct(l, prm) for l in out[i]], sk), which
        assert no[i] > max(na[i], nb[i]) > 0
        assert noise_budget_bits(na[i], moduli, t) > 0 and noise_budget_bits(nb[i], moduli, t) > 0
    # the per-limb values are the BFV form on the same memory
    per = ctx.bfv_noise(out.reshape(B * d, 2, len(moduli), prm.ring_degree), sk_np)
    assert [max(per[i * d:(i + 1) * d]) for i in range(B)] == no


# ------------------------------------------------------------------ forms and errors

def test_device_forms_equal_host_forms_and_repeat(gpu_available):
    import torch
    prm = P.cfg3_params(1024)
    ctx = HipContext.from_params(prm)
    rng = np.random.default_rng(13)
    n, moduli = prm.ring_degree, prm.ct_basis.moduli
    L, B, d = len(moduli), 4, 2
    sk_np = uniform_residues(rng, (), moduli, n)
    ct = uniform_residues(rng, (B, 2), moduli, n)
    exp = rng.integers(0, prm.plain_modulus, size=(B, n), dtype=np.uint64)
    want, want_plain = ctx.bfv_noise(ct, sk_np, return_plain=True)
    assert ctx.bfv_noise(ct, sk_np) == want, "two calls on the same input"
    want_exp = ctx.bfv_noise(ct, sk_np, expected=exp)
    want_d = ctx.dbfv_noise(d, ct.reshape(B // d, d, 2, L, n), sk_np)
    assert want_d == [max(want[0:2]), max(want[2:4])]

    dev = torch.device("cuda:0")
    to_dev = lambda a: torch.from_numpy(a.view(np.int64)).to(dev)
    words = lambda t: [sum(int(w) << (64 * k) for k, w in enumerate(row)) for row in t.cpu().numpy().view(np.uint64)]
    ct_d, sk_d, exp_d = to_dev(ct), to_dev(sk_np), to_dev(exp)
    for _ in range(2):
        out = torch.full((B, L), -1, dtype=torch.int64, device=dev)
        plain = torch.full((B, n), -1, dtype=torch.int64, device=dev)
        ctx.bfv_noise_dev(ct_d, 2, sk_d, out, B, plain_out=plain)
        ctx.synchronize()
        assert words(out) == want
        assert np.array_equal(plain.cpu().numpy().view(np.uint64), want_plain)
    out = torch.full((B, L), -1, dtype=torch.int64, device=dev)
    ctx.bfv_noise_dev(ct_d, 2, sk_d, out, B, expected=exp_d)
    ctx.synchronize()
    assert words(out) == want_exp
    out = torch.full((B // d, L), -1, dtype=torch.int64, device=dev)
    ctx.dbfv_noise_dev(d, ct_d, sk_d, out, B // d)
    ctx.synchronize()
    assert words(out) == want_d


def test_errors_and_empty_batch(gpu_available):
    prm = P.cfg3_params(64)
    ctx = HipContext.from_params(prm)
    n, L = prm.ring_degree, 3
    sk = np.zeros((L, n), dtype=np.uint64)
    with pytest.raises(ExactoError) as e:
        ctx.bfv_noise(np.zeros((1, 0, L, n), dtype=np.uint64), sk)
    assert e.value.variant == "InvalidParam"
    assert str(e.value) == "invalid parameter: ciphertext has no polynomials"
    with pytest.raises(ExactoError) as e2:
        ctx.bfv_decrypt(np.zeros((1, 0, L, n), dtype=np.uint64), sk)
    assert str(e2.value) == str(e.value) and e2.value.variant == e.value.variant
    with pytest.raises(ExactoError) as e:
        ctx.dbfv_noise(0, np.zeros((1, 0, 2, L, n), dtype=np.uint64), sk)
    assert e.value.variant == "InvalidParam"
    assert str(e.value) == "invalid parameter: num_digits must be >= 1"
    with pytest.raises(ExactoError) as e2:
        ctx.dbfv_decrypt(0, 16, 256, np.zeros((1, 0, 2, L, n), dtype=np.uint64), sk)
    assert str(e2.value) == str(e.value)
    assert ctx.bfv_noise(np.zeros((0, 2, L, n), dtype=np.uint64), sk) == []
    assert ctx.dbfv_noise(2, np.zeros((0, 2, 2, L, n), dtype=np.uint64), sk) == []


def test_plain_modulus_above_the_first_auxiliary_prime(gpu_available):
    # the rounding runs in the first internal auxiliary prime (below 2^60): with p above it, only the
    # form that needs no rounding (expected given, no plaintext output) is served
    p = (1 << 61) - 1
    prm = P.BfvParamsBuilder().ring_degree(64).plain_modulus(p).ct_moduli(P.Q3).build()
    ctx, sk, sk_np, _ = _setup(prm, 5)
    rng = np.random.default_rng(2)
    n, moduli = prm.ring_degree, prm.ct_basis.moduli
    ct = uniform_residues(rng, (2, 2), moduli, n)
    exp = rng.integers(0, 1 << 62, size=(2, n), dtype=np.uint64) * np.uint64(3)
    got = ctx.bfv_noise(ct, sk_np, expected=exp)
    for i in range(2):
        assert got[i] == noise_ref.bfv_noise(np_to_ct(ct[i], prm), sk, expected=[int(v) for v in exp[i]])
    for kw in ({}, {"expected": exp, "return_plain": True}):
        with pytest.raises(ExactoError) as e:
            ctx.bfv_noise(ct, sk_np, **kw)
        assert e.value.variant == "NotImplemented"
        assert "plain_modulus below the first internal auxiliary prime" in str(e.value)
    with pytest.raises(ExactoError) as e:
        ctx.bfv_decrypt(ct, sk_np)
    assert e.value.variant == "NotImplemented"

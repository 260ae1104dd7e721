"""Slot linear transforms on dBFV ciphertexts with wide diagonals, on the CPU (tests/dbfv_lt_ref.py).

  1. the slot identity at the plaintext level (n = 16, tests/dbfv_batch_ref.py): the sum over r of the limb
     products of encode(W_r) with sigma_{k_r}(encode(x)) decodes to sum_r W_r[s] x[rot_r(s)] mod p slot by slot;
  2. the bound on t for the parameters of the GPU decrypt-level tests (DECRYPT_SETS): the largest centred digit,
     R d (b - 1)^2 for the widest low limb plus the folded terms (DESIGN.md §4 for one product, times R), stays
     below t / 2, the all-extreme operands decode, and a batching prime just too small does not;
  2b. the worst-case noise of a transform under device-generated Galois keys decides which (n, set) the GPU
     decrypt-level test may use;
  3. the reference is the composition it claims to be (rotations limb by limb, then the product);
  4. the route a context takes (fused or staged) restated, for tests/test_gpu_dbfv_lt.py to hold against the
     library's report;
  5. the new symbols are exported, bound and declared.
"""

import os
import random

import numpy as np
import pytest

import batch_ref as R
import dbfv_batch_ref as D
import dbfv_lt_ref as LT
import dbfv_plain_ref as PR
import hoist_ref
from bridge import uniform_residues
from exacto_amd import _ffi
from oracle import params as P
from oracle.dbfv import small_reps
from oracle.ring import NttPlan, is_prime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = 1 << 64
P64 = U64 - 59

STEPS = [0, 1, 3]                       # the rotations of the decrypt-level tests: the identity and two keyed
# (t, base, d, p) of the GPU decrypt-level tests, R = len(STEPS); p = 0 is 2^64.  Both t are 1 mod 2048, so they
# batch at n = 16, 64 and 1024 alike, and the bound does not depend on n: every slot is a scalar of its own.
# 3127297 is the smallest such prime above 2 * 3 * 8 * 255^2 = 3121200: a transform multiplies the noise of the
# rotations by plaintext coefficients up to t and divides Delta by t, so the smallest t the digits allow
# leaves the most room for noise (the rotations' own noise is measured in DESIGN.md §4, "Hoisted rotations").
DECRYPT_SETS = [(12289, 16, 2, 256), (3127297, 256, 8, 0)]


def rotation_noise_bits(n: int) -> int:
    """noise_inf of a hoisted rotation under device-generated Galois keys over cfg3's primes, as DESIGN.md §4
    ("Hoisted rotations") records it: 124 bits at n = 64 and 130 at n = 4096, one bit per doubling of n."""
    return 124 + (n // 64).bit_length() - 1


def transform_noise_bits(n: int, t: int, d: int) -> int:
    """Worst case of the transform's noise in bits.  The identity's term carries fresh noise, which is nothing
    next to a keyed rotation's; a limb sums at most d digit pairs per keyed rotation, and a pair is a negacyclic
    product of n terms, a lifted diagonal coefficient below t times a noise coefficient of the rotated limb.
    Neither parameter set of DECRYPT_SETS folds."""
    keyed = sum(1 for k in STEPS if k % (n // 2))
    return (keyed * d * n * t).bit_length() + rotation_noise_bits(n)


def noise_fits(n: int, t: int, d: int) -> bool:
    """The worst case stays below Delta / 2 = floor(Q / t) / 2 over cfg3's primes."""
    Q = 1
    for q in P.Q3:
        Q *= int(q)
    return transform_noise_bits(n, t, d) < (Q // t // 2).bit_length()


# (n, t, base, d, p): the decrypt-level cases of the GPU tests are those whose noise fits as well; NOISE_BOUND
# holds what does not: p = 2^64 at n = 1024 (test_the_noise_bound_decides_the_decrypt_level_cases)
DECRYPT_CASES = [(n,) + s for n in (64, 1024) for s in DECRYPT_SETS if noise_fits(n, s[0], s[2])]
NOISE_BOUND = [(n,) + s for n in (64, 1024) for s in DECRYPT_SETS if not noise_fits(n, s[0], s[2])]

NEW_SYMBOLS = ["exacto_dbfv_rotate_hoisted", "exacto_dbfv_rotate_hoisted_dev", "exacto_dbfv_diagonals_create",
               "exacto_dbfv_diagonals_create_dev", "exacto_dbfv_diagonals_destroy", "exacto_dbfv_diagonals_info",
               "exacto_dbfv_linear_transform", "exacto_dbfv_linear_transform_dev",
               "exacto_dbfv_linear_transform_prepared", "exacto_dbfv_linear_transform_prepared_dev",
               "exacto_ctx_set_dbfv_lt_fused"]


def digit_bound(R_, base, d, p):
    """The largest digit a limb of reduce(sum_r W_r * rot_r(x)) can hold: wide limb m has min(m, 2d - 2 - m) + 1
    digit pairs per rotation, each at most (b - 1)^2, and limb i takes wide limb i plus rep[m - d][i] times
    every high limb m."""
    pairs = [min(m, 2 * d - 2 - m) + 1 for m in range(2 * d - 1)]
    wide = [R_ * c * (base - 1) ** 2 for c in pairs]
    reps = small_reps(base, d, p)
    return max(wide[i] + sum(abs(reps[m - d][i]) * wide[m] for m in range(d, 2 * d - 1)) for i in range(d))


def fused_route(n: int, L: int, gadget_base: int, d: int, fused_on: bool = False) -> bool:
    """The route of exacto_dbfv_linear_transform on a context with default switches: the staged route, unless
    exacto_ctx_set_dbfv_lt_fused(ctx, 1) turned the fused kernel on; even then the 31-bit key switch (exact RNS,
    so two primes at least, from n = 1024 on, 16-bit digits) and more than 8 digits stay on the staged route."""
    ks32 = L >= 2 and n >= 1024 and gadget_base <= 65536
    return fused_on and not ks32 and d <= 8


def plain_lt(x, W, steps, n, t, base, d, p):
    """sum_r encode(W_r) * sigma_{3^steps[r]}(encode(x)) on plaintexts [d][n], folded limb by limb."""
    px = D.encode(x, n, t, d, base, p)
    acc = [[0] * n for _ in range(d)]
    for w, k in zip(W, steps):
        rot = D.automorphism(px, pow(3, k, 2 * n), n, t)
        acc = D.limb_add(acc, D.limb_mul(D.encode(w, n, t, d, base, p), rot, n, t, d, base, p), t)
    return acc


def slotwise_lt(x, W, steps, n, p):
    m = D.modulus(p)
    rots = [R.rotate_rows(list(x), k, n) for k in steps]
    return [sum(w[s] * r[s] for w, r in zip(W, rots)) % m for s in range(n)]


def wide_operands(n, p, R_, seed):
    """x [n], W [R][n] below p, uniform, with slot 0 of every operand p - 1."""
    m = D.modulus(p)
    rng = random.Random(seed)
    x = [rng.randrange(m) for _ in range(n)]
    W = [[rng.randrange(m) for _ in range(n)] for _ in range(R_)]
    x[0] = m - 1
    for w in W:
        w[0] = m - 1
    return x, W


@pytest.mark.parametrize("t,base,d,p", DECRYPT_SETS + [(12289, 16, 2, 251), (1073750017, 256, 8, P64)])
def test_the_slot_identity_at_the_plaintext_level(t, base, d, p):
    n = 16
    steps = [0, 1, 3, n // 2 - 1, 1]          # the identity, a duplicate
    # as many of them as t holds (p = 251: the folded limb 0 reaches 1350 per rotation, four fit 12289 / 2;
    # 3127297 is sized for the three rotations of the decrypt-level tests)
    R_ = max(r for r in range(1, len(steps) + 1) if digit_bound(r, base, d, p) < t // 2)
    assert R_ >= 3
    steps = steps[:R_]
    x, W = wide_operands(n, p, R_, 5 + d)
    got = D.decode(plain_lt(x, W, steps, n, t, base, d, p), n, t, d, base, p)
    assert got == slotwise_lt(x, W, steps, n, p)


@pytest.mark.parametrize("t,base,d,p", DECRYPT_SETS)
def test_the_decrypt_level_parameters_hold_the_bound(t, base, d, p):
    """All-extreme operands (every slot of x and of every W_r is p - 1) reach the bound's digits."""
    m, R_ = D.modulus(p), len(STEPS)
    for n in (16, 64, 1024):
        assert NttPlan.try_new(n, t) is not None and t < 1 << 32
    assert base <= t and base ** d >= m
    assert digit_bound(R_, base, d, p) < t // 2
    n = 16
    x, W = [m - 1] * n, [[m - 1] * n for _ in range(R_)]
    acc = plain_lt(x, W, STEPS, n, t, base, d, p)
    centred = [c if c <= t // 2 else c - t for row in acc for c in R.decode(row, n, t)]
    assert max(abs(c) for c in centred) == digit_bound(R_, base, d, p)      # the bound is attained
    assert D.decode(acc, n, t, d, base, p) == slotwise_lt(x, W, STEPS, n, p)


@pytest.mark.parametrize("t,base,d,p", DECRYPT_SETS)
def test_the_reference_decrypts_at_the_decrypt_level_parameters(t, base, d, p):
    """Ciphertext level at n = 64 over cfg3's primes: the oracle's encryptions and Galois keys through
    dbfv_lt_ref decrypt to the slot-wise sums."""
    from oracle import bfv as obfv
    from oracle.ring import CoeffPoly
    from bridge import ct_to_np, np_to_ct
    from test_dbfv_batch_ref import oracle_params
    from test_hoist_ref import _gen_galois_key, _keys_np
    n = 64
    if p == 0:
        assert t == min(c for c in range(2 * digit_bound(len(STEPS), base, d, p) // 2048 * 2048 + 1, 1 << 23, 2048)
                        if c > 2 * digit_bound(len(STEPS), base, d, p) and is_prime(c))
    prm = oracle_params(n, t, base, d, p).bfv_params
    rng = random.Random(n + d)
    sk = obfv.gen_secret_key(prm, rng)
    elements = [pow(3, k, 2 * n) for k in STEPS]
    gks = np.stack([_keys_np(_gen_galois_key(sk, k, rng)) for k in elements])
    x, W = wide_operands(n, p, len(STEPS), 3)
    limbs = [obfv.encrypt_sk(CoeffPoly(row, t), sk, rng) for row in D.encode(x, n, t, d, base, p)]
    ct = np.stack([ct_to_np(limb) for limb in limbs])[None]
    pts = np.array([D.encode(w, n, t, d, base, p) for w in W], dtype=np.uint64)
    out = LT.linear_transform(prm, ct, elements, gks, pts, base, d, p)
    dec = [obfv.decrypt(np_to_ct(out[0, k], prm), sk).coeffs for k in range(d)]
    assert D.decode(dec, n, t, d, base, p) == slotwise_lt(x, W, STEPS, n, p)


def test_the_noise_bound_decides_the_decrypt_level_cases():
    """Device-generated Galois keys are far noisier than the oracle's (rotation_noise_bits), and a transform
    multiplies a rotation's noise by plaintext coefficients up to t while the budget Delta / 2 shrinks with t.
    p = 256 fits at both ring degrees and p = 2^64 at n = 64; at n = 1024 p = 2^64 does not: 3127297 is already
    the smallest batching prime its digits allow (test_the_reference_decrypts_at_the_decrypt_level_parameters),
    a larger t only adds noise and takes budget, so no t serves that case over cfg3's 180-bit Q."""
    assert rotation_noise_bits(64) == 124 and rotation_noise_bits(1024) == 128 and rotation_noise_bits(4096) == 130
    u64 = DECRYPT_SETS[1]
    assert DECRYPT_CASES == [(64,) + DECRYPT_SETS[0], (64,) + u64, (1024,) + DECRYPT_SETS[0]]
    assert NOISE_BOUND == [(1024,) + u64]
    assert (transform_noise_bits(64, 12289, 2), transform_noise_bits(64, 3127297, 8)) == (146, 156)
    assert (transform_noise_bits(1024, 12289, 2), transform_noise_bits(1024, 3127297, 8)) == (154, 164)
    Q = 1
    for q in P.Q3:
        Q *= int(q)
    assert ((Q // 12289 // 2).bit_length(), (Q // 3127297 // 2).bit_length()) == (166, 158)
    # both ring degrees and both p stay under test
    assert {c[0] for c in DECRYPT_CASES} == {64, 1024} and {c[4] for c in DECRYPT_CASES} == {256, 0}


def test_a_batching_prime_just_too_small_does_not_decode():
    """b = 16, d = 2, p = 256, three rotations: limb 1 reaches 3 * 2 * 15^2 = 1350.  t = 2689 is the largest
    batching prime of n = 16 below 2 * 1350, and 1350 > floor(2689 / 2) = 1344; 2753, the next one, decodes."""
    n, base, d, p, R_ = 16, 16, 2, 256, len(STEPS)
    assert digit_bound(R_, base, d, p) == 1350
    small, ok = 2689, 2753
    assert all(is_prime(t) and (t - 1) % (2 * n) == 0 for t in (small, ok))
    assert not any(is_prime(t) for t in range(small + 2 * n, ok, 2 * n))
    assert small // 2 < 1350 <= ok // 2
    x, W = [p - 1] * n, [[p - 1] * n for _ in range(R_)]
    want = slotwise_lt(x, W, STEPS, n, p)
    assert D.decode(plain_lt(x, W, STEPS, n, ok, base, d, p), n, ok, d, base, p) == want
    assert D.decode(plain_lt(x, W, STEPS, n, small, base, d, p), n, small, d, base, p) != want


def test_the_reference_is_the_composition():
    """dbfv_lt_ref rearranges hoist_ref's rotations of the limbs and hands them to dbfv_plain_ref."""
    n, base, d, p, B = 16, 16, 2, 251, 2
    prm = P.BfvParamsBuilder().ring_degree(n).plain_modulus(12289).ct_moduli(P.Q3).build()
    q = prm.ct_basis.moduli
    elements = [3, 1, 2 * n - 1]
    rng = np.random.default_rng(7)
    ct = uniform_residues(rng, (B, d, 2), q, n)
    gks = uniform_residues(rng, (len(elements), prm.gadget_digits, 2), q, n)
    pts = rng.integers(0, U64, size=(len(elements), d, n), dtype=np.uint64)
    rot = LT.rotate_hoisted(prm, ct, elements, gks)
    assert rot.shape == (B, len(elements), d, 2, len(q), n)
    H = hoist_ref.rotate_hoisted(prm, ct.reshape(B * d, 2, len(q), n), elements, gks)
    for b in range(B):
        for j in range(d):
            assert np.array_equal(rot[b, :, j], H[b * d + j])
    assert np.array_equal(rot[:, 1], ct)                                    # the identity element
    want = PR.mul_sum_direct(rot, pts[None], q, base, d, p)
    assert np.array_equal(LT.linear_transform(prm, ct, elements, gks, pts, base, d, p), want)
    assert np.array_equal(LT.linear_transform(prm, ct, elements, gks, pts, base, d, p, rotated=rot), want)


def test_the_route_restated():
    """The cases of tests/test_gpu_dbfv_lt.py, which asserts the library's report against this function."""
    on = dict(fused_on=True)
    assert fused_route(16, 3, 65536, 2, **on) and fused_route(64, 3, 65536, 8, **on) and fused_route(64, 1, 65536, 8, **on)
    assert fused_route(4096, 1, 65536, 8, **on)                 # the u64_dbfv preset: one prime, HPS
    assert not fused_route(1024, 3, 65536, 2, **on) and not fused_route(4096, 3, 65536, 8, **on)
    assert not fused_route(64, 3, 65536, D.min_digits(3, 10 ** 9 + 7), **on)    # more than 8 digits: the list kernel
    assert not fused_route(64, 3, 65536, 8) and not fused_route(4096, 1, 65536, 8)      # the default is staged


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
    assert "pub struct ExactoDbfvDiagonals" in rs
    for method in ("dbfv_rotate_hoisted", "dbfv_linear_transform", "dbfv_diagonals"):
        assert hasattr(_ffi.HipContext, method) and hasattr(_ffi.HipContext, method + "_dev"), method
    for method in ("dbfv_rotate_rows_many", "dbfv_batch_linear_transform", "set_dbfv_lt_fused"):
        assert hasattr(_ffi.HipContext, method), method
    assert hasattr(_ffi, "DbfvDiagonals")
    with open(os.path.join(ROOT, "include", "exacto.hpp")) as f:
        hpp = f.read()
    for name in ("class DbfvDiagonals", "dbfv_rotate_hoisted(", "dbfv_rotate_rows_many(", "dbfv_linear_transform("):
        assert name in hpp, name

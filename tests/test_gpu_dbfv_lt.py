"""Slot linear transforms on dBFV ciphertexts with wide public diagonals on the GPU:
exacto_dbfv_rotate_hoisted, exacto_dbfv_diagonals_*, exacto_dbfv_linear_transform[_prepared][_dev].

The reference is tests/dbfv_lt_ref.py (hoist_ref's rotations of the limbs handed to dbfv_plain_ref, held on the
CPU by tests/test_dbfv_lt_ref.py); every comparison is np.array_equal over whole outputs.

  1. the transform on arbitrary residues (not encryptions) against the reference, in the host form and both
     _dev forms, raw and prepared: uniform items, one item with every residue q_l - 1 against diagonal words
     2^64 - 1, one item all zero.  The fused kernel (dbfv_hoist.hip: the limb-wise key switch, d <= 8) at n = 16
     (a partial block), n = 64, one prime (HPS) and three, every fold class, R = 1 and 5, identities and a
     duplicate, one key and all of them, B = 1 and 5; the staged route (rotations into scratch read by the
     plaintext-product kernel) on the 31-bit key switch at n = 1024, with more than eight digits (the list
     kernel), and for every fused case again on the staged route, which is the default (the fused kernel
     measured slower, DESIGN.md §6.16, and runs after exacto_ctx_set_dbfv_lt_fused(ctx, 1));
  2. the lazy accumulation with a prime just below 2^62, every product (q - 1)^2;
  3. neither the item chunk nor the term chunk changes a result;
  4. exacto_dbfv_rotate_hoisted against exacto_bfv_rotate_hoisted of the limbs in the same process;
  5. encryptions under device-generated keys decrypt to sum_r W_r[s] x[rot_r(s)] mod p slot by slot, for the
     cases whose digits and whose noise tests/test_dbfv_lt_ref.py admits;
  6. the errors, in the header's order, and valid calls after them.

The route switch is a context setter, not an environment variable, so the staged runs of the fused cases need
no child process: the same context runs both routes and the outputs are compared directly.
"""

import functools

import numpy as np
import pytest

import dbfv_batch_ref as D
import dbfv_lt_ref as LT
from bridge import uniform_residues
from exacto_amd import _ffi
from exacto_amd._ffi import HipContext, ExactoError
from hoist_shapes import _bfv, _hps
from oracle import params as P
from oracle.ring import is_prime
from test_dbfv_batch_ref import oracle_params
from test_dbfv_lt_ref import (DECRYPT_CASES, NOISE_BOUND, STEPS, fused_route, rotation_noise_bits,
                              transform_noise_bits)

pytestmark = pytest.mark.gpu

KEY = [31, 32, 33, 34]
U64 = 1 << 64
P64 = U64 - 59
Q62 = 4611686018427365377            # the largest prime below 2^62 that is 1 mod 2048
D14 = D.min_digits(3, 10 ** 9 + 7)

# (base, d, p): a small fold; none (i + j < d only); large fold digits with high limbs
SHAPES = [(16, 2, 251), (256, 8, 0), (256, 8, P64)]

PARAMS = {
    "n16": _bfv(16, P.Q3),               # L n = 48: one partial block
    "n64": _bfv(64, P.Q3),
    "hps64": _hps(64),                   # the u64_dbfv preset's one 60-bit prime
    "n1024": _bfv(1024, P.Q3),           # the 31-bit key switch
}

ELEMENTS = {
    "three": lambda n: [3, 1, 2 * n - 1],
    "one": lambda n: [1],                                     # the identity alone: no key at all
    "five": lambda n: [1, 3, 2 * n + 1, 3, 1],                # the identity first, in the middle, last; a duplicate
    "keyed": lambda n: [3, 5, 2 * n - 1],
}


@functools.lru_cache(maxsize=None)
def _prm(name):
    return PARAMS[name]()


@functools.lru_cache(maxsize=None)
def _ctx(name):
    return HipContext.from_params(_prm(name))


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint64, order="C").view(np.int64)).to(torch.device("cuda:0"))


def _full(shape):
    import torch
    return torch.full(shape, -1, dtype=torch.int64, device="cuda:0")


def _ready():
    import torch
    torch.cuda.synchronize()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


@functools.lru_cache(maxsize=None)
def _case(pname, base, d, p, els, num_keys, B):
    """(elements, ct [B][d][2][L][n], gks, pts [R][d][n], the reference's rotations and transform), computed once
    and shared read-only.  Item 1 has every residue q_l - 1 and rotation 0's diagonal every word 2^64 - 1; item 2
    is zero."""
    prm = _prm(pname)
    n, q = prm.ring_degree, prm.ct_basis.moduli
    elements = ELEMENTS[els](n)
    R = len(elements)
    rng = np.random.default_rng(n + 31 * d + 7 * R + B)
    ct = uniform_residues(rng, (B, d, 2), q, n)
    if B >= 3:
        ct[1] = (np.array(q, dtype=np.uint64) - np.uint64(1))[None, None, :, None]
        ct[2] = 0
    guse = prm.gadget_digits if num_keys is None else num_keys
    gks = uniform_residues(rng, (R, guse, 2), q, n)
    pts = rng.integers(0, U64, size=(R, d, n), dtype=np.uint64)
    pts[0] = U64 - 1
    rot = LT.rotate_hoisted(prm, ct, elements, gks, threads=4)
    want = LT.linear_transform(prm, ct, elements, gks, pts, base, d, p, rotated=rot)
    for a in (ct, gks, pts, rot, want):
        a.setflags(write=False)
    return elements, ct, gks, pts, rot, want


def _keyset(ctx, elements, gks):
    return ctx.galois_keyset(elements, gks if any(e % (2 * ctx.n) != 1 for e in elements) else None)


def _check(ctx, ks, base, d, p, ct, pts, want, forms=("host", "dev")):
    """The host form and both _dev forms, raw and prepared; the inputs stay as they were."""
    B, L, n = ct.shape[0], ct.shape[3], ct.shape[4]
    R = pts.shape[0]
    dg = ctx.dbfv_diagonals(d, pts)
    assert (dg.R, dg.d) == (R, d)
    if "host" in forms:
        got, depth = ctx.dbfv_linear_transform(d, base, p, ct, ks, pts)
        assert np.array_equal(got, want), "host, raw"
        assert depth.tolist() == [1] * B
        got, depth = ctx.dbfv_linear_transform(d, base, p, ct, ks, dg)
        assert np.array_equal(got, want) and depth.tolist() == [1] * B, "host, prepared"
    if "dev" in forms:
        ct_d, pts_d = _dev(ct), _dev(pts)
        out = _full((B, d, 2, L, n))
        _ready()
        ctx.dbfv_linear_transform_dev(d, base, p, ct_d, ks, pts_d, out, B)
        ctx.synchronize()
        assert np.array_equal(_host(out), want), "_dev, raw"
        dgd = ctx.dbfv_diagonals_dev(d, pts_d, R)
        out.fill_(-1)
        _ready()
        ctx.dbfv_linear_transform_dev(d, base, p, ct_d, ks, dgd, out, B)
        ctx.synchronize()
        assert np.array_equal(_host(out), want), "_dev, prepared"
        assert np.array_equal(_host(ct_d), ct) and np.array_equal(_host(pts_d), pts), "the inputs are untouched"
        dgd.close()
    dg.close()


def _route(ctx, pname, d, fused_on=False):
    """The library's report of the route, held against the restatement of tests/test_dbfv_lt_ref.py."""
    prm = _prm(pname)
    dg = ctx.dbfv_diagonals(d, np.zeros((1, d, ctx.n), dtype=np.uint64))
    fused = dg.fused
    dg.close()
    assert fused == fused_route(prm.ring_degree, ctx.L, prm.gadget_base, d, fused_on=fused_on)
    assert (ctx.ks32_primes > 0) == (pname == "n1024")
    return fused


# (params, elements, num_keys, B) of the fused route; every one of them runs the three SHAPES
FUSED = [
    ("n16", "three", None, 5),
    ("n64", "three", None, 5),
    ("hps64", "three", None, 5),
    ("n64", "one", None, 5),             # R = 1, the identity alone (guse = 0)
    ("n64", "five", None, 5),            # R = 5
    ("n64", "keyed", 1, 5),              # guse = 1
    ("n64", "keyed", None, 1),           # guse = 12 > 4: across the unroll tail; B = 1
]


# ------------------------------------------------------------------ 1. arithmetic on arbitrary residues

@pytest.mark.parametrize("base,d,p", SHAPES)
@pytest.mark.parametrize("pname,els,num_keys,B", FUSED)
def test_fused_route_against_the_reference(gpu_available, pname, els, num_keys, B, base, d, p):
    ctx = _ctx(pname)
    assert not _route(ctx, pname, d), "the default is the staged route"
    elements, ct, gks, pts, _, want = _case(pname, base, d, p, els, num_keys, B)
    ks = _keyset(ctx, elements, gks)
    assert ks.ks32_primes == 0 and ks.num_keys_used == (0 if els == "one" else gks.shape[1])
    ctx.set_dbfv_lt_fused(True)
    try:
        assert _route(ctx, pname, d, fused_on=True), "these cases are the fused kernel's"
        _check(ctx, ks, base, d, p, ct, pts, want)
    finally:
        ctx.set_dbfv_lt_fused(False)
    # the same on the staged route: the same bits
    _check(ctx, ks, base, d, p, ct, pts, want, forms=("dev",))
    ks.close()


@pytest.mark.parametrize("base,d,p", SHAPES[:2])
def test_staged_route_on_the_31_bit_key_switch(gpu_available, base, d, p):
    ctx = _ctx("n1024")
    ctx.set_dbfv_lt_fused(True)                                # the 31-bit key switch stays on the staged route
    try:
        assert not _route(ctx, "n1024", d, fused_on=True)
    finally:
        ctx.set_dbfv_lt_fused(False)
    elements, ct, gks, pts, _, want = _case("n1024", base, d, p, "three", None, 3)
    ks = _keyset(ctx, elements, gks)
    assert ks.ks32_primes > 0
    _check(ctx, ks, base, d, p, ct, pts, want)
    ks.close()


def test_staged_route_with_more_than_eight_digits(gpu_available):
    """d = 14 at n = 64: the limb-wise rotations into scratch, then the list kernel."""
    base, d, p = 3, D14, 10 ** 9 + 7
    ctx = _ctx("n64")
    assert d > 8 and not _route(ctx, "n64", d)
    elements, ct, gks, pts, _, want = _case("n64", base, d, p, "three", None, 3)
    ks = _keyset(ctx, elements, gks)
    _check(ctx, ks, base, d, p, ct, pts, want)
    ks.close()


# ------------------------------------------------------------------ 2. the lazy accumulation

@pytest.mark.parametrize("base,d,p,R", [(16, 2, 251, 9), (256, 8, P64, 3), (256, 8, 0, 3)])
def test_a_prime_just_below_2_62(gpu_available, base, d, p, R):
    """q < 2^62: a 128-bit sum holds 16 products and the kernel reduces after 14, so d = 2 reduces every 7
    rotations and d = 8 every rotation.  Identity elements keep the residues q - 1 of item 1 as they are, and the
    constant polynomial q - 1 lifts to q - 1 in every position: every product of item 1 is (q - 1)^2."""
    assert is_prime(Q62) and (Q62 - 1) % 2048 == 0 and Q62.bit_length() == 62
    n, B = 16, 3
    prm = P.BfvParamsBuilder().ring_degree(n).plain_modulus(12289).ct_moduli([Q62]).build()
    ctx = HipContext.from_params(prm)
    ctx.set_dbfv_lt_fused(True)                                # the fused kernel's own flushes
    flush = ctx.dbfv_plain_limits()[0]
    assert flush == 14 and R > flush // d, "the case crosses the flush count"
    rng = np.random.default_rng(d + R)
    ct = uniform_residues(rng, (B, d, 2), [Q62], n)
    ct[1] = Q62 - 1
    ct[2] = 0
    top = np.zeros((R, d, n), dtype=np.uint64)
    top[..., 0] = Q62 - 1
    elements = [1 + 2 * n * r for r in range(R)]              # all the identity
    ks = ctx.galois_keyset(elements, None)
    unread = uniform_residues(rng, (R, 1, 2), [Q62], n)          # the identity reads no key
    want = LT.linear_transform(prm, ct, elements, unread, top, base, d, p)
    _check(ctx, ks, base, d, p, ct, top, want)
    # ... and keyed rotations of uniform items under uniform diagonals with the same prime
    elements = [3] * (R - 1) + [1]
    gks = uniform_residues(rng, (R, prm.gadget_digits, 2), [Q62], n)
    pts = rng.integers(0, U64, size=(R, d, n), dtype=np.uint64)
    ks2 = ctx.galois_keyset(elements, gks)
    want = LT.linear_transform(prm, ct, elements, gks, pts, base, d, p)
    _check(ctx, ks2, base, d, p, ct, pts, want, forms=("dev",))


# ------------------------------------------------------------------ 3. chunks change nothing

@pytest.mark.parametrize("pname", ["n64", "n1024"])
def test_chunks_change_nothing(gpu_available, pname):
    """set_plain_terms(2) with R = 5 (n = 1024: R = 3): later rotation groups add into out, in the fused kernel
    and in the staged product; set_chunk(1) and a chunk smaller than d: one dBFV ciphertext per launch."""
    base, d, p = 256, 8, P64
    els, B = ("five", 5) if pname == "n64" else ("three", 3)
    if pname == "n1024":
        base, d, p = 256, 8, 0
    ctx = HipContext.from_params(_prm(pname))                    # a context of its own: the settings stay here
    elements, ct, gks, pts, _, want = _case(pname, base, d, p, els, None, B)
    ks = _keyset(ctx, elements, gks)
    dg = ctx.dbfv_diagonals(d, pts)
    for fused in ((True, False) if pname == "n64" else (True,)):
        ctx.set_dbfv_lt_fused(fused)
        for chunk, terms in ((64, 2), (1, 0), (d - 1, 2), (2 * d + 1, 0)):
            ctx.set_chunk(chunk)
            ctx.set_plain_terms(terms)
            raw, _ = ctx.dbfv_linear_transform(d, base, p, ct, ks, pts)
            assert np.array_equal(raw, want), (fused, chunk, terms, "raw")
            prep, _ = ctx.dbfv_linear_transform(d, base, p, ct, ks, dg)
            assert np.array_equal(prep, want), (fused, chunk, terms, "prepared")
    ks.close()


# ------------------------------------------------------------------ 4. the rotations alone

@pytest.mark.parametrize("pname,base,d,p", [("n64", 256, 8, P64), ("n1024", 16, 2, 251)])
def test_rotate_hoisted_is_the_bfv_call_on_the_limbs(gpu_available, pname, base, d, p):
    ctx = HipContext.from_params(_prm(pname))                    # a context of its own: the chunk stays here
    els, B = ("five", 5) if pname == "n64" else ("three", 3)
    elements, ct, gks, _, rot, _ = _case(pname, base, d, p, els, None, B)
    R, L, n = len(elements), ctx.L, ctx.n
    ks = _keyset(ctx, elements, gks)
    limbs = ctx.bfv_rotate_hoisted(ct.reshape(B * d, 2, L, n), ks)             # [B*d][R][2][L][n]
    want = np.ascontiguousarray(limbs.reshape(B, d, R, 2, L, n).transpose(0, 2, 1, 3, 4, 5))
    assert np.array_equal(want, rot), "the BFV call against the reference"
    got = ctx.dbfv_rotate_hoisted(ct, ks)
    assert got.shape == (B, R, d, 2, L, n) and np.array_equal(got, want), "host form"
    ct_d, out = _dev(ct), _full((B, R, d, 2, L, n))
    _ready()
    for chunk in (64, 1, d + 1):
        ctx.set_chunk(chunk)
        out.fill_(-1)
        _ready()
        ctx.dbfv_rotate_hoisted_dev(d, ct_d, ks, out, B)
        ctx.synchronize()
        assert np.array_equal(_host(out), want), ("_dev form", chunk)
    assert np.array_equal(_host(ct_d), ct)
    ks.close()


# ------------------------------------------------------------------ 5. decrypt level

def _roll(v, s):
    h = v.shape[-1] // 2
    return np.concatenate([np.roll(v[..., :h], -s, axis=-1), np.roll(v[..., h:], -s, axis=-1)], axis=-1)


def _encrypted_transform(n, t, base, d, p):
    """Device-generated keys, dbfv_batch_encrypt_sk of random wide values (slots 0 and 1 extreme), the rotations
    and the transform with random wide diagonals; the rotations decrypt, and the transform is the composition of
    the calls that existed before bit for bit, so its noise is the composition's.  Returns what the decrypt-level
    test goes on with and the measured noise_inf bits (rotated limb, transform, the budget Delta / 2)."""
    m, B, R = D.modulus(p), 2, len(STEPS)
    prm = oracle_params(n, t, base, d, p).bfv_params
    ctx = HipContext.from_params(prm)
    rng = np.random.default_rng(n + d)
    sk = ctx.gen_secret_key(KEY, stream=1)
    gks = np.zeros((R, ctx.G, 2, ctx.L, n), dtype=np.uint64)
    for r, s in enumerate(STEPS):
        if s % (n // 2):
            gks[r] = ctx.gen_galois_key(sk, _ffi.galois_element_rotate_rows(n, s), KEY, stream=10 + r)
    x = rng.integers(0, m, size=(B, n), dtype=np.uint64)
    W = rng.integers(0, m, size=(R, n), dtype=np.uint64)
    x[0, :2] = m - 1
    W[:, :2] = m - 1
    args = (d, base, p)
    ct = ctx.dbfv_batch_encrypt_sk(*args, x, sk, KEY, stream=3)
    ks = ctx.rotate_rows_keyset(STEPS, gks)
    rot = ctx.dbfv_rotate_rows_many(ct, STEPS, ks)
    for r, s in enumerate(STEPS):
        assert np.array_equal(ctx.dbfv_batch_decrypt(*args, np.ascontiguousarray(rot[:, r]), sk), _roll(x, s)), s
    with pytest.raises(ValueError):
        ctx.dbfv_rotate_rows_many(ct, STEPS[::-1], ks)
    got, depth = ctx.dbfv_batch_linear_transform(*args, ct, ks, W)
    assert depth.tolist() == [1] * B
    comp, _ = ctx.dbfv_plain_mul_sum(*args, rot, ctx.dbfv_batch_encode(*args, W)[None])
    assert np.array_equal(got, comp)
    noise = ctx.dbfv_noise(d, got, sk)
    assert noise == ctx.dbfv_noise(d, comp, sk)
    Q = 1
    for q in prm.ct_basis.moduli:
        Q *= int(q)
    rot_bits = max(int(v).bit_length() for r in range(R) for v in ctx.dbfv_noise(d, np.ascontiguousarray(rot[:, r]), sk))
    bits = (rot_bits, max(int(v).bit_length() for v in noise), (Q // t // 2).bit_length())
    print(f"n={n} t={t} d={d}: noise_inf bits: rotated {bits[0]}, transform {bits[1]}; Delta / 2 has {bits[2]}")
    # the model of tests/test_dbfv_lt_ref.py covers what the device's keys give
    assert rot_bits <= rotation_noise_bits(n)
    assert bits[1] <= transform_noise_bits(n, t, d)
    return ctx, sk, x, W, got, bits


@pytest.mark.parametrize("n,t,base,d,p", DECRYPT_CASES)
def test_slots_decrypt_level(gpu_available, n, t, base, d, p):
    """The cases tests/test_dbfv_lt_ref.py admits: the digits of the sums fit t, and the worst-case noise of the
    transform under device-generated Galois keys fits Delta / 2.  Measured on an MI355X (noise_inf bits: rotated
    limb, transform, budget): n = 64: 124, 142, 166 at (t = 12289, d = 2) and 124, 151, 158 at (3127297, 8);
    n = 1024: 128, 149, 166 at (12289, 2)."""
    m = D.modulus(p)
    ctx, sk, x, W, got, bits = _encrypted_transform(n, t, base, d, p)
    assert bits[1] < bits[2]
    want = np.zeros(x.shape, dtype=object)
    for r, s in enumerate(STEPS):
        want = (want + W[r].astype(object) * _roll(x, s).astype(object)) % m
    assert np.array_equal(ctx.dbfv_batch_decrypt(d, base, p, got, sk), want.astype(np.uint64))


@pytest.mark.parametrize("n,t,base,d,p", NOISE_BOUND)
def test_a_case_the_noise_bound_rules_out(gpu_available, n, t, base, d, p):
    """p = 2^64 at n = 1024 over cfg3's primes: no batching prime serves it (tests/test_dbfv_lt_ref.py), so nothing
    is decrypted here; the rotations still decrypt and the transform is still the composition's bits and noise.
    Measured on an MI355X: rotated limb 128 bits, transform 158 bits, Delta / 2 has 158 bits."""
    _encrypted_transform(n, t, base, d, p)


# ------------------------------------------------------------------ 6. errors, in the header's order

def test_errors(gpu_available):
    base, d, p = 16, 2, 251
    ctx = _ctx("n64")
    elements, ct, gks, pts, _, want = _case("n64", base, d, p, "three", None, 5)
    B, L, n, R = 5, ctx.L, ctx.n, len(elements)
    ks = _keyset(ctx, elements, gks)
    dg = ctx.dbfv_diagonals(d, pts)

    def fails(fn, variant, words=None):
        with pytest.raises(ExactoError) as e:
            fn()
        assert e.value.variant == variant, str(e.value)
        if words:
            assert words in str(e.value), str(e.value)

    lt = ctx.dbfv_linear_transform
    other = HipContext.from_params(_bfv(128, P.Q3)())
    ct128 = np.zeros((1, d, 2, L, 128), dtype=np.uint64)
    pts128 = np.zeros((R, d, 128), dtype=np.uint64)
    # a key set from another context, before the dBFV parameters are looked at
    fails(lambda: other.dbfv_linear_transform(d, 1, p, ct128, ks, pts128), "InvalidParam", "galois key set")
    fails(lambda: other.dbfv_rotate_hoisted(ct128, ks), "InvalidParam", "galois key set")
    # DbfvParams::new, then more than 64 digits, before the handle
    fails(lambda: lt(d, 1, p, ct, ks, dg), "InvalidParam", "base must be >= 2")
    fails(lambda: lt(d, 2, p, ct, ks, dg), "InvalidParam", "< plain_modulus")
    ct65 = np.zeros((1, 65, 2, L, n), dtype=np.uint64)
    fails(lambda: lt(65, 2, 0, ct65, ks, dg), "InvalidParam", "64 digits")
    # a handle from another context, with another R, with another d; the depth comes after the handle
    dg128 = other.dbfv_diagonals(d, pts128)
    fails(lambda: lt(d, base, p, ct, ks, dg128, depth_ct=[1] * B), "InvalidParam", "other parameters")
    dg2 = ctx.dbfv_diagonals(d, pts[:2])
    fails(lambda: lt(d, base, p, ct, ks, dg2, depth_ct=[1] * B), "InvalidParam", "rotations")
    dg3 = ctx.dbfv_diagonals(3, np.zeros((R, 3, n), dtype=np.uint64))
    ct3 = np.zeros((1, 3, 2, L, n), dtype=np.uint64)
    fails(lambda: lt(3, 16, 251, ct3[:, :3], ks, dg), "InvalidParam", "digits")
    assert (dg3.R, dg3.d) == (R, 3)
    # depth >= 1
    fails(lambda: lt(d, base, p, ct, ks, pts, depth_ct=[0, 0, 1, 0, 0]), "NotImplemented", "lattice reduction")
    fails(lambda: lt(d, base, p, ct, ks, dg, depth_ct=[1] * B), "NotImplemented")
    # misaligned _dev buffers, after the depth; then overlap
    ct_d, pts_d, out = _dev(ct), _dev(pts), _full((B * d * 2 * L * n + 2,))
    _ready()
    ltd = ctx.dbfv_linear_transform_dev
    fails(lambda: ltd(d, base, p, ct_d, ks, pts_d, out[1:], B, depth_ct=[1] * B), "NotImplemented")
    fails(lambda: ltd(d, base, p, ct_d, ks, pts_d, out[1:], B), "InvalidParam", "16-byte aligned")
    fails(lambda: ltd(d, base, p, ct_d, ks, dg, out[1:], B), "InvalidParam", "16-byte aligned")
    fails(lambda: ltd(d, base, p, ct_d, ks, pts_d, ct_d, B), "InvalidParam", "overlap")
    fails(lambda: ltd(d, base, p, ct_d, ks, dg, ct_d, B), "InvalidParam", "overlap")
    fails(lambda: ltd(d, base, p, ct_d, ks, pts_d, pts_d, 1), "InvalidParam", "overlap")
    fails(lambda: ctx.dbfv_rotate_hoisted_dev(d, ct_d, ks, ct_d, B), "InvalidParam", "overlap")
    # diagonals_create's own
    fails(lambda: ctx.dbfv_diagonals(65, np.zeros((1, 65, n), dtype=np.uint64)), "InvalidParam", "64 digits")
    fails(lambda: ctx.dbfv_diagonals(d, pts[:0]), "InvalidParam")
    # batch == 0
    got, depth = lt(d, base, p, ct[:0], ks, pts)
    assert got.shape == (0, d, 2, L, n) and depth.shape == (0,)
    assert lt(d, base, p, ct[:0], ks, dg)[0].shape == (0, d, 2, L, n)
    assert ctx.dbfv_rotate_hoisted(ct[:0], ks).shape == (0, R, d, 2, L, n)
    ltd(d, base, p, ct_d, ks, pts_d, out, 0)
    # after the errors the next valid calls give the reference's bits, and the BFV calls are as they were
    assert np.array_equal(lt(d, base, p, ct, ks, pts)[0], want)
    assert np.array_equal(lt(d, base, p, ct, ks, dg)[0], want)
    flat = np.ascontiguousarray(ct.reshape(B * d, 2, L, n))
    before = ctx.bfv_rotate_hoisted(flat, ks)
    assert np.array_equal(lt(d, base, p, ct, ks, dg)[0], want)
    assert np.array_equal(ctx.bfv_rotate_hoisted(flat, ks), before)
    for h in (dg, dg2, dg3, dg128):
        h.close()
    h.close()                                                  # closing twice is fine
    ks.close()

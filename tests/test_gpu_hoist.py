"""Hoisted rotations and slot linear transforms on the GPU: exacto_galois_keyset_*, exacto_bfv_rotate_hoisted,
exacto_bfv_linear_transform (hoist.hip, ks32.hip's hoisted MAC).

The reference is tests/hoist_ref.py (held against the Python oracle in tests/test_hoist_ref.py); every
comparison is np.array_equal over whole outputs, ciphertexts and keys are uniform residues, and output buffers
are pre-filled with -1.

  1. parity with hoist_ref on every path: limb-wise MAC (n < 1024, u64 digits, HPS, a generic prime) and the
     31-bit path (n = 2048 its smallest shape here, 4096 with the pinned transforms, 8192 with L = 4), elements
     [3, 1, 2n - 1, 3], with every key and with two, host and _dev forms, two chunks;
  2. the linear transform, bit for bit hoist_ref's and the composition of existing library calls;
  3. decrypt level on device-generated keys: rotate_rows_many and batch_linear_transform on slots;
  4. state: repeatable, undisturbed by and not disturbing the single automorphism and the multiply;
  5. errors.
"""
import functools

import numpy as np
import pytest

import hoist_ref
from oracle import params as P
from exacto_amd import _ffi
from exacto_amd._ffi import HipContext, ExactoError
from bridge import uniform_residues

pytestmark = pytest.mark.gpu

KEY = [11, 22, 33, 44]


def _b20():
    return P.BfvParamsBuilder().ring_degree(64).plain_modulus(65537).ct_moduli(P.Q3).gadget_base(1 << 20).build()


# name -> (params, B, the context runs the 31-bit key switch)
CASES = {
    "multiprime16": (lambda: P.BfvParamsBuilder().ring_degree(16).plain_modulus(257)
                     .ct_moduli([65537, 1099509805057]).gadget_base(8).build(), 3, False),
    "cfg3_n64": (lambda: P.cfg3_params(64), 3, False),
    "cfg3_n64_base2p20": (_b20, 3, False),
    "compact": (P.compact_bfv, 3, False),
    "u64_dbfv": (lambda: P.u64_dbfv().bfv_params, 3, False),
    "cfg3_n2048": (lambda: P.cfg3_params(2048), 3, True),
    "cfg3_n4096": (lambda: P.cfg3_params(4096), 1, True),
    "cfg5_n8192": (lambda: P.cfg5_params(8192).bfv_params, 1, True),
}
LT_CASES = ["multiprime16", "cfg3_n64", "cfg3_n2048", "cfg3_n4096"]


def _elements(n):
    return [3, 1, 2 * n - 1, 3]


@functools.lru_cache(maxsize=None)
def _case(name, few):
    """(params, ct, gks, hoist_ref's rotations), computed once and shared (read-only) by the tests."""
    mk, B, _ = CASES[name]
    prm = mk()
    n, q = prm.ring_degree, prm.ct_basis.moduli
    rng = np.random.default_rng(sum(map(ord, name)) + few)
    ct = uniform_residues(rng, (B, 2), q, n)
    gks = uniform_residues(rng, (4, 2 if few else prm.gadget_digits, 2), q, n)
    want = hoist_ref.rotate_hoisted(prm, ct, _elements(n), gks, threads=4)
    for a in (ct, gks, want):
        a.setflags(write=False)
    return prm, ct, gks, want


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


def _ctx(prm, chunk=2):
    ctx = HipContext.from_params(prm)
    ctx.set_chunk(chunk)
    return ctx


# ------------------------------------------------------------------ 1. parity

@pytest.mark.parametrize("few", [0, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_hoist_ref(gpu_available, name, few):
    prm, ct, gks, want = _case(name, few)
    n, B, k32 = prm.ring_degree, CASES[name][1], CASES[name][2]
    ctx = _ctx(prm)
    print(name, "ks32_primes", ctx.ks32_primes)
    assert (ctx.ks32_primes > 0) == k32
    ks = ctx.galois_keyset(_elements(n), gks)
    assert ks.R == 4 and ks.num_keys_used == min(prm.gadget_digits, gks.shape[1])
    assert (ks.ks32_primes > 0) == k32
    got = ctx.bfv_rotate_hoisted(ct, ks)
    assert np.array_equal(got, want), "host form"
    assert np.array_equal(got[:, 1], ct), "element 1 copies the input"
    # _dev forms: the set from device keys (released before use), the rotations into a -1 filled buffer
    gks_d, ct_d = _dev(gks), _dev(ct)
    out = _full((B, 4, 2, ctx.L, n))
    _ready()
    ksd = ctx.galois_keyset_dev(_elements(n), gks_d, gks.shape[1])
    del gks_d
    ctx.bfv_rotate_hoisted_dev(ct_d, ksd, out, B)
    ctx.synchronize()
    assert np.array_equal(_host(out), want), "_dev form"
    ks.close()
    ksd.close()


# ------------------------------------------------------------------ 2. linear transform

@pytest.mark.parametrize("name", LT_CASES)
def test_linear_transform(gpu_available, name):
    prm, ct, gks, hoisted = _case(name, 0)
    n, B = prm.ring_degree, CASES[name][1]
    ctx = _ctx(prm)
    ks = ctx.galois_keyset(_elements(n), gks)
    rng = np.random.default_rng(7)
    pts = rng.integers(0, prm.plain_modulus, size=(4, n), dtype=np.uint64)
    pts[0, :3] = [2**64 - 1, prm.plain_modulus, 2**63]     # any u64, lifted as bfv_plain_mul lifts it
    want = hoist_ref.linear_transform(prm, hoisted, pts, threads=4)
    got = ctx.bfv_linear_transform(ct, ks, pts)
    assert np.array_equal(got, want), "hoist_ref"
    # the composition of existing calls on the library's own rotations
    rot = ctx.bfv_rotate_hoisted(ct, ks)
    acc = None
    for r in range(4):
        term = ctx.bfv_plain_mul(np.ascontiguousarray(rot[:, r]), np.repeat(pts[r][None], B, axis=0))
        acc = term if acc is None else ctx.bfv_add(acc, term)
    assert np.array_equal(got, acc), "composition"
    ct_d, pts_d, out = _dev(ct), _dev(pts), _full((B, 2, ctx.L, n))
    _ready()
    ctx.bfv_linear_transform_dev(ct_d, ks, pts_d, out, B)
    ctx.synchronize()
    assert np.array_equal(_host(out), want), "_dev form"


# ------------------------------------------------------------------ 3. decrypt level

def _roll(v, s):
    h = v.shape[-1] // 2
    return np.concatenate([np.roll(v[..., :h], -s, axis=-1), np.roll(v[..., h:], -s, axis=-1)], axis=-1)


@pytest.mark.parametrize("n", [64, 4096])
def test_slots_decrypt_level(gpu_available, n):
    prm = P.cfg3_params(n)
    t = prm.plain_modulus
    ctx = _ctx(prm)
    B = 3 if n == 64 else 2
    rng = np.random.default_rng(n)
    sk = ctx.gen_secret_key(KEY, stream=1)
    steps = (0, 1, -1, 5, n // 2 - 1)
    gks = np.zeros((len(steps), ctx.G, 2, ctx.L, n), dtype=np.uint64)
    for r, s in enumerate(steps):
        if s % (n // 2):
            gks[r] = ctx.gen_galois_key(sk, _ffi.galois_element_rotate_rows(n, s), KEY, stream=10 + r)
    v = rng.integers(0, t, size=(B, n), dtype=np.uint64)
    ct = ctx.batch_encrypt_sk(v, sk, KEY, stream=3)
    ks = ctx.rotate_rows_keyset(steps, gks)
    rot = ctx.rotate_rows_many(ct, steps, ks)
    for r, s in enumerate(steps):
        dec = ctx.batch_decrypt(np.ascontiguousarray(rot[:, r]), sk)
        assert np.array_equal(dec, _roll(v, s)), s
        one = ctx.rotate_rows(ct, s, gks[r] if s % (n // 2) else None)
        assert np.array_equal(dec, ctx.batch_decrypt(one, sk)), s
    # noise of the hoisted and the one-at-a-time rotations (recorded in DESIGN.md, no ratio asserted)
    pt_rot = ctx.batch_encode(_roll(v, 5))
    hoisted_noise = max(ctx.bfv_noise(np.ascontiguousarray(rot[:, 3]), sk, expected=pt_rot))
    single_noise = max(ctx.bfv_noise(ctx.rotate_rows(ct, 5, gks[3]), sk, expected=pt_rot))
    print(f"n={n} noise_inf bits: hoisted {int(hoisted_noise).bit_length()}, single {int(single_noise).bit_length()}")
    # a slot linear map with four random diagonals
    w = rng.integers(0, t, size=(4, n), dtype=np.uint64)
    ks4 = ctx.rotate_rows_keyset(steps[:4], gks[:4])
    got = ctx.batch_decrypt(ctx.batch_linear_transform(ct, ks4, w), sk)
    want = np.zeros((B, n), dtype=object)
    for r, s in enumerate(steps[:4]):
        want = (want + w[r].astype(object) * _roll(v, s).astype(object)) % t
    assert np.array_equal(got, want.astype(np.uint64))


# ------------------------------------------------------------------ 4. state and interference

@pytest.mark.parametrize("name", ["cfg3_n64", "cfg3_n2048"])
def test_state_and_interference(gpu_available, name):
    prm, ct, gks, want = _case(name, 0)
    n, q = prm.ring_degree, prm.ct_basis.moduli
    ctx = _ctx(prm)
    rng = np.random.default_rng(1)
    rlk = uniform_residues(rng, (prm.gadget_digits, 2), q, n)
    ctx.load_relin_key(rlk)
    gk5 = uniform_residues(rng, (prm.gadget_digits, 2), q, n)
    auto_before = ctx.bfv_apply_automorphism(ct, 5, gk5)
    ks = ctx.galois_keyset(_elements(n), gks)
    other = uniform_residues(rng, (2, prm.gadget_digits, 2), q, n)
    ks2 = ctx.galois_keyset([5, 2 * n - 1], other)
    want2 = hoist_ref.rotate_hoisted(prm, ct[:1], [5, 2 * n - 1], other, threads=4)
    first = ctx.bfv_rotate_hoisted(ct, ks)
    assert np.array_equal(first, want)
    assert np.array_equal(ctx.bfv_rotate_hoisted(ct, ks), first), "the same call twice"
    assert np.array_equal(ctx.bfv_rotate_hoisted(ct[:1], ks2), want2), "a second set"
    prod = ctx.bfv_mul_and_relin(ct, ct)
    assert np.array_equal(ctx.bfv_apply_automorphism(ct, 5, gk5), auto_before), "single automorphism unchanged"
    assert np.array_equal(ctx.bfv_rotate_hoisted(ct, ks), first), "valid after other calls"
    assert np.array_equal(ctx.bfv_rotate_hoisted(ct[:1], ks2), want2)
    assert np.array_equal(ctx.bfv_mul_and_relin(ct, ct), prod)


# ------------------------------------------------------------------ 5. errors

def test_errors(gpu_available):
    prm = P.cfg3_params(64)
    n, q = prm.ring_degree, prm.ct_basis.moduli
    ctx = _ctx(prm)
    rng = np.random.default_rng(2)
    gks = uniform_residues(rng, (2, prm.gadget_digits, 2), q, n)
    ct = uniform_residues(rng, (2, 2), q, n)

    def invalid(fn, words=None):
        with pytest.raises(ExactoError) as e:
            fn()
        assert e.value.variant == "InvalidParam", str(e.value)
        if words:
            assert words in str(e.value)

    invalid(lambda: ctx.galois_keyset([3, 4], gks), "hoisted automorphisms require odd Galois elements")
    invalid(lambda: ctx.galois_keyset([], gks[:0]))
    invalid(lambda: ctx.galois_keyset([3, 5], gks[:, :0]))
    ks = ctx.galois_keyset([3, 5], gks)
    # all-identity sets need no key at all
    ident = ctx.galois_keyset([1, 2 * n + 1], None)
    assert np.array_equal(ctx.bfv_rotate_hoisted(ct, ident), np.stack([ct, ct], axis=1))
    # out aliasing ct (_dev)
    buf = _full((2 * 3, 2, ctx.L, n))
    _ready()
    invalid(lambda: ctx.bfv_rotate_hoisted_dev(buf, ks, buf, 2), "overlap")
    # a set from a context with another n, and with another gadget base
    invalid(lambda: _ctx(P.cfg3_params(128)).bfv_rotate_hoisted(np.zeros((1, 2, 3, 128), dtype=np.uint64), ks))
    other = _ctx(P.BfvParamsBuilder().ring_degree(64).plain_modulus(65537).ct_moduli(P.Q3).gadget_base(256).build())
    invalid(lambda: other.bfv_rotate_hoisted(ct, ks))
    invalid(lambda: other.bfv_linear_transform(ct, ks, np.zeros((2, n), dtype=np.uint64)))
    # B = 0 is fine
    assert ctx.bfv_rotate_hoisted(ct[:0], ks).shape == (0, 2, 2, ctx.L, n)
    assert ctx.bfv_linear_transform(ct[:0], ks, np.zeros((2, n), dtype=np.uint64)).shape == (0, 2, ctx.L, n)
    ctx.bfv_rotate_hoisted_dev(buf, ks, buf, 0)

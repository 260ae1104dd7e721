"""SIMD batching on the GPU: exacto_batch_encode / decode (batch.hip), row rotations and the compositions.

The reference is tests/batch_ref.py (oracle.ring.NttPlan's transform mod t, held against evaluation by
Horner's rule in tests/test_batch_ref.py); every comparison is np.array_equal over whole outputs.

  1. parity with batch_ref, both directions, host, _dev and in place, at the smallest shapes of every
     kernel form (n < 1024: the LDS radix-2 kernel; n >= 1024: 16 values per thread) and arithmetic
     (t < 2^30 lazy, t < 2^31 reduced operands, t < 2^32 64-bit carries; primes on both sides of 2^31
     and just below 2^32);
  2. round trip at B = 257, and the compositions bit for bit at B = 5 in chunks of 2;
  3. the plaintext's 64-bit forward transform on a context with ct_moduli = [t], read through the slot
     map, gives the values back;
  4. the _dev encode reduces mod t, the host encode rejects with the reference's words;
  5. contexts that cannot batch: the errors, and that everything else still works;
  6. end to end on device-generated keys: sums, products, plaintext products, rotations, swap, trace;
  7. encoding twice gives the same bits.
"""

import numpy as np
import pytest

import batch_ref as R
from dispatch_cases import TOP3
from exacto_amd import _ffi
from exacto_amd._ffi import HipContext, ExactoError
from oracle import bootstrap as ob, params as P
from bridge import uniform_residues

pytestmark = pytest.mark.gpu

KEY = [5, 6, 7, 8]

# every t is prime and == 1 mod 2n
SHAPES = [
    (16, 97), (16, 2147483489), (16, 2147483713), (16, 4294966657),
    (64, 257), (64, 65537), (64, 2147483137), (64, 2147483777), (64, 4294966657),
    (512, 65537),
    (1024, 12289), (1024, 2147473409), (1024, 2147493889), (1024, 4294957057),
    (2048, 65537),
    (4096, 40961), (4096, 65537), (4096, 2147377153), (4096, 2147565569), (4096, 4294828033),
    (8192, 65537),
    (16384, 65537), (16384, 2147352577), (16384, 2148728833), (16384, 4294475777),
]


def _ctx(n, t):
    """A context whose ciphertext primes serve every n <= 16384 (the batching tables depend on (n, t) only)."""
    return HipContext(n, TOP3[:2], [], t, 0, device=0)


def _items(n, t):
    """All t - 1, all zero, a single 1 at slots 0, 1, n/2 - 1, n/2, n - 1, two uniform rows."""
    rng = np.random.default_rng(n * 31 + t % 1000003)
    rows = [np.full(n, t - 1, dtype=np.uint64), np.zeros(n, dtype=np.uint64)]
    for s in (0, 1, n // 2 - 1, n // 2, n - 1):
        e = np.zeros(n, dtype=np.uint64)
        e[s] = 1
        rows.append(e)
    rows += [rng.integers(0, t, size=n, dtype=np.uint64) for _ in range(2)]
    return np.stack(rows)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(torch.device("cuda:0"))


def _ready():
    """torch's copies, fills and clones run on torch's stream, the library on the context's own (non-blocking)
    one: finish the former before the library touches the buffers."""
    import torch
    torch.cuda.synchronize()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


# ------------------------------------------------------------------ 1. parity

@pytest.mark.parametrize("n,t", SHAPES)
def test_parity_with_batch_ref(gpu_available, n, t):
    import torch
    assert (t - 1) % (2 * n) == 0
    ctx = _ctx(n, t)
    assert ctx.batch_info() == R.find_psi(n, t)
    v = _items(n, t)
    B = v.shape[0]
    want_enc, want_dec = R.encode_many(v, n, t), R.decode_many(v, n, t)
    assert np.array_equal(ctx.batch_encode(v), want_enc), "host encode"
    assert np.array_equal(ctx.batch_decode(v), want_dec), "host decode"
    v_d = _dev(v)
    out = torch.full((B, n), -1, dtype=torch.int64, device=v_d.device)
    _ready()
    ctx.batch_encode_dev(v_d, out, B)
    ctx.synchronize()
    assert np.array_equal(_host(out), want_enc), "_dev encode"
    out.fill_(-1)
    _ready()
    ctx.batch_decode_dev(v_d, out, B)
    ctx.synchronize()
    assert np.array_equal(_host(out), want_dec), "_dev decode"
    inplace = v_d.clone()
    _ready()
    ctx.batch_encode_dev(inplace, inplace, B)
    ctx.synchronize()
    assert np.array_equal(_host(inplace), want_enc), "_dev encode in place"
    ctx.batch_decode_dev(inplace, inplace, B)
    ctx.synchronize()
    assert np.array_equal(_host(inplace), v), "_dev decode in place gives the values back"
    assert np.array_equal(_host(v_d), v), "the input is untouched"
    # the host form in place (one numpy buffer as input and output)
    buf = v.copy()
    _ffi.check(ctx._lib.exacto_batch_encode(ctx._h, buf.ctypes.data, buf.ctypes.data, B))
    assert np.array_equal(buf, want_enc), "host encode in place"


# ------------------------------------------------------------------ 2. round trip, chunks

def test_round_trip_many_items(gpu_available):
    n, t, B = 4096, 65537, 257
    ctx = _ctx(n, t)
    v = np.random.default_rng(3).integers(0, t, size=(B, n), dtype=np.uint64)
    pt = ctx.batch_encode(v)
    assert pt.max() < t
    assert np.array_equal(ctx.batch_decode(pt), v)
    for b in (0, 128, 256):
        assert np.array_equal(pt[b], R.encode_many(v[b:b + 1], n, t)[0]), b


def test_compositions_in_chunks(gpu_available):
    prm = P.cfg3_params(1024)
    n, t, B = prm.ring_degree, prm.plain_modulus, 5
    ctx = HipContext.from_params(prm)
    sk = ctx.gen_secret_key(KEY, stream=1)
    pk = ctx.gen_public_key(sk, KEY, stream=2)
    v = np.random.default_rng(4).integers(0, t, size=(B, n), dtype=np.uint64)
    pt = ctx.batch_encode(v)
    want_sk, want_pk = ctx.encrypt_sk(pt, sk, KEY, stream=3), ctx.encrypt_pk(pt, pk, KEY, stream=4)
    want_dec = ctx.batch_decode(ctx.bfv_decrypt(want_pk, sk))
    assert np.array_equal(want_dec, v)
    for chunk in (2, 512):
        ctx.set_chunk(chunk)
        assert np.array_equal(ctx.batch_encrypt_sk(v, sk, KEY, stream=3), want_sk), ("sk", chunk)
        assert np.array_equal(ctx.batch_encrypt_pk(v, pk, KEY, stream=4), want_pk), ("pk", chunk)
        assert np.array_equal(ctx.batch_decrypt(want_pk, sk), want_dec), ("decrypt", chunk)
    # the _dev forms on device buffers
    import torch
    ctx.set_chunk(2)
    ct = torch.full((B, 2, ctx.L, n), -1, dtype=torch.int64, device="cuda:0")
    v_d, sk_d = _dev(v), _dev(sk)
    _ready()
    ctx.batch_encrypt_sk_dev(v_d, sk_d, KEY, 3, ct, B)
    ctx.synchronize()
    assert np.array_equal(_host(ct), want_sk)
    vals = torch.full((B, n), -1, dtype=torch.int64, device="cuda:0")
    _ready()
    ctx.batch_decrypt_dev(ct, 2, sk_d, vals, B)
    ctx.synchronize()
    assert np.array_equal(_host(vals), v)


# ------------------------------------------------------------------ 3. against the 64-bit transform

def test_cross_check_with_the_64_bit_transform(gpu_available):
    n, t = 4096, 65537
    v = np.random.default_rng(5).integers(0, t, size=(3, n), dtype=np.uint64)
    pt = _ctx(n, t).batch_encode(v)
    wide = HipContext(n, [t], [], 257, 0, device=0)          # the plaintext prime as a ciphertext prime
    evals = wide.ntt_fwd(pt)                                 # stored in storage_order()
    assert np.array_equal(evals[:, np.array(R.slot_positions(n, t))], v)


# ------------------------------------------------------------------ 4. input range

def test_input_range(gpu_available):
    n, t = 1024, 12289
    ctx = _ctx(n, t)
    v = np.random.default_rng(6).integers(0, t, size=(2, n), dtype=np.uint64)
    big = v.copy()
    big[0, 0], big[0, 7], big[1, n - 1] = t, t + 5, 2 ** 64 - 1
    import torch
    out = torch.full((2, n), -1, dtype=torch.int64, device="cuda:0")
    big_d = _dev(big)
    _ready()
    ctx.batch_encode_dev(big_d, out, 2)
    ctx.synchronize()
    assert np.array_equal(_host(out), ctx.batch_encode(big % np.uint64(t)))
    assert np.array_equal(ctx.batch_decode(big), ctx.batch_decode(big % np.uint64(t)))   # decode reduces in both forms
    with pytest.raises(ExactoError) as e:
        ctx.batch_encode(big)
    assert e.value.variant == "InvalidParam" and f"plaintext {t} >= plain_modulus {t}" in str(e.value)
    with pytest.raises(ExactoError) as e:
        ctx.batch_encode(big[1:])
    assert f"plaintext {2 ** 64 - 1} >= plain_modulus {t}" in str(e.value)
    assert ctx.batch_encode(np.zeros((0, n), dtype=np.uint64)).shape == (0, n)           # batch == 0


# ------------------------------------------------------------------ 5. errors

def _still_works(ctx):
    """bfv_add and rotate_rows on a context whose batching call failed."""
    n, q = ctx.n, ctx.ct_moduli
    rng = np.random.default_rng(8)
    ct = uniform_residues(rng, (2, 2), q, n)
    gk = uniform_residues(rng, (ctx.G, 2), q, n)
    want = (ct.astype(object) * 2) % np.array(q, dtype=object)[None, None, :, None]
    assert np.array_equal(ctx.bfv_add(ct, ct), want.astype(np.uint64))
    assert np.array_equal(ctx.rotate_rows(ct, 3, gk), ctx.bfv_apply_automorphism(ct, pow(3, 3, 2 * n), gk))
    assert np.array_equal(ctx.rotate_rows(ct, n // 2), ct)


@pytest.mark.parametrize("make,t", [
    (lambda: HipContext.from_params(P.compact_bfv()), 257),            # 257 - 1 = 256 is not a multiple of 2048
    (lambda: _ctx(16, 33), 33),                                         # == 1 mod 32, composite
])
def test_contexts_that_cannot_batch(gpu_available, make, t):
    ctx = make()
    msg = f"batching requires a prime plaintext modulus t ≡ 1 (mod 2n), got t={t}, n={ctx.n}"
    v = np.zeros((1, ctx.n), dtype=np.uint64)
    for call in (ctx.batch_info, lambda: ctx.batch_encode(v), lambda: ctx.batch_decode(v)):
        with pytest.raises(ExactoError) as e:
            call()
        assert e.value.variant == "InvalidParam" and msg in str(e.value)
    _still_works(ctx)


@pytest.mark.parametrize("n,t", [(16, 4294967681), (4096, 4294991873)])
def test_plaintext_moduli_above_2_32(gpu_available, n, t):
    assert (t - 1) % (2 * n) == 0 and t > 2 ** 32
    ctx = _ctx(n, t)
    v = np.zeros((1, n), dtype=np.uint64)
    for call in (ctx.batch_info, lambda: ctx.batch_encode(v), lambda: ctx.batch_decrypt(np.zeros((1, 2, 2, n), dtype=np.uint64), v)):
        with pytest.raises(ExactoError) as e:
            call()
        assert e.value.variant == "NotImplemented" and "batching for plaintext moduli >= 2^32" in str(e.value)
    _still_works(ctx)


def test_dev_buffer_errors(gpu_available):
    import torch
    n, t = 64, 257
    ctx = _ctx(n, t)
    buf = torch.zeros(4 * n + 2, dtype=torch.int64, device="cuda:0")
    base = buf.data_ptr()
    assert base % 16 == 0
    _ready()
    for fn in (ctx.batch_encode_dev, ctx.batch_decode_dev):
        for a, b in ((base + 8, base + 2 * n * 8), (base, base + 2 * n * 8 + 8),      # misaligned
                     (base, base + n * 8), (base + n * 8, base)):                      # partly overlapping (2 items)
            with pytest.raises(ExactoError) as e:
                fn(a, b, 2)
            assert e.value.variant == "InvalidParam", (a - base, b - base)
        fn(base, base + 2 * n * 8, 2)                                                   # disjoint: fine
        fn(base, base, 2)                                                               # in place: fine
    ctx.synchronize()


# ------------------------------------------------------------------ 6. end to end

@pytest.mark.parametrize("n", [64, 4096])
def test_end_to_end(gpu_available, n):
    prm = P.cfg3_params(n)
    t, B, h = prm.plain_modulus, 2, n // 2
    ctx = HipContext.from_params(prm)
    sk = ctx.gen_secret_key(KEY, stream=1)
    ctx.gen_relin_key(sk, KEY, stream=2, resident=True)
    rng = np.random.default_rng(9)
    a, b, w = (rng.integers(0, t, size=(B, n), dtype=np.uint64) for _ in range(3))
    ca, cb = ctx.batch_encrypt_sk(a, sk, KEY, stream=3), ctx.batch_encrypt_sk(b, sk, KEY, stream=4)
    dec = lambda ct: ctx.batch_decrypt(ct, sk)
    T = np.uint64(t)
    assert np.array_equal(dec(ca), a)
    assert np.array_equal(dec(ctx.bfv_add(ca, cb)), (a + b) % T)
    assert np.array_equal(dec(ctx.bfv_mul_and_relin(ca, cb)), a * b % T)
    assert np.array_equal(dec(ctx.bfv_plain_mul(ca, ctx.batch_encode(w))), a * w % T)
    for i, k in enumerate((1, -1, 5, h - 1)):
        el = pow(3, k % h, 2 * n)
        assert _ffi.galois_element_rotate_rows(n, k) == el
        gk = ctx.gen_galois_key(sk, el, KEY, stream=10 + i)
        rot = ctx.rotate_rows(ca, k, gk)
        assert np.array_equal(rot, ctx.bfv_apply_automorphism(ca, el, gk)), k
        want = np.concatenate([np.roll(a[:, :h], -k, axis=1), np.roll(a[:, h:], -k, axis=1)], axis=1)
        assert np.array_equal(dec(rot), want), k
    assert np.array_equal(ctx.rotate_rows(ca, h), ca)                      # the identity: no key
    assert np.array_equal(ctx.rotate_rows(ca, -h, None), ca)
    gks = ctx.gen_galois_key(sk, 2 * n - 1, KEY, stream=20)
    sw = ctx.swap_rows(ca, gks)
    assert np.array_equal(sw, ctx.bfv_apply_automorphism(ca, _ffi.galois_element_swap_rows(n), gks))
    assert np.array_equal(dec(sw), np.concatenate([a[:, h:], a[:, :h]], axis=1))
    els, tks = ctx.gen_trace_galois_keys(sk, KEY, stream=30)
    assert els == ob.required_trace_elements(n)
    total = a.sum(axis=1) % T                                               # n t < 2^64
    assert np.array_equal(dec(ctx.bfv_trace(ca, els, tks)), np.repeat(total[:, None], n, axis=1))


# ------------------------------------------------------------------ 7. determinism

def test_encoding_twice_gives_the_same_bits(gpu_available):
    n, t = 8192, 65537
    ctx = _ctx(n, t)
    v = np.random.default_rng(10).integers(0, t, size=(4, n), dtype=np.uint64)
    first = ctx.batch_encode(v)                  # builds the tables
    assert np.array_equal(ctx.batch_encode(v), first)
    assert np.array_equal(_ctx(n, t).batch_encode(v), first)      # and a fresh context builds the same ones

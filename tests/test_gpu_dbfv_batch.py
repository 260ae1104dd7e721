"""Slot-packed dBFV on the GPU: exacto_dbfv_batch_* (batch.hip's fused dbfv_batch_encode_kernel /
dbfv_batch_decode_kernel, one workgroup per item looping over the d digits) and the wide-slot rotations.

The reference is tests/dbfv_batch_ref.py (batch_ref's transform mod t over oracle.dbfv's digits, held on the CPU
by tests/test_dbfv_batch_ref.py); every comparison is np.array_equal over whole outputs.

  1. the transforms alone against dbfv_batch_ref, host and _dev forms, at the smallest shapes of every kernel
     (n < 1024: the LDS radix-2 form; n >= 1024: 16 values per thread), arithmetic (lazy, wide, strict) and
     accumulator (p = 0: 64-bit wrapping; a bounded sum: signed 64-bit; otherwise the 128-bit rule);
  2. dbfv_batch_encrypt_sk / _pk are encrypt_sk / encrypt_pk over the reference's [B d][n] plaintexts bit for
     bit, with a chunk boundary inside the batch;
  3. dbfv_batch_decrypt is bfv_decrypt, batch_decode and the Python recomposition, and returns the values;
  4. dbfv_mul / dbfv_square / dbfv_add / dbfv_sub of batch-encrypted operands decrypt to the slot-wise result
     mod p, and dbfv_rotate_rows / dbfv_swap_rows move the wide slots;
  5. the errors, in the header's order.
"""

import numpy as np
import pytest

import batch_ref as R
import dbfv_batch_ref as D
from dispatch_cases import TOP3
from exacto_amd._ffi import HipContext, ExactoError
from oracle import dbfv as odbfv, params as P

pytestmark = pytest.mark.gpu

KEY = [11, 12, 13, 14]
U64 = 1 << 64
P64 = U64 - 59                    # a prime just below 2^64: the 128-bit accumulator

# (n, t, base, d, p); p = 0 is 2^64
SMALL = [
    (16, 1153, 16, 2, 256),
    (64, 1153, 16, 2, 251),
    (16, 1040449, 256, 8, 0),
    (32, 2147483713, 3, D.min_digits(3, 10 ** 9 + 7), 10 ** 9 + 7),       # strict, a base that is no power of two
    (16, 1040449, 256, 8, P64),                                            # sums beyond 2^63: the i128 rule
]
BIG = [
    (1024, 12289, 16, 2, 256),                                             # lazy
    (1024, 1073750017, 256, 8, 0),                                         # wide
    (1024, 2147493889, 256, 8, 0),                                         # strict
    (1024, 12289, 256, 8, P64),                                            # lazy, the i128 rule
    (4096, 1073153, 256, 8, 0),                                            # the u64 profile's batching prime
    # 1024 threads per workgroup: no row loaded ahead, and the 128-bit sums in four walks over the digits
    (16384, 65537, 256, 8, 0),
    (16384, 65537, 256, 8, P64),
    (16384, 4294475777, 256, 8, 0),                                        # strict
]


def _ctx(n, t, L=2):
    """cfg3's primes (== 1 mod 16384); at n = 16384 the top special primes == 1 mod 32768."""
    return HipContext(n, (TOP3 if n > 8192 else P.Q3)[:L], [], t, 0, device=0)


def _values(n, p, B, seed):
    """Item 0: slots 0 .. 3 hold 0, 1, p - 1, p - 1 and the rest is uniform below p; item 1: uniform u64 (values
    >= p, reduced); the others uniform below p."""
    m = D.modulus(p)
    rng = np.random.default_rng(seed)
    v = np.array([[int(x) % m for x in rng.integers(0, U64, size=n, dtype=np.uint64)] for _ in range(B)],
                 dtype=np.uint64)
    v[0, :4] = [0, 1, m - 1, m - 1]
    if p:
        v[1] = rng.integers(0, U64, size=n, dtype=np.uint64)
        v[1, 0], v[1, 1] = p, U64 - 1
    return v


def _reduced(v, p):
    return v if p == 0 else v % np.uint64(p)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(torch.device("cuda:0"))


def _ready():
    """torch's copies and fills run on torch's stream, the library on the context's own: finish the former."""
    import torch
    torch.cuda.synchronize()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


# ------------------------------------------------------------------ 1. the transforms alone

@pytest.mark.parametrize("n,t,base,d,p", SMALL + BIG)
def test_transforms_against_the_reference(gpu_available, n, t, base, d, p):
    import torch
    B = 3
    assert (t - 1) % (2 * n) == 0 and base <= t and base ** d >= D.modulus(p)
    ctx = _ctx(n, t)
    v = _values(n, p, B, n + d)
    want_pt = D.encode_many(v, n, t, d, base, p)
    got_pt = ctx.dbfv_batch_encode(d, base, p, v)
    assert got_pt.shape == (B, d, n)
    assert np.array_equal(got_pt, want_pt), "host encode"
    # decode inputs: the encodings; slot digits anywhere in [0, t) (negative once centred); arbitrary u64
    rng = np.random.default_rng(n * 7 + d)
    neg = R.encode_many(rng.integers(0, t, size=(d, n), dtype=np.uint64), n, t)
    neg_top = R.encode_many(np.full((d, n), t // 2 + 1, dtype=np.uint64), n, t)        # every digit the most negative
    wild = rng.integers(0, U64, size=(d, n), dtype=np.uint64)
    pts = np.stack([want_pt[0], want_pt[1], neg, neg_top, wild])
    want_v = D.decode_many(pts, n, t, d, base, p)
    assert np.array_equal(want_v[:2], _reduced(v[:2], p))
    assert np.array_equal(ctx.dbfv_batch_decode(d, base, p, pts), want_v), "host decode"
    # the _dev forms
    v_d, pts_d = _dev(v), _dev(pts)
    pt_out = torch.full((B, d, n), -1, dtype=torch.int64, device=v_d.device)
    v_out = torch.full((pts.shape[0], n), -1, dtype=torch.int64, device=v_d.device)
    _ready()
    ctx.dbfv_batch_encode_dev(d, base, p, v_d, pt_out, B)
    ctx.dbfv_batch_decode_dev(d, base, p, pts_d, v_out, pts.shape[0])
    ctx.synchronize()
    assert np.array_equal(_host(pt_out), want_pt), "_dev encode"
    assert np.array_equal(_host(v_out), want_v), "_dev decode"
    assert np.array_equal(_host(v_d), v) and np.array_equal(_host(pts_d), pts), "the inputs are untouched"


def test_every_limb_is_the_slot_encoding_of_its_digits(gpu_available):
    """Against the library's own exacto_batch_encode of host digits: the same zeta, the same slot matrix."""
    n, t, base, d, p = 1024, 12289, 16, 2, 256
    ctx = _ctx(n, t)
    v = _values(n, p, 2, 5)
    dig = np.array([D.digits(row.tolist(), d, base, p) for row in v], dtype=np.uint64)
    assert np.array_equal(ctx.dbfv_batch_encode(d, base, p, v), ctx.batch_encode(dig.reshape(-1, n)).reshape(2, d, n))


# ------------------------------------------------------------------ 2. encrypt is the stated composition

@pytest.mark.parametrize("n,t,L,B,chunk", [(64, 1153, 1, 3, 2), (1024, 12289, 3, 2, 512)])
def test_encrypt_is_encode_then_encrypt(gpu_available, n, t, L, B, chunk):
    import torch
    base, d, p = 16, 2, 256
    ctx = _ctx(n, t, L)
    sk = ctx.gen_secret_key(KEY, stream=1)
    pk = ctx.gen_public_key(sk, KEY, stream=2)
    v = _values(n, p, B, 6)
    pts = D.encode_many(v, n, t, d, base, p).reshape(B * d, n)
    want_sk, want_pk = ctx.encrypt_sk(pts, sk, KEY, stream=3), ctx.encrypt_pk(pts, pk, KEY, stream=4)
    ctx.set_chunk(chunk)
    got = ctx.dbfv_batch_encrypt_sk(d, base, p, v, sk, KEY, stream=3)
    assert got.shape == (B, d, 2, L, n)
    assert np.array_equal(got.reshape(want_sk.shape), want_sk), "sk"
    got = ctx.dbfv_batch_encrypt_pk(d, base, p, v, pk, KEY, stream=4)
    assert np.array_equal(got.reshape(want_pk.shape), want_pk), "pk"
    ct = torch.full((B, d, 2, L, n), -1, dtype=torch.int64, device="cuda:0")
    v_d, sk_d, pk_d = _dev(v), _dev(sk), _dev(pk)
    _ready()
    ctx.dbfv_batch_encrypt_sk_dev(d, base, p, v_d, sk_d, KEY, 3, ct, B)
    ctx.synchronize()
    assert np.array_equal(_host(ct).reshape(want_sk.shape), want_sk), "_dev sk"
    ctx.dbfv_batch_encrypt_pk_dev(d, base, p, v_d, pk_d, KEY, 4, ct, B)
    ctx.synchronize()
    assert np.array_equal(_host(ct).reshape(want_pk.shape), want_pk), "_dev pk"


# ------------------------------------------------------------------ 3. decrypt

@pytest.mark.parametrize("n,t,L,B,chunk", [(64, 1153, 1, 3, 2), (1024, 12289, 3, 2, 512)])
def test_decrypt_is_decrypt_then_decode(gpu_available, n, t, L, B, chunk):
    import torch
    base, d, p = 16, 2, 256
    ctx = _ctx(n, t, L)
    sk = ctx.gen_secret_key(KEY, stream=1)
    v = _values(n, p, B, 7)
    ct = ctx.dbfv_batch_encrypt_sk(d, base, p, v, sk, KEY, stream=5)
    slots = ctx.batch_decode(ctx.bfv_decrypt(ct.reshape(B * d, 2, L, n), sk)).reshape(B, d, n).tolist()
    want = np.array([[odbfv.digit_recompose_signed([slots[b][k][s] for k in range(d)], base, p, t) for s in range(n)]
                     for b in range(B)], dtype=np.uint64)
    assert np.array_equal(want, _reduced(v, p))
    ctx.set_chunk(chunk)
    assert np.array_equal(ctx.dbfv_batch_decrypt(d, base, p, ct, sk), want)
    out = torch.full((B, n), -1, dtype=torch.int64, device="cuda:0")
    ct_d, sk_d = _dev(ct), _dev(sk)
    _ready()
    ctx.dbfv_batch_decrypt_dev(d, base, p, ct_d, sk_d, out, B)
    ctx.synchronize()
    assert np.array_equal(_host(out), want)


# ------------------------------------------------------------------ 4. arithmetic end to end

@pytest.mark.parametrize("n,t,base,d,p", [(16, 1153, 16, 2, 256), (16, 1040449, 256, 8, 0), (1024, 12289, 16, 2, 256)])
def test_arithmetic_end_to_end(gpu_available, n, t, base, d, p):
    m, B, h = D.modulus(p), 2, n // 2
    ctx = _ctx(n, t, 3)                                       # the parameters of test_dbfv_batch_ref.oracle_params
    sk = ctx.gen_secret_key(KEY, stream=1)
    ctx.gen_relin_key(sk, KEY, stream=2, resident=True)
    a, b = _reduced(_values(n, p, B, 8), p), _reduced(_values(n, p, B, 9), p)
    b[0, 2] = m - 2                                           # slot 2: (p - 1)(p - 2); slot 3: (p - 1)^2
    args = (d, base, p)
    ca = ctx.dbfv_batch_encrypt_sk(*args, a, sk, KEY, stream=3)
    cb = ctx.dbfv_batch_encrypt_sk(*args, b, sk, KEY, stream=4)
    dec = lambda ct: ctx.dbfv_batch_decrypt(*args, ct, sk)
    mod = lambda rows: np.array([[int(x) % m for x in row] for row in rows], dtype=np.uint64)
    ai, bi = a.astype(object), b.astype(object)
    assert np.array_equal(dec(ca), a)
    assert np.array_equal(dec(ctx.dbfv_mul(*args, ca, cb)[0]), mod(ai * bi)), "mul"
    assert np.array_equal(dec(ctx.dbfv_square(*args, ca)[0]), mod(ai * ai)), "square"
    assert np.array_equal(dec(ctx.dbfv_add(ca, cb)[0]), mod(ai + bi)), "add"
    assert np.array_equal(dec(ctx.dbfv_sub(ca, cb)[0]), mod(ai - bi)), "sub"
    for i, k in enumerate((1, -1)):
        gk = ctx.gen_galois_key(sk, pow(3, k % h, 2 * n), KEY, stream=10 + i)
        want = np.array([R.rotate_rows(row.tolist(), k, n) for row in a], dtype=np.uint64)
        assert np.array_equal(dec(ctx.dbfv_rotate_rows(ca, k, gk)), want), k
    gk = ctx.gen_galois_key(sk, 2 * n - 1, KEY, stream=20)
    want = np.array([R.swap_rows(row.tolist(), n) for row in a], dtype=np.uint64)
    assert np.array_equal(dec(ctx.dbfv_swap_rows(ca, gk)), want)


# ------------------------------------------------------------------ 5. errors

def _raises(call, variant, text):
    with pytest.raises(ExactoError) as e:
        call()
    assert e.value.variant == variant and text in str(e.value), str(e.value)


def test_a_context_that_cannot_batch(gpu_available):
    ctx = HipContext.from_params(P.compact_bfv())             # t = 257, n = 1024
    n = ctx.n
    msg = f"batching requires a prime plaintext modulus t ≡ 1 (mod 2n), got t=257, n={n}"
    v, pt = np.zeros((1, n), dtype=np.uint64), np.zeros((1, 2, n), dtype=np.uint64)
    ct, sk = np.zeros((1, 2, 2, ctx.L, n), dtype=np.uint64), np.zeros((ctx.L, n), dtype=np.uint64)
    for call in (lambda: ctx.dbfv_batch_encode(2, 16, 256, v), lambda: ctx.dbfv_batch_decode(2, 16, 256, pt),
                 lambda: ctx.dbfv_batch_encrypt_sk(2, 16, 256, v, sk, KEY),
                 lambda: ctx.dbfv_batch_decrypt(2, 16, 256, ct, sk),
                 lambda: ctx.dbfv_batch_encode(0, 16, 256, v)):          # the batching error comes first
        _raises(call, "InvalidParam", msg)


def test_parameter_errors_in_order(gpu_available):
    n, t = 64, 1153
    ctx = _ctx(n, t, 1)
    v = np.zeros((1, n), dtype=np.uint64)
    sk = np.zeros((1, n), dtype=np.uint64)
    for enc in (lambda d, b, p: ctx.dbfv_batch_encode(d, b, p, v),
                lambda d, b, p: ctx.dbfv_batch_decode(d, b, p, np.zeros((1, d, n), dtype=np.uint64)),
                lambda d, b, p: ctx.dbfv_batch_encrypt_sk(d, b, p, v, sk, KEY),
                lambda d, b, p: ctx.dbfv_batch_encrypt_pk(d, b, p, v, np.zeros((2, 1, n), dtype=np.uint64), KEY),
                lambda d, b, p: ctx.dbfv_batch_decrypt(d, b, p, np.zeros((1, d, 2, 1, n), dtype=np.uint64), sk)):
        _raises(lambda: enc(1, 2048, 256), "InvalidParam", f"dBFV base 2048 must be <= BFV plaintext modulus {t}")
        _raises(lambda: enc(0, 16, 256), "InvalidParam", "num_digits must be >= 1")
        _raises(lambda: enc(1, 16, 256), "InvalidParam", "base^digits = 16 < plain_modulus = 256")
        _raises(lambda: enc(7, 256, 0), "InvalidParam", f"base^digits = {256 ** 7} < plain_modulus = {U64}")
        _raises(lambda: enc(1, 1, 256), "InvalidParam", "base must be >= 2")
        _raises(lambda: enc(0, 2048, 256), "InvalidParam", "num_digits must be >= 1")     # before the base range


def test_dev_buffer_errors_and_empty_batches(gpu_available):
    import torch
    n, t, d, base, p = 64, 1153, 2, 16, 256
    ctx = _ctx(n, t, 1)
    buf = torch.zeros(8 * n + 2, dtype=torch.int64, device="cuda:0")
    lo = buf.data_ptr()
    assert lo % 16 == 0
    _ready()
    w = 8                                                      # bytes per word
    # values [2][n] at a, pt [2][d][n] at b
    for a, b in ((lo + 8, lo + 4 * n * w), (lo, lo + 4 * n * w + 8),                     # misaligned
                 (lo, lo + n * w), (lo + 2 * n * w, lo), (lo + 2 * n * w, lo + 2 * n * w),  # overlapping
                 (0, lo), (lo, 0)):                                                       # null
        _raises(lambda: ctx.dbfv_batch_encode_dev(d, base, p, a, b, 2), "InvalidParam", "dbfv batch")
        _raises(lambda: ctx.dbfv_batch_decode_dev(d, base, p, b, a, 2), "InvalidParam", "dbfv batch")
    ctx.dbfv_batch_encode_dev(d, base, p, lo, lo + 2 * n * w, 2)                           # adjacent: fine
    ctx.dbfv_batch_decode_dev(d, base, p, lo + 2 * n * w, lo, 2)
    ctx.synchronize()
    # batch == 0 returns 0, in every form
    ctx.dbfv_batch_encode_dev(d, base, p, lo, lo, 0)
    ctx.dbfv_batch_decode_dev(d, base, p, lo, lo, 0)
    assert ctx.dbfv_batch_encode(d, base, p, np.zeros((0, n), dtype=np.uint64)).shape == (0, d, n)
    assert ctx.dbfv_batch_decode(d, base, p, np.zeros((0, d, n), dtype=np.uint64)).shape == (0, n)
    sk = ctx.gen_secret_key(KEY, stream=1)
    assert ctx.dbfv_batch_encrypt_sk(d, base, p, np.zeros((0, n), dtype=np.uint64), sk, KEY).shape == (0, d, 2, 1, n)
    assert ctx.dbfv_batch_decrypt(d, base, p, np.zeros((0, d, 2, 1, n), dtype=np.uint64), sk).shape == (0, n)

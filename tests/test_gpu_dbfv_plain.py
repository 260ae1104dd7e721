"""dBFV plaintext products on the GPU: exacto_dbfv_plain_mul_sum / _mul / _add / _sub (dbfv_plain.hip's fused
dbfv_plain_mul_kernel: the registers form for d <= 8, the list form above) and the slot-level helpers.

The reference is tests/dbfv_plain_ref.py (held on the CPU by tests/test_dbfv_plain_ref.py); every comparison is
np.array_equal over whole outputs.

  1. the products on arbitrary residues (not encryptions) against the reference: uniform items, one item with
     every residue q_l - 1 against plaintext words 2^64 - 1, one item all zero; the packed tail (n = 16) and the
     WIDE form (n = 1024); one and three primes; two and three components; folds that are empty, small, large
     and dense; a shared plaintext and one per item; K = 1 and 3; host and _dev forms; and term counts beyond the
     kernel's lazy-accumulation flush count and beyond one term chunk, also with a prime just below 2^62, where
     a 128-bit sum holds 16 products only;
  2. batch-encrypted operands times dbfv_batch_plain_mul / _dot / _add / _sub decrypt to the slot-wise results
     mod p, and dbfv_plain_mul agrees after decryption with dbfv_mul against an encryption of the same values;
  3. dbfv_plain_add / _sub are bfv_plain_add on the B * d limbs bit for bit, and undo each other;
  4. depths and the errors, in the header's order;
  5. no result depends on the item chunk or on the term chunk.
"""

import functools

import numpy as np
import pytest

import dbfv_batch_ref as D
import dbfv_plain_ref as PR
from bridge import uniform_residues
from exacto_amd._ffi import HipContext, ExactoError
from oracle import params as P
from oracle.ring import is_prime
from test_dbfv_plain_ref import DECODES, operands, slotwise_dot

pytestmark = pytest.mark.gpu

KEY = [21, 22, 23, 24]
U64 = 1 << 64
P64 = U64 - 59
Q62 = 4611686018427365377            # the largest prime below 2^62 that is 1 mod 2048
B = 3

# (base, d, p): a small fold; none (i + j < d only); large fold digits; d > 8 (the list form), dense fold
SHAPES = [(16, 2, 251), (256, 8, 0), (256, 8, P64), (3, D.min_digits(3, 10 ** 9 + 7), 10 ** 9 + 7)]


@functools.lru_cache(maxsize=None)
def _ctx(n, moduli, t=12289):
    return HipContext(n, list(moduli), [], t, 0, device=0)


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint64).view(np.int64)).to(torch.device("cuda:0"))


def _ready():
    """torch's copies and fills run on torch's stream, the library on the context's own: finish the former."""
    import torch
    torch.cuda.synchronize()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


@functools.lru_cache(maxsize=None)
def _case(n, moduli, base, d, p, K):
    """Inputs with three components and the reference for a plaintext per item and for one shared plaintext
    (item 1's), computed once: fewer components or primes are prefixes of both."""
    rng = np.random.default_rng(n + 31 * d + K)
    cts = uniform_residues(rng, (B, K, d, 3), moduli, n)
    for l, q in enumerate(moduli):
        cts[1, ..., l, :] = q - 1
    cts[2] = 0
    pts = rng.integers(0, U64, size=(B, K, d, n), dtype=np.uint64)
    pts[1] = U64 - 1
    lifted = PR.lift(pts, moduli, n)
    own = PR.mul_sum_direct(cts, pts, moduli, base, d, p, lifted)
    shared = PR.mul_sum_direct(cts, pts[1:2], moduli, base, d, p, lifted[1:2])
    for a in (cts, pts, own, shared):
        a.setflags(write=False)
    return cts, pts, own, shared


def _check_products(ctx, cts, pts, want, base, d, p, forms=("host", "dev")):
    """cts [B][K][d][polys][L][n] against pts [B or 1][K][d][n] in the host and _dev forms (K = 1: also _mul)."""
    import torch
    K, polys, L, n = cts.shape[1], cts.shape[3], cts.shape[4], cts.shape[5]
    pb = pts.shape[0]
    if "host" in forms:
        got, depth = ctx.dbfv_plain_mul_sum(d, base, p, cts, pts)
        assert np.array_equal(got, want), "host"
        assert depth.tolist() == [1] * B
        if K == 1:
            got, depth = ctx.dbfv_plain_mul(d, base, p, cts[:, 0], pts[:, 0])
            assert np.array_equal(got, want) and depth.tolist() == [1] * B, "host, plain_mul"
    if "dev" in forms:
        cts_d, pts_d = _dev(cts), _dev(pts)
        out = torch.full((B, d, polys, L, n), -1, dtype=torch.int64, device="cuda:0")
        _ready()
        ctx.dbfv_plain_mul_sum_dev(d, base, p, cts_d, K, polys, pts_d, pb, out, B)
        ctx.synchronize()
        assert np.array_equal(_host(out), want), "_dev"
        if K == 1:
            out.fill_(-1)
            _ready()
            ctx.dbfv_plain_mul_dev(d, base, p, cts_d, polys, pts_d, pb, out, B)
            ctx.synchronize()
            assert np.array_equal(_host(out), want), "_dev, plain_mul"
        assert np.array_equal(_host(cts_d), cts) and np.array_equal(_host(pts_d), pts), "the inputs are untouched"


# ------------------------------------------------------------------ 1. arithmetic on arbitrary residues

@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("base,d,p", SHAPES)
@pytest.mark.parametrize("polys", [2, 3])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("n", [16, 1024])
def test_products_against_the_reference(gpu_available, n, L, polys, base, d, p, K):
    ctx = _ctx(n, tuple(P.Q3[:L]))
    cts3, pts, own3, shared3 = _case(n, tuple(P.Q3), base, d, p, K)
    cts = np.ascontiguousarray(cts3[:, :, :, :polys, :L])
    _check_products(ctx, cts, pts, np.ascontiguousarray(own3[:, :, :polys, :L]), base, d, p)
    _check_products(ctx, cts, pts[1:2], np.ascontiguousarray(shared3[:, :, :polys, :L]), base, d, p)


def test_more_terms_than_a_flush_and_than_a_term_chunk(gpu_available):
    """Cfg3's 60-bit primes: a 128-bit sum takes 2^8 - 2 products, so d = 2 reduces in place every 127 terms, and
    64 terms are lifted at a time: K = 130 crosses both, the second term chunk adding into out."""
    n, base, d, p, K = 16, 16, 2, 251, 130
    moduli = tuple(P.Q3)
    ctx = _ctx(n, moduli)
    FLUSH_PRODUCTS, CHUNK_TERMS = ctx.dbfv_plain_limits()
    assert (FLUSH_PRODUCTS, CHUNK_TERMS) == (2 ** (128 - 2 * 60) - 2, 64)
    FLUSH_TERMS = FLUSH_PRODUCTS // d
    assert K > FLUSH_TERMS and K > CHUNK_TERMS
    cts3, pts, own, shared = _case(n, moduli, base, d, p, K)
    cts = np.ascontiguousarray(cts3[:, :, :, :2])
    _check_products(ctx, cts, pts, np.ascontiguousarray(own[:, :, :2]), base, d, p)
    _check_products(ctx, cts, pts[1:2], np.ascontiguousarray(shared[:, :, :2]), base, d, p)
    ctx.set_plain_terms(K)                                    # one chunk: the flush inside the kernel's loop
    assert ctx.dbfv_plain_limits()[1] == K
    try:
        _check_products(ctx, cts, pts, np.ascontiguousarray(own[:, :, :2]), base, d, p)
    finally:
        ctx.set_plain_terms(0)


@pytest.mark.parametrize("n,base,d,p,K", [
    (16, 16, 2, 251, 9),                                      # 7 terms between two reductions
    (16, 256, 8, P64, 3), (1024, 256, 8, P64, 3),             # every term, and the fold's d - 1 products after it
    (16, 256, 8, 0, 3),
    (16, 3, D.min_digits(3, 10 ** 9 + 7), 10 ** 9 + 7, 2),    # the list form: 14 products
])
def test_a_prime_just_below_2_62(gpu_available, n, base, d, p, K):
    """q < 2^62 is the largest a context accepts: (q - 1)^2 is just below 2^124 and a 128-bit sum holds 16
    products, so the kernels reduce after 14; item 1 has every product (q - 1)^2."""
    assert is_prime(Q62) and (Q62 - 1) % 2048 == 0 and Q62.bit_length() == 62
    moduli = (Q62,)
    ctx = _ctx(n, moduli)
    assert ctx.dbfv_plain_limits()[0] == 14
    cts3, pts, own, shared = _case(n, moduli, base, d, p, K)
    cts = np.ascontiguousarray(cts3[:, :, :, :2])
    _check_products(ctx, cts, pts, np.ascontiguousarray(own[:, :, :2]), base, d, p)
    _check_products(ctx, cts, pts[1:2], np.ascontiguousarray(shared[:, :, :2]), base, d, p, forms=("dev",))
    # the constant polynomial q - 1 lifts to q - 1 in every position: every product of item 1 is (q - 1)^2
    top = np.zeros((1, K, d, n), dtype=np.uint64)
    top[..., 0] = Q62 - 1
    want = PR.mul_sum_direct(cts, top, moduli, base, d, p)
    _check_products(ctx, cts, top, want, base, d, p, forms=("dev",))


# ------------------------------------------------------------------ 2. end to end

def _slot_operands(n, p, K, shared):
    """a [B][K][n], w [B or 1][K][n] with test_dbfv_plain_ref.operands' extremes in slots 0 .. 3 of every row."""
    a, w = [], []
    for b in range(B):
        x, y = operands(n, p, K, 40 + b)
        a.append(x)
        w.append(y)
    w = w[:1] if shared else w
    return np.array(a, dtype=np.uint64), np.array(w, dtype=np.uint64)


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("n,t,base,d,p,K", DECODES + [(1024, 12289, 16, 2, 256, 3)])
def test_slot_products_end_to_end(gpu_available, n, t, base, d, p, K, shared):
    m = D.modulus(p)
    ctx = _ctx(n, tuple(P.Q3), t)                             # the parameters of test_dbfv_batch_ref.oracle_params
    sk = ctx.gen_secret_key(KEY, stream=1)
    a, w = _slot_operands(n, p, K, shared)
    args = (d, base, p)
    cts = np.stack([ctx.dbfv_batch_encrypt_sk(*args, a[:, k], sk, KEY, stream=3 + k) for k in range(K)], axis=1)
    dec = lambda ct: ctx.dbfv_batch_decrypt(*args, ct, sk)
    wb = np.broadcast_to(w, a.shape)
    want = np.array([slotwise_dot(a[b].tolist(), wb[b].tolist(), p) for b in range(B)], dtype=np.uint64)
    got, depth = ctx.dbfv_batch_plain_dot(*args, cts, w)
    assert depth.tolist() == [1] * B
    assert np.array_equal(dec(got), want), "dot"
    mod = lambda rows: np.array([[int(x) % m for x in row] for row in rows], dtype=np.uint64)
    a0, w0 = a[:, 0].astype(object), wb[:, 0].astype(object)
    if K == 1:
        got, _ = ctx.dbfv_batch_plain_mul(*args, cts[:, 0], w[:, 0])
        assert np.array_equal(dec(got), mod(a0 * w0)), "mul"
    assert np.array_equal(dec(ctx.dbfv_batch_plain_add(*args, cts[:, 0], w[:, 0])), mod(a0 + w0)), "add"
    assert np.array_equal(dec(ctx.dbfv_batch_plain_sub(*args, cts[:, 0], w[:, 0])), mod(a0 - w0)), "sub"


@pytest.mark.parametrize("n,t,base,d,p", [(16, 1153, 16, 2, 256), (16, 1040449, 256, 8, 0)])
def test_plain_mul_agrees_with_dbfv_mul_after_decryption(gpu_available, n, t, base, d, p):
    import torch
    ctx = _ctx(n, tuple(P.Q3), t)
    sk = ctx.gen_secret_key(KEY, stream=1)
    ctx.gen_relin_key(sk, KEY, stream=2, resident=True)
    a, w = _slot_operands(n, p, 1, False)
    a, w = a[:, 0], w[:, 0]
    args = (d, base, p)
    ca = ctx.dbfv_batch_encrypt_sk(*args, a, sk, KEY, stream=3)
    cw = ctx.dbfv_batch_encrypt_sk(*args, w, sk, KEY, stream=4)
    want = ctx.dbfv_batch_decrypt(*args, ctx.dbfv_mul(*args, ca, cw)[0], sk)
    got = ctx.dbfv_plain_mul(*args, ca, ctx.dbfv_batch_encode(*args, w))[0]
    assert np.array_equal(ctx.dbfv_batch_decrypt(*args, got, sk), want)
    # the slot-level _dev helper: encode and product on the device
    ca_d, w_d = _dev(ca), _dev(w)
    pt = torch.zeros((B, d, n), dtype=torch.int64, device="cuda:0")
    out = torch.full((B, d, 2, 3, n), -1, dtype=torch.int64, device="cuda:0")
    _ready()
    ctx.dbfv_batch_plain_mul_dev(*args, ca_d, 2, w_d, B, pt, out, B)
    ctx.synchronize()
    assert np.array_equal(_host(out), got)


# ------------------------------------------------------------------ 3. plain_add / plain_sub

@pytest.mark.parametrize("n,L,polys,d", [(16, 3, 2, 8), (1024, 1, 3, 2), (64, 3, 2, 19)])
def test_plain_add_is_bfv_plain_add_on_the_limbs(gpu_available, n, L, polys, d):
    import torch
    moduli = tuple(P.Q3[:L])
    ctx = _ctx(n, moduli)
    rng = np.random.default_rng(n + d)
    ct = uniform_residues(rng, (B, d, polys), moduli, n)
    pt = rng.integers(0, U64, size=(B, d, n), dtype=np.uint64)
    pt[1] = U64 - 1
    flat = ct.reshape(B * d, polys, L, n)
    for pts in (pt, pt[1:2]):
        pb = pts.shape[0]
        rows = np.ascontiguousarray(np.broadcast_to(pts, pt.shape)).reshape(B * d, n)
        want = ctx.bfv_plain_add(flat, rows).reshape(ct.shape)
        assert np.array_equal(want, PR.addsub_direct(ct, pts, moduli, 12289))
        got = ctx.dbfv_plain_add(ct, pts)
        assert np.array_equal(got, want), "add"
        diff = ctx.dbfv_plain_sub(ct, pts)
        assert np.array_equal(diff, PR.addsub_direct(ct, pts, moduli, 12289, sub=True)), "sub"
        assert np.array_equal(ctx.dbfv_plain_add(diff, pts), ct), "sub then add"
        assert np.array_equal(ctx.dbfv_plain_sub(got, pts), ct), "add then sub"
        ct_d, pt_d = _dev(ct), _dev(pts)
        out = torch.full(ct.shape, -1, dtype=torch.int64, device="cuda:0")
        _ready()
        ctx.dbfv_plain_add_dev(d, ct_d, polys, pt_d, pb, out, B)
        ctx.synchronize()
        assert np.array_equal(_host(out), want), "_dev add"
        ctx.dbfv_plain_sub_dev(d, out, polys, pt_d, pb, out, B)                      # in place
        ctx.synchronize()
        assert np.array_equal(_host(out), ct), "_dev sub, in place"


# ------------------------------------------------------------------ 4. depth and errors

def _raises(call, variant, text):
    with pytest.raises(ExactoError) as e:
        call()
    assert e.value.variant == variant and text in str(e.value), str(e.value)


CHAINED = "chained dBFV multiplication requires ciphertext-level lattice reduction"


def test_depths(gpu_available):
    n, base, d, p, K = 16, 16, 2, 256, 3
    ctx = _ctx(n, tuple(P.Q3[:1]))
    cts = np.zeros((B, K, d, 2, 1, n), dtype=np.uint64)
    pts = np.zeros((1, K, d, n), dtype=np.uint64)
    out, depth = ctx.dbfv_plain_mul_sum(d, base, p, cts, pts, depth_ct=np.zeros((B, K), dtype=np.uint32))
    assert depth.tolist() == [1] * B and not out.any()
    for b, k in ((0, 0), (B - 1, K - 1)):
        dc = np.zeros((B, K), dtype=np.uint32)
        dc[b, k] = 1
        _raises(lambda: ctx.dbfv_plain_mul_sum(d, base, p, cts, pts, depth_ct=dc), "NotImplemented", CHAINED)
    _raises(lambda: ctx.dbfv_plain_mul(d, base, p, cts[:, 0], pts[:, 0], depth_ct=[0, 2, 0]), "NotImplemented", CHAINED)


def test_errors_in_the_headers_order(gpu_available):
    import torch
    n, base, d, p, K, polys = 64, 16, 2, 256, 2, 2
    ctx = _ctx(n, tuple(P.Q3[:1]))
    w = 8                                                      # bytes per word
    limb = polys * n
    buf = torch.zeros((B * K * d + B * d) * limb + B * K * d * n + 4, dtype=torch.int64, device="cuda:0")
    lo = buf.data_ptr()
    assert lo % 16 == 0
    _ready()
    cts, out = lo, lo + B * K * d * limb * w
    pts = out + B * d * limb * w
    deep = np.ones((B, K), dtype=np.uint32)

    def call(cts=cts, K=K, polys=polys, pts=pts, pb=B, out=out, batch=B, d=d, base=base, p=p, depth=None):
        return lambda: ctx.dbfv_plain_mul_sum_dev(d, base, p, cts, K, polys, pts, pb, out, batch, depth)

    # each call has every later error too
    later = dict(K=0, polys=0, pb=2, d=1, depth=deep, out=cts + 8)
    _raises(call(cts=0, **later), "InvalidParam", "null argument")
    _raises(call(pts=0, **later), "InvalidParam", "null argument")
    later.pop("out")
    _raises(call(out=0, **later), "InvalidParam", "null argument")
    later["out"] = cts + 8
    _raises(call(**later), "InvalidParam", "mismatched ct/pt lengths")
    later.pop("K")
    _raises(call(**later), "InvalidParam", "ciphertext has no components")
    later.pop("polys")
    _raises(call(**later), "InvalidParam", "plaintext batch must be 1 or the batch")
    later.pop("pb")
    _raises(call(**later), "InvalidParam", "base^digits = 16 < plain_modulus = 256")
    _raises(call(base=1, **{**later, "d": 0}), "InvalidParam", "base must be >= 2")
    _raises(call(**{**later, "d": 0}), "InvalidParam", "num_digits must be >= 1")
    later.pop("d")
    _raises(call(**later), "NotImplemented", CHAINED)
    later.pop("depth")
    _raises(call(**later), "InvalidParam", "16-byte aligned")
    _raises(call(cts=cts + 8, out=cts), "InvalidParam", "16-byte aligned")        # misaligned and overlapping
    _raises(call(pts=pts + 8), "InvalidParam", "16-byte aligned")
    for bad in (cts, cts + 16, out - 16, pts, pts - 16, pts + (B * K * d * n - 2) * w):
        _raises(call(out=bad), "InvalidParam", "must not overlap")
    _raises(call(out=pts, pb=1), "InvalidParam", "must not overlap")
    call()()                                                   # adjacent buffers: fine
    call(pb=1)()
    ctx.synchronize()
    # batch == 0 returns 0 in every form, after the checks
    call(batch=0, pb=1)()
    call(batch=0, pb=0)()
    _raises(call(batch=0, pb=2), "InvalidParam", "plaintext batch must be 1 or the batch")
    got, depth = ctx.dbfv_plain_mul_sum(d, base, p, np.zeros((0, K, d, polys, 1, n), dtype=np.uint64),
                                        np.zeros((1, K, d, n), dtype=np.uint64))
    assert got.shape == (0, d, polys, 1, n) and depth.shape == (0,)
    assert ctx.dbfv_plain_add(np.zeros((0, d, polys, 1, n), dtype=np.uint64), np.zeros((1, d, n), dtype=np.uint64)).shape \
        == (0, d, polys, 1, n)
    # the host forms check the same things in the same order
    hc, hp = np.zeros((B, K, d, polys, 1, n), dtype=np.uint64), np.zeros((2, K, d, n), dtype=np.uint64)
    _raises(lambda: ctx.dbfv_plain_mul_sum(1, base, p, hc[:, :, :1], hp[:, :, :1]), "InvalidParam",
            "plaintext batch must be 1 or the batch")
    _raises(lambda: ctx.dbfv_plain_mul_sum(d, base, p, hc[:, :0], hp[:1, :0]), "InvalidParam", "mismatched ct/pt lengths")
    _raises(lambda: ctx.dbfv_plain_mul_sum(1, base, p, hc[:, :, :1], hp[:1, :, :1]), "InvalidParam",
            "base^digits = 16 < plain_modulus = 256")
    # plain_add / plain_sub: null, no components, the plaintext batch, no digits
    for fn in (ctx.dbfv_plain_add_dev, ctx.dbfv_plain_sub_dev):
        _raises(lambda: fn(0, 0, 0, pts, 2, out, B), "InvalidParam", "null argument")
        _raises(lambda: fn(0, cts, 0, pts, 2, out, B), "InvalidParam", "ciphertext has no components")
        _raises(lambda: fn(0, cts, polys, pts, 2, out, B), "InvalidParam", "plaintext batch must be 1 or the batch")
        _raises(lambda: fn(0, cts, polys, pts, 1, out, B), "InvalidParam", "num_digits must be >= 1")
        fn(d, cts, polys, pts, 1, out, 0)


def test_no_batching_context_is_required(gpu_available):
    """t = 257 at n = 1024 cannot batch (257 is not 1 mod 2048); the products and sums are defined all the same."""
    prm = P.compact_bfv()
    ctx = HipContext.from_params(prm)
    n, q = prm.ring_degree, prm.ct_basis.moduli
    base, d, p = 16, 2, 251
    rng = np.random.default_rng(3)
    cts = uniform_residues(rng, (B, 1, d, 2), q, n)
    pts = rng.integers(0, U64, size=(1, 1, d, n), dtype=np.uint64)
    assert np.array_equal(ctx.dbfv_plain_mul_sum(d, base, p, cts, pts)[0], PR.mul_sum_direct(cts, pts, q, base, d, p))
    assert np.array_equal(ctx.dbfv_plain_sub(cts[:, 0], pts[:, 0]),
                          PR.addsub_direct(cts[:, 0], pts[:, 0], q, prm.plain_modulus, sub=True))
    _raises(lambda: ctx.dbfv_batch_plain_mul(d, base, p, cts[:, 0], np.zeros((1, n), dtype=np.uint64)), "InvalidParam",
            "batching requires a prime plaintext modulus")


# ------------------------------------------------------------------ 5. independence of the chunkings

@pytest.mark.parametrize("base,d,p", [(16, 2, 251), (256, 8, P64), (3, D.min_digits(3, 10 ** 9 + 7), 10 ** 9 + 7)])
def test_results_do_not_depend_on_the_chunks(gpu_available, base, d, p):
    n, K = 16, 3
    moduli = tuple(P.Q3)
    ctx = HipContext(n, list(moduli), [], 12289, 0, device=0)    # its own context: the settings stay here
    cts3, pts, own, shared = _case(n, moduli, base, d, p, K)
    cts = np.ascontiguousarray(cts3[:, :, :, :2])
    own, shared = np.ascontiguousarray(own[:, :, :2]), np.ascontiguousarray(shared[:, :, :2])
    for chunk, terms in ((1, 0), (2, 0), (0, 1), (0, 2), (2, 2), (1, 1)):
        ctx.set_chunk(chunk)
        ctx.set_plain_terms(terms)
        assert np.array_equal(ctx.dbfv_plain_mul_sum(d, base, p, cts, pts)[0], own), (chunk, terms)
        assert np.array_equal(ctx.dbfv_plain_mul_sum(d, base, p, cts, pts[1:2])[0], shared), (chunk, terms)
        assert np.array_equal(ctx.dbfv_plain_add(cts[:, 0], pts[:, 0]),
                              PR.addsub_direct(cts[:, 0], pts[:, 0], moduli, 12289)), (chunk, terms)

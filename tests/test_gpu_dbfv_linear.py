"""dBFV on the device beyond the product: the limb-wise operations (dbfv/eval.rs:11-71,
dbfv/keyswitch.rs, dbfv/advanced.rs:15-29) and the linear maps between digit vectors
(dbfv/advanced.rs:36-160: exacto_dbfv_linear_map, _change_base, _div_by_base).

The maps are linear, so uniform canonical residues are enough for bit-exactness: against Python
integers for the kernel, against the oracle's literal bfv_plain_mul / bfv_add / bfv_sub sequence for
each function.  Real encryptions then check the semantics with the reference's own test values
(advanced.rs:183-221).
"""
import zlib

import numpy as np
import pytest

from oracle import bfv as obfv, dbfv as odbfv, params as P
from oracle.ring import CoeffPoly
from exacto_amd import _ffi
from exacto_amd._ffi import HipContext, ExactoError
from bridge import uniform_residues, np_to_ct, ct_to_np, np_to_rns

pytestmark = pytest.mark.gpu

KEY = [0x452821E638D01377, 0xBE5466CF34E90C6C, 0xC0AC29B7C97C50DD, 0x3F84D5B5B5470917]
Q1 = [1099509805057]
T = {1: 929, 3: 65537}   # BFV plaintext moduli: compact_dbfv's and cfg3's


@pytest.fixture(scope="module")
def ctxs(gpu_available):
    made = {}

    def get(n, L):
        if (n, L) not in made:
            made[(n, L)] = HipContext(n, Q1 if L == 1 else P.Q3, plain_modulus=T[L])
        return made[(n, L)]
    return get


def matrix_of(kind, d_out, d_in, t, rng):
    if kind == "random":
        return [[int(rng.integers(0, 1 << 64, dtype=np.uint64)) for _ in range(d_in)] for _ in range(d_out)]
    if kind == "above_t":       # entries >= t, congruent to small values: the mod t step shows
        return [[t * int(rng.integers(1, 1 << 40)) + int(rng.integers(0, 3)) for _ in range(d_in)]
                for _ in range(d_out)]
    if kind == "worst":
        return [[t - 1] * d_in for _ in range(d_out)]
    return [[0] * d_in for _ in range(d_out)]


def bigint_map(matrix, x, moduli, t):
    """out[b][j][p][l] = sum_i ((m_ji mod t) mod q_l) x[b][i][p][l] mod q_l with Python integers."""
    B, d_in, polys, L, n = x.shape
    xo = x.astype(object)
    out = np.zeros((B, len(matrix), polys, L, n), dtype=object)
    for j, row in enumerate(matrix):
        for l, q in enumerate(moduli):
            acc = np.zeros((B, polys, n), dtype=object)
            for i, m in enumerate(row):
                s = m % t % q
                if s:
                    acc = (acc + s * xo[:, i, :, l, :]) % q
            out[:, j, :, l, :] = acc
    return out.astype(np.uint64)


@pytest.mark.parametrize("kind", ["random", "above_t", "worst", "zero"])
@pytest.mark.parametrize("dims", [(2, 4), (2, 1), (8, 16), (3, 5)])
@pytest.mark.parametrize("B,polys", [(1, 3), (3, 2)])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("n", [16, 1024])
def test_linear_map_bit_exact(ctxs, n, L, B, polys, dims, kind):
    ctx = ctxs(n, L)
    q, t = ctx.ct_moduli, T[L]
    d_in, d_out = dims
    rng = np.random.default_rng(zlib.crc32(repr((n, L, B, polys, dims, kind)).encode()))
    m = matrix_of(kind, d_out, d_in, t, rng)
    if kind == "worst":   # every term the largest possible: (t - 1) (q_l - 1)
        x = np.empty((B, d_in, polys, L, n), dtype=np.uint64)
        for l, ql in enumerate(q):
            x[..., l, :] = ql - 1
    else:
        x = uniform_residues(rng, (B, d_in, polys), q, n)
    got = ctx.dbfv_linear_map(m, x)
    assert got.shape == (B, d_out, polys, L, n)
    assert np.array_equal(got, bigint_map(m, x, q, t))
    if kind == "zero":
        assert not got.any()


# ---- the oracle composition: the literal sequence of advanced.rs

def scalar_plain_mul(ct, scalar):
    """advanced.rs:162-171."""
    prm = ct.params
    coeffs = [0] * prm.ring_degree
    coeffs[0] = scalar % prm.plain_modulus
    return obfv.bfv_plain_mul(ct, CoeffPoly(coeffs, prm.plain_modulus))


def oracle_change_base(limbs, dp, new_base, new_d):
    """advanced.rs:111-145."""
    p = (1 << 64) if dp.plain_modulus == 0 else dp.plain_modulus
    transform = [[0] * dp.num_digits for _ in range(new_d)]
    b_pow = 1
    for i in range(dp.num_digits):
        digits = odbfv.digit_decompose(b_pow % p, new_base, new_d)
        for j in range(new_d):
            transform[j][i] = digits[j]
        b_pow = b_pow * dp.base % p
    zero = obfv.bfv_sub(limbs[0], limbs[0])
    out = []
    for j in range(new_d):
        acc = zero
        for i in range(dp.num_digits):
            if transform[j][i] == 0:
                continue
            acc = obfv.bfv_add(acc, scalar_plain_mul(limbs[i], transform[j][i]))
        out.append(acc)
    return out


def oracle_div_by_base(limbs, dp):
    """advanced.rs:44-78."""
    d, t = dp.num_digits, dp.bfv_params.plain_modulus
    c0_div = scalar_plain_mul(limbs[0], pow(dp.base % t, -1, t))
    zero = obfv.bfv_sub(limbs[d - 1], limbs[d - 1])
    out = [zero] * d
    out[0] = obfv.bfv_add(limbs[1], c0_div) if d >= 2 else c0_div
    for i in range(1, d):
        out[i] = limbs[i + 1] if i + 1 < d else zero
    return out


@pytest.fixture(scope="module")
def sets(gpu_available):
    out = {}
    for name, dp in (("compact", P.compact_dbfv()), ("cfg4", P.cfg4_params(1024))):
        ctx = HipContext.from_params(dp.bfv_params)
        rng = np.random.default_rng(len(name))
        x = uniform_residues(rng, (1, dp.num_digits, 2), dp.bfv_params.ct_basis.moduli, dp.bfv_params.ring_degree)
        limbs = [np_to_ct(x[0, i], dp.bfv_params) for i in range(dp.num_digits)]
        out[name] = (dp, ctx, x, limbs)
    return out


@pytest.mark.parametrize("name,new_base,new_d", [("compact", 4, 4), ("compact", 3, 6), ("cfg4", 16, 4)])
def test_change_base_equals_oracle_composition(sets, name, new_base, new_d):
    dp, ctx, x, limbs = sets[name]
    got = ctx.dbfv_change_base(dp.num_digits, dp.base, dp.plain_modulus, new_base, new_d, x)
    want = np.stack([ct_to_np(c) for c in oracle_change_base(limbs, dp, new_base, new_d)])
    assert got.shape == (1, new_d, 2, ctx.L, ctx.n)
    assert np.array_equal(got[0], want)
    # and the same through the generic entry point with the host-built matrix
    m = _ffi.dbfv_change_base_matrix(dp.num_digits, dp.base, dp.plain_modulus, new_base, new_d)
    assert np.array_equal(ctx.dbfv_linear_map(m, x), got)


@pytest.mark.parametrize("name", ["compact", "cfg4"])
def test_div_by_base_equals_oracle_composition(sets, name):
    dp, ctx, x, limbs = sets[name]
    got, new_plain = ctx.dbfv_div_by_base(dp.num_digits, dp.base, dp.plain_modulus, x)
    want = np.stack([ct_to_np(c) for c in oracle_div_by_base(limbs, dp)])
    assert np.array_equal(got[0], want)
    assert new_plain == dp.plain_modulus // dp.base
    assert not got[0, -1].any()


def test_div_by_base_single_digit(sets):
    """d = 1: the one limb is base^-1 c_0 (advanced.rs:67-71)."""
    dp, ctx, x, limbs = sets["compact"]
    got, new_plain = ctx.dbfv_div_by_base(1, 16, 16, x[:, :1])
    want = ct_to_np(scalar_plain_mul(limbs[0], pow(16, -1, 929)))
    assert np.array_equal(got[0, 0], want) and new_plain == 1


# ---- semantics on real encryptions (advanced.rs:183-221)

@pytest.fixture(scope="module")
def real(gpu_available):
    dp = P.compact_dbfv()
    ctx = HipContext.from_params(dp.bfv_params)
    sk = ctx.gen_secret_key(KEY, stream=1)
    return dp, ctx, sk


def test_div_by_base_divides_plaintext_and_modulus(real):
    dp, ctx, sk = real
    ct = ctx.dbfv_encrypt_sk(2, 16, 256, [48, 240], sk, KEY, stream=2)
    out, new_plain = ctx.dbfv_div_by_base(2, 16, 256, ct)
    assert new_plain == 16
    assert [int(v) for v in ctx.dbfv_decrypt(2, 16, new_plain, out, sk)] == [3, 15]
    lim = [np_to_ct(out[0, k], dp.bfv_params) for k in range(2)]
    osk = obfv.SecretKey(np_to_rns(sk, dp.bfv_params.ct_basis), dp.bfv_params, None)
    oct_ = odbfv.DbfvCiphertext(lim, 1, 0, P.DbfvParams(dp.bfv_params, 16, 2, 16))
    assert odbfv.dbfv_decrypt_scalar(oct_, osk) == 3


def test_change_base_preserves_values(real):
    dp, ctx, sk = real
    values = [0, 1, 15, 42, 127, 255]
    ct = ctx.dbfv_encrypt_sk(2, 16, 256, values, sk, KEY, stream=3)
    out = ctx.dbfv_change_base(2, 16, 256, 4, 4, ct)
    assert [int(v) for v in ctx.dbfv_decrypt(4, 4, 256, out, sk)] == values
    out = ctx.dbfv_change_base(2, 16, 256, 3, 6, ct)
    assert [int(v) for v in ctx.dbfv_decrypt(6, 3, 256, out, sk)] == values


def test_automorphism_preserves_scalar(real):
    dp, ctx, sk = real
    gk = ctx.gen_galois_key(sk, 3, KEY, stream=4)
    ct = ctx.dbfv_encrypt_sk(2, 16, 256, [42], sk, KEY, stream=5)
    out = ctx.dbfv_apply_automorphism(ct, 3, gk)
    assert [int(v) for v in ctx.dbfv_decrypt(2, 16, 256, out, sk)] == [42]


# ---- the limb-wise wrappers equal the BFV entry points on the [B * d] batch

@pytest.fixture(scope="module")
def limbwise(gpu_available):
    prm = P.compact_dbfv().bfv_params
    ctx = HipContext.from_params(prm)
    rng = np.random.default_rng(11)
    q, n = prm.ct_basis.moduli, prm.ring_degree
    ctx.load_relin_key(uniform_residues(rng, (prm.gadget_digits, 2), q, n))
    B, d = 3, 2
    data = {p: uniform_residues(rng, (B, d, p), q, n) for p in (2, 3)}
    data["b2"] = uniform_residues(rng, (B, d, 2), q, n)
    data["gk"] = uniform_residues(rng, (prm.gadget_digits, 2), q, n)
    return ctx, data, B, d


def flat(x):
    return x.reshape((-1,) + x.shape[2:])


def test_add_sub_neg_equal_per_limb_bfv(limbwise):
    ctx, data, B, d = limbwise
    for a, b in ((data[2], data["b2"]), (data[2], data[3]), (data[3], data[2])):
        got, _ = ctx.dbfv_add(a, b)
        assert np.array_equal(flat(got), ctx.bfv_add(flat(a), flat(b)))
        got, _ = ctx.dbfv_sub(a, b)
        assert np.array_equal(flat(got), ctx.bfv_sub(flat(a), flat(b)))
    for p in (2, 3):
        assert np.array_equal(flat(ctx.dbfv_neg(data[p])), ctx.bfv_neg(flat(data[p])))


def test_relinearize_equals_per_limb_bfv(limbwise):
    ctx, data, B, d = limbwise
    got = ctx.dbfv_relinearize(data[3])
    assert got.shape == (B, d, 2, ctx.L, ctx.n)
    assert np.array_equal(flat(got), ctx.relinearize(flat(data[3])))
    assert np.array_equal(ctx.dbfv_relinearize(data[2]), data[2])   # polys < 3: cloned


def test_apply_automorphism_equals_per_limb_bfv(limbwise):
    ctx, data, B, d = limbwise
    got = ctx.dbfv_apply_automorphism(data[2], 5, data["gk"])
    assert np.array_equal(flat(got), ctx.bfv_apply_automorphism(flat(data[2]), 5, data["gk"]))


def test_depth_out_is_the_max(limbwise):
    ctx, data, B, d = limbwise
    _, dout = ctx.dbfv_add(data[2], data["b2"], depth_a=[0, 1, 2], depth_b=[1, 0, 2])
    assert list(dout) == [1, 1, 2]
    _, dout = ctx.dbfv_sub(data[2], data["b2"], depth_a=[3, 0, 0])   # NULL depth_b = 0
    assert list(dout) == [3, 0, 0]
    _, dout = ctx.dbfv_add(data[2], data["b2"])
    assert list(dout) == [0, 0, 0]


def test_device_forms(limbwise):
    import torch
    ctx, data, B, d = limbwise
    dev = torch.device("cuda:0")

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)

    def down(tn):
        return tn.cpu().numpy().view(np.uint64)

    a, b = up(data[2]), up(data["b2"])
    out = torch.zeros_like(a)
    dout = ctx.dbfv_add_dev(a, d, 2, b, d, 2, out, B, depth_a=[0, 1, 0])
    ctx.synchronize()
    assert np.array_equal(down(out), ctx.dbfv_add(data[2], data["b2"])[0]) and list(dout) == [0, 1, 0]
    wide = torch.zeros((B, 4, 2, ctx.L, ctx.n), dtype=torch.int64, device=dev)
    ctx.dbfv_change_base_dev(2, 16, 256, 4, 4, a, wide, B)
    ctx.synchronize()
    assert np.array_equal(down(wide), ctx.dbfv_change_base(2, 16, 256, 4, 4, data[2]))
    assert ctx.dbfv_div_by_base_dev(2, 16, 256, a, out, B) == 16
    ctx.synchronize()
    assert np.array_equal(down(out), ctx.dbfv_div_by_base(2, 16, 256, data[2])[0])
    with pytest.raises(ExactoError) as e:      # out must not alias in
        ctx.dbfv_linear_map_dev([[1, 0], [0, 1]], 2, a, a, B)
    assert e.value.variant == "InvalidParam" and "must not overlap" in str(e.value)


# ---- error paths, by variant and message

def raises(variant, text, fn, *args, **kw):
    with pytest.raises(ExactoError) as e:
        fn(*args, **kw)
    assert e.value.variant == variant
    assert text in str(e.value), str(e.value)


def test_limbwise_errors(limbwise, ctxs):
    ctx, data, B, d = limbwise
    three = np.concatenate([data[2], data[2][:, :1]], axis=1)            # d = 3
    raises("DimensionMismatch", "dimension mismatch: expected 2, got 3", ctx.dbfv_add, data[2], three)
    raises("DimensionMismatch", "dimension mismatch: expected 3, got 2", ctx.dbfv_sub, three, data[2])
    four = np.concatenate([data[3], data[3][:, :, :1]], axis=2)          # polys = 4
    raises("InvalidParam", "relinearization only supports degree-2 ciphertexts", ctx.dbfv_relinearize, four)
    raises("InvalidParam", "automorphism requires degree-1 ciphertext", ctx.dbfv_apply_automorphism, data[3], 3,
           data["gk"])
    raises("InvalidParam", "galois key is empty", ctx.dbfv_apply_automorphism, data[2], 3,
           np.zeros((0, 2, ctx.L, ctx.n), dtype=np.uint64))
    nokey = ctxs(1024, 1)                                                # a context without a resident key
    raises("MissingKey", "relinearization key not loaded", nokey.dbfv_relinearize, data[3])


def test_linear_map_errors(limbwise):
    ctx, data, B, d = limbwise
    x = data[2]
    raises("InvalidParam", "new base must be >= 2", ctx.dbfv_change_base, 2, 16, 256, 1, 4, x)
    raises("InvalidParam", "new_num_digits must be >= 1", ctx.dbfv_change_base, 2, 16, 256, 4, 0, x)
    raises("InvalidParam", "base^digits = 64 < plain_modulus = 256", ctx.dbfv_change_base, 2, 16, 256, 4, 3, x)
    raises("InvalidParam", "base^digits = 16 < plain_modulus = 256", ctx.dbfv_change_base, 1, 16, 256, 4, 4, x[:, :1])
    raises("InvalidParam", "base not invertible modulo BFV plaintext modulus", ctx.dbfv_div_by_base, 1, 929, 929,
           x[:, :1])
    raises("InvalidParam", "plaintext modulus 250 is not divisible by base 16", ctx.dbfv_div_by_base, 2, 16, 250, x)
    wide = np.zeros((1, 41, 2, ctx.L, ctx.n), dtype=np.uint64)
    raises("InvalidParam", "plaintext modulus 18446744073709551616 is not divisible by base 3", ctx.dbfv_div_by_base,
           41, 3, 0, wide)
    raises("InvalidParam", "base^digits = 16 < plain_modulus = 256", ctx.dbfv_div_by_base, 1, 16, 256, x[:, :1])

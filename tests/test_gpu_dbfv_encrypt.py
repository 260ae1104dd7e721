"""dBFV encryption on the GPU: exacto_dbfv_encrypt_{sk,pk} and exacto_dbfv_encrypt_poly_{sk,pk}
(dbfv/encrypt.rs:17-141).

The randomness contract makes the result testable bit for bit: limb k of item b is item b*d + k of
exacto_encrypt_{sk,pk} called with the same (key, stream, sigma) on the [B*d][n] digit plaintexts,
which this file builds on the host with the oracle's digit_decompose.  The values then go round
through the GPU decryptors and the oracle's.
"""
import numpy as np
import pytest

from oracle import bfv as obfv, dbfv as odbfv, params as P
from exacto_amd._ffi import HipContext, ExactoError
from bridge import np_to_ct, np_to_rns

pytestmark = pytest.mark.gpu

KEY = [0x243F6A8885A308D3, 0x13198A2E03707344, 0xA4093822299F31D0, 0x082EFA98EC4E6C89]


class Case:
    """One parameter set with its context and keys (made once per module)."""

    def __init__(self, bfv, base, d, plain):
        self.bfv, self.base, self.d, self.plain = bfv, base, d, plain
        self.ctx = HipContext.from_params(bfv)
        self.n = bfv.ring_degree
        self.sk = self.ctx.gen_secret_key(KEY, stream=1)
        self.pk = self.ctx.gen_public_key(self.sk, KEY, stream=2)

    @property
    def args(self):
        return self.d, self.base, self.plain

    def reduce(self, v):
        return int(v) if self.plain == 0 else int(v) % self.plain

    def scalar_digit_pts(self, values):
        """[B*d][n]: digit k of value b as the constant polynomial (encrypt.rs:105-118)."""
        pt = np.zeros((len(values) * self.d, self.n), dtype=np.uint64)
        for b, v in enumerate(values):
            pt[b * self.d:(b + 1) * self.d, 0] = odbfv.digit_decompose(self.reduce(v), self.base, self.d)
        return pt

    def poly_digit_pts(self, pts):
        """[B*d][n]: polynomial of the k-th digits of item b (poly_digit_decompose)."""
        out = np.zeros((pts.shape[0], self.d, self.n), dtype=np.uint64)
        for b in range(pts.shape[0]):
            for j in range(self.n):
                out[b, :, j] = odbfv.digit_decompose(self.reduce(pts[b, j]), self.base, self.d)
        return out.reshape(-1, self.n)


@pytest.fixture(scope="module")
def cases(gpu_available):
    compact, u64 = P.compact_dbfv(), P.u64_dbfv()
    return {
        "compact": Case(compact.bfv_params, compact.base, compact.num_digits, compact.plain_modulus),
        "u64": Case(u64.bfv_params, u64.base, u64.num_digits, u64.plain_modulus),
        # a base that is no power of two, over compact_dbfv's BFV parameters (t = 929 >= 10)
        "base10": Case(compact.bfv_params, 10, 3, 1000),
    }


def scalar_values(name):
    if name == "u64":
        return [0, (1 << 64) - 1, 0x9E3779B97F4A7C15]
    if name == "base10":
        return [0, 999, 1234567]          # the last is reduced mod 1000
    return [0, 255, 300]                  # 300 is reduced mod 256


@pytest.mark.parametrize("name", ["compact", "u64", "base10"])
def test_scalar_encrypt_equals_bfv_encrypt_of_host_digits(cases, name):
    c = cases[name]
    values = scalar_values(name)
    pts = c.scalar_digit_pts(values)
    got = c.ctx.dbfv_encrypt_sk(*c.args, values, c.sk, KEY, stream=21)
    want = c.ctx.encrypt_sk(pts, c.sk, KEY, stream=21)
    assert got.shape == (len(values), c.d, 2, c.ctx.L, c.n)
    assert np.array_equal(got.reshape(want.shape), want)
    got = c.ctx.dbfv_encrypt_pk(*c.args, values, c.pk, KEY, stream=22)
    want = c.ctx.encrypt_pk(pts, c.pk, KEY, stream=22)
    assert np.array_equal(got.reshape(want.shape), want)


@pytest.mark.parametrize("name", ["compact", "base10"])
def test_poly_encrypt_equals_bfv_encrypt_of_host_digits(cases, name):
    c = cases[name]
    rng = np.random.default_rng(7)
    B = 3
    pts = rng.integers(0, c.plain, size=(B, c.n), dtype=np.uint64)
    pts[0, :4] = [c.plain - 1, 0, c.plain + 5, (1 << 64) - 1]   # coefficients >= p are reduced
    dig = c.poly_digit_pts(pts)
    got = c.ctx.dbfv_encrypt_poly_sk(*c.args, pts, c.sk, KEY, stream=31)
    want = c.ctx.encrypt_sk(dig, c.sk, KEY, stream=31)
    assert np.array_equal(got.reshape(want.shape), want)
    got = c.ctx.dbfv_encrypt_poly_pk(*c.args, pts, c.pk, KEY, stream=32)
    want = c.ctx.encrypt_pk(dig, c.pk, KEY, stream=32)
    assert np.array_equal(got.reshape(want.shape), want)


def oracle_ct(c, ct_np):
    prm = P.DbfvParams(c.bfv, c.base, c.d, c.plain)
    return odbfv.DbfvCiphertext([np_to_ct(ct_np[k], c.bfv) for k in range(c.d)], c.d, 0, prm)


def oracle_sk(c):
    return obfv.SecretKey(np_to_rns(c.sk, c.bfv.ct_basis), c.bfv, None)


@pytest.mark.parametrize("name", ["compact", "u64", "base10"])
def test_scalar_round_trip(cases, name):
    c = cases[name]
    values = scalar_values(name)
    want = np.array([c.reduce(v) for v in values], dtype=np.uint64)
    ct_sk = c.ctx.dbfv_encrypt_sk(*c.args, values, c.sk, KEY, stream=41)
    ct_pk = c.ctx.dbfv_encrypt_pk(*c.args, values, c.pk, KEY, stream=42)
    for ct in (ct_sk, ct_pk):
        assert np.array_equal(c.ctx.dbfv_decrypt(*c.args, ct, c.sk), want)
    if name != "u64":   # the oracle decryptor in Python: the n = 1024 sets
        sk = oracle_sk(c)
        for b in range(len(values)):
            assert odbfv.dbfv_decrypt_scalar(oracle_ct(c, ct_sk[b]), sk) == int(want[b])
        assert odbfv.dbfv_decrypt_scalar(oracle_ct(c, ct_pk[1]), sk) == int(want[1])


@pytest.mark.parametrize("name", ["compact", "base10"])
def test_poly_round_trip_reduces_coefficients(cases, name):
    c = cases[name]
    rng = np.random.default_rng(9)
    pts = rng.integers(0, 1 << 63, size=(2, c.n), dtype=np.uint64)   # nearly all >= p
    pts[1, :3] = [0, c.plain - 1, c.plain]
    want = pts % np.uint64(c.plain)
    ct_sk = c.ctx.dbfv_encrypt_poly_sk(*c.args, pts, c.sk, KEY, stream=51)
    ct_pk = c.ctx.dbfv_encrypt_poly_pk(*c.args, pts, c.pk, KEY, stream=52)
    for ct in (ct_sk, ct_pk):
        assert np.array_equal(c.ctx.dbfv_decrypt_poly(*c.args, ct, c.sk), want)
    got = odbfv.dbfv_decrypt_poly(oracle_ct(c, ct_sk[1]), oracle_sk(c))
    assert got == [int(v) for v in want[1]]


def test_device_form_equals_host_form(cases):
    import torch
    c = cases["compact"]
    values = [42, 255, 7]
    want = c.ctx.dbfv_encrypt_sk(*c.args, values, c.sk, KEY, stream=61)
    dev = torch.device("cuda:0")
    v = torch.from_numpy(np.array(values, dtype=np.uint64).view(np.int64)).to(dev)
    sk = torch.from_numpy(c.sk.view(np.int64)).to(dev)
    ct = torch.zeros(want.shape, dtype=torch.int64, device=dev)
    c.ctx.dbfv_encrypt_sk_dev(*c.args, v, sk, KEY, 61, ct, len(values))
    c.ctx.synchronize()
    assert np.array_equal(ct.cpu().numpy().view(np.uint64), want)


def test_errors(cases):
    c = cases["compact"]
    with pytest.raises(ExactoError) as e:     # base 1024 > t = 929 (1024^1 >= 256 passes DbfvParams::new)
        c.ctx.dbfv_encrypt_sk(1, 1024, 256, [1], c.sk, KEY)
    assert e.value.variant == "InvalidParam"
    assert str(e.value) == "invalid parameter: dBFV base 1024 must be <= BFV plaintext modulus 929"
    with pytest.raises(ExactoError) as e:
        c.ctx.dbfv_encrypt_pk(1, 1024, 256, [1], c.pk, KEY)
    assert "dBFV base 1024 must be <= BFV plaintext modulus 929" in str(e.value)
    pt = np.zeros((1, c.n), dtype=np.uint64)
    for fn, key in ((c.ctx.dbfv_encrypt_poly_sk, c.sk), (c.ctx.dbfv_encrypt_poly_pk, c.pk)):
        with pytest.raises(ExactoError) as e:
            fn(16, 16, 0, pt, key, KEY)
        assert e.value.variant == "InvalidParam"
        assert str(e.value) == ("invalid parameter: polynomial dBFV plaintext requires finite plain_modulus "
                                "(plain_modulus=0 is scalar-only)")
    with pytest.raises(ExactoError) as e:     # DbfvParams::new runs first
        c.ctx.dbfv_encrypt_sk(1, 16, 256, [1], c.sk, KEY)
    assert str(e.value) == "invalid parameter: base^digits = 16 < plain_modulus = 256"

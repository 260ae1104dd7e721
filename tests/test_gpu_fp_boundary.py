"""The float-sum scale paths (kernels.hip fpq_y / fpq_acc / fpq_flush, fpc_lift, ks32_fpc_one) on the GPU
at their centring boundary, at the library's default band (fpq_lim = 1/2 - 2^-40): tests/fp_boundary.py
puts s = [p T]_Q within a few units (and within 2^-45 Q, 2^-41 Q) of +-Q/2 in most lanes of a wave, where
the lane must take the Garner fallback, and just outside the band, at 0 and at Q - 1 in the others, where it
must not; tests/test_fp_boundary_inputs.py shows on the CPU model that the lanes split that way and that a
kernel ignoring the band would centre some of them wrongly.  Also the limb counts L = 2, 5, 6 of the
30-bit-limb scale / lift kernels, and special primes at the bottom of their window (d = 2^60 - q about
2^23.9, where the special-prime bounds are tight).

Everything is bit-exact against the Python oracle (n <= 1024), the C restatement (n = 4096, computed in
the test) or its committed digest (n = 8192, tests/golden/make_golden.py --boundary-digests), and for
bfv_mul_no_relin also against a closed form that does not go through the oracle's tensor.  No selection
switch may be set: this file is about the default selection.

The CPU restatements of the same arithmetic: tests/test_fpq.py, tests/test_fpc_crt.py, tests/test_ks32_fpc.py.
"""

import json
import os

import numpy as np
import pytest

from oracle import params as P, cref
from exacto_amd._ffi import HipContext, PATH_EXACT_RNS
from test_gpu_bfv import oracle_mul, random_case
from test_gpu_variants import SWITCHES
from test_gpu_worstcase import pad
import fp_boundary as F

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

assert not [k for k in SWITCHES if k in os.environ], "selection switches set: not the default band"


def check_bfv(prm, ct1, ct2, rlk, want3, want2, pad_to=0, want_pad=None):
    """bfv_mul_no_relin == want3, bfv_mul_and_relin == want2 and relinearize(no_relin) == and_relin on
    item 0; with pad_to, uniform items fill the batch (both pipeline lanes) and items 1, 2 are compared too."""
    q, n = prm.ct_basis.moduli, prm.ring_degree
    ctx = HipContext.from_params(prm)
    assert ctx.path == PATH_EXACT_RNS and ctx.num_internal_aux == len(q) + 1
    ctx.load_relin_key(rlk)
    c1, c2 = pad(ct1, ct2, pad_to, q, n, 5)
    got3 = ctx.bfv_mul_no_relin(c1, c2)
    got2 = ctx.bfv_mul_and_relin(c1, c2)
    for w in want3:
        assert np.array_equal(got3[:1], w)
    assert np.array_equal(got2[:1], want2)
    assert np.array_equal(ctx.relinearize(got3), got2)
    if want_pad is not None:
        assert np.array_equal(got2[1:3], want_pad(c1[1:3], c2[1:3]))
    return ctx


# ---------------------------------------------------------------- bfv, cfg3's basis, default band

@pytest.mark.parametrize("which", ["c0c1", "c1c2"])
@pytest.mark.parametrize("n", [64, 1024])
def test_bfv_boundary_cfg3_small(gpu_available, n, which):
    prm = P.cfg3_params(n)
    ct1, ct2, coeffs = F.bfv_case(prm, which)
    rlk = F.uniform_key(prm)
    want3 = [oracle_mul(prm, ct1, ct2, rlk, relin=False), F.closed_form(prm, coeffs, which)]
    check_bfv(prm, ct1, ct2, rlk, want3, oracle_mul(prm, ct1, ct2, rlk))


@pytest.mark.parametrize("which", ["c0c1", "c1c2"])
def test_bfv_boundary_cfg3_full(gpu_available, which):
    """n = 4096 in a batch of 200 products (two pipeline lanes of 100), two uniform items compared too."""
    prm = P.cfg3_params(4096)
    ct1, ct2, coeffs = F.bfv_case(prm, which)
    rlk = F.uniform_key(prm)
    want3 = [cref.bfv_mul(prm, ct1, ct2, None, relin=False, threads=8), F.closed_form(prm, coeffs, which)]
    ctx = check_bfv(prm, ct1, ct2, rlk, want3, cref.bfv_mul_and_relin(prm, ct1, ct2, rlk, threads=8), pad_to=200,
                    want_pad=lambda a, b: cref.bfv_mul_and_relin(prm, a, b, rlk, threads=8))
    assert ctx.ks32_primes == 3


# ---------------------------------------------------------------- L = 2, 5, 6

@pytest.mark.parametrize("n", [64, 1024])
@pytest.mark.parametrize("L", [2, 5, 6])
def test_limb_counts_uniform(gpu_available, L, n):
    prm = F.low_params(n, L, 65537)
    ct1, ct2, rlk = random_case(prm, 2, 100 * L + n)
    ctx = HipContext.from_params(prm)
    assert ctx.path == PATH_EXACT_RNS and ctx.num_internal_aux == L + 1
    ctx.load_relin_key(rlk)
    got3, got2 = ctx.bfv_mul_no_relin(ct1, ct2), ctx.bfv_mul_and_relin(ct1, ct2)
    assert np.array_equal(got3, oracle_mul(prm, ct1, ct2, rlk, relin=False))
    assert np.array_equal(got2, oracle_mul(prm, ct1, ct2, rlk))
    assert np.array_equal(ctx.relinearize(got3), got2)


@pytest.mark.parametrize("which", ["c0c1", "c1c2"])
@pytest.mark.parametrize("n", [64, 1024])
@pytest.mark.parametrize("L", [2, 5, 6])
def test_limb_counts_boundary(gpu_available, L, n, which):
    prm = F.low_params(n, L, 65537)
    ct1, ct2, coeffs = F.bfv_case(prm, which)
    rlk = F.uniform_key(prm)
    want3 = [oracle_mul(prm, ct1, ct2, rlk, relin=False), F.closed_form(prm, coeffs, which)]
    check_bfv(prm, ct1, ct2, rlk, want3, oracle_mul(prm, ct1, ct2, rlk))


# ---------------------------------------------------------------- the bottom of the special window

@pytest.mark.parametrize("kind", ["uniform", "c0c1", "c1c2"])
def test_low_window_cfg3_shape(gpu_available, kind):
    """n = 4096 over the three lowest special primes == 1 mod 16384 (p = 65537, G = 12): cfg3's shape."""
    prm = F.low_params(4096, 3, 65537)
    assert prm.gadget_digits == 12
    if kind == "uniform":
        ct1, ct2, rlk = random_case(prm, 1, 61)
    else:
        ct1, ct2, _ = F.bfv_case(prm, kind)
        rlk = F.uniform_key(prm)
    want = cref.bfv_mul_and_relin(prm, ct1, ct2, rlk, threads=8)
    ctx = HipContext.from_params(prm)
    assert ctx.path == PATH_EXACT_RNS and ctx.num_internal_aux == 4 and ctx.ks32_primes == 3
    ctx.load_relin_key(rlk)
    assert np.array_equal(ctx.bfv_mul_and_relin(ct1, ct2), want)


def digest_case(name):
    with open(os.path.join(GOLD, "digests.json")) as f:
        spec = json.load(f)[name]
    prm, x, y, rlk = F.digest_inputs(name)
    assert F.sha(np.concatenate([x.ravel(), y.ravel(), rlk.ravel()])) == spec["sha256_inputs"]
    return spec, prm, x, y, rlk


def test_low_window_cfg5_shape(gpu_available):
    """n = 8192 over the four lowest special primes (p = 1040407, base 256): cfg5's bfv shape, B = 1."""
    spec, prm, ct1, ct2, rlk = digest_case("boundary_low4_bfv")
    ctx = HipContext.from_params(prm)
    assert ctx.path == PATH_EXACT_RNS and ctx.num_internal_aux == 5
    ctx.load_relin_key(rlk)
    assert F.sha(ctx.bfv_mul_and_relin(ct1, ct2)[:1]) == spec["sha256_out"]


# ---------------------------------------------------------------- dbfv: psum

@pytest.mark.parametrize("basis", ["cfg4", "low3"])
def test_dbfv_boundary_cfg4(gpu_available, basis):
    """A psum row adds Garner-fallback products and fpq_flush'ed products into one carry; over cfg4's basis
    and over the three lowest special primes with cfg4's dBFV parameters (fpq_flush with d about 2^24).
    64 items: 192 products, two lanes."""
    dp = P.cfg4_params(4096)
    if basis == "low3":
        dp = P.DbfvParams(F.low_params(4096, 3, dp.bfv_params.plain_modulus), dp.base, dp.num_digits,
                          dp.plain_modulus)
    prm = dp.bfv_params
    q, n, d = prm.ct_basis.moduli, 4096, dp.num_digits
    a, b, rlk = F.dbfv_case(dp)
    want = cref.dbfv_mul(dp, a, b, rlk, threads=8)
    ctx = HipContext.from_params(prm)
    assert ctx.psum_max >= 2
    ctx.load_relin_key(rlk)
    a2, b2 = pad(a, b, 64, q, n, 6)
    out, _ = ctx.dbfv_mul(d, dp.base, dp.plain_modulus, a2, b2)
    assert np.array_equal(out[:1], want)


def test_dbfv_boundary_cfg5(gpu_available):
    """cfg5 (n = 8192, d = 8: limb 7 sums 8 products) in the bench's batch of 8, pinned by digest."""
    spec, dp, a, b, rlk = digest_case("boundary_cfg5_dbfv")
    prm = dp.bfv_params
    ctx = HipContext.from_params(prm)
    assert ctx.psum_max >= 8
    ctx.load_relin_key(rlk)
    a2, b2 = pad(a, b, 8, prm.ct_basis.moduli, spec["n"], 7)
    out, _ = ctx.dbfv_mul(dp.num_digits, dp.base, dp.plain_modulus, a2, b2)
    assert F.sha(out[:1]) == spec["sha256_out"]

"""CPU check that tests/fp_boundary.py's inputs do what tests/test_gpu_fp_boundary.py relies on, at every
basis that file runs: the model of the kernel's float sum (tests/test_fpq.py) sends the near-+-Q/2 lanes
to the Garner fallback and the others to the fast path, both in numbers within one wave; the fast path's
arithmetic holds on every lane; ignoring the band would centre some lane wrongly (so a kernel without
the band, or with the comparison reversed, returns a coefficient off by one); the closed form the GPU test
compares with equals the oracle's bfv_mul_no_relin; and the context's auxiliary basis keeps the special
path (K = L + 1, every prime above 2^60 - 2^24).

A Python restatement of the device arithmetic, not the kernel: the kernel runs in
tests/test_gpu_fp_boundary.py."""
import math
import random

import numpy as np
import pytest

from oracle import bfv as obfv, params as P
from bridge import ct_to_np, np_to_ct
from test_fpc_crt import Q3, Q4, aux_basis
from test_fpq import check, consts, fpq
import fp_boundary as F

LOW4 = F.low_window_primes(16384, 4)
LOW6 = F.low_window_primes(2048, 6)
# name: (n, plaintext modulus, ciphertext primes)
BASES = {
    "cfg3": (4096, 65537, Q3), "cfg4": (4096, 260111, Q3), "cfg5": (8192, 1040407, Q4),
    "low3": (4096, 65537, LOW4[:3]), "low3_cfg4": (4096, 260111, LOW4[:3]), "low4": (8192, 1040407, LOW4),
    "L2": (1024, 65537, LOW6[:2]), "L5": (1024, 65537, LOW6[:5]), "L6": (1024, 65537, LOW6),
}
SIZES = {name: sorted({64, 1024, n}) for name, (n, _, _) in BASES.items()}


def test_low_window_search():
    assert LOW4 == F.LOW_16384 and LOW6 == F.LOW_2048
    for q in LOW4 + LOW6:
        assert F.WINDOW_LO < q < F.WINDOW_LO + (1 << 21)          # 2^23.8 < d = 2^60 - q < 2^24
    assert all(q % 16384 == 1 for q in LOW4) and all(q % 2048 == 1 for q in LOW6)


@pytest.mark.parametrize("name", sorted(BASES))
def test_band_decision_per_boundary_value(name):
    """(a) and (d): the model's decision on every boundary value, and the wrong beta without the band."""
    _, p, qs = BASES[name]
    Q = math.prod(qs)
    pz = F.pz_consts(qs, p)
    pinv = pow(p, -1, Q)
    wrong = 0
    for s, kind in F.boundary_values(Q):
        x = F.centre(s * pinv % Q, Q)
        assert F.in_band(qs, p, [x]) == [kind == "band"], (name, s - Q // 2, kind)
        z, f, b = fpq([x % q for q in qs], qs, pz)
        got = sum(zi * (Q // q) for zi, q in zip(z, qs)) - int(b) * Q
        if kind == "fast":
            assert got == F.centre(s, Q)
        else:
            wrong += got != F.centre(s, Q)
    assert wrong >= 1, name


@pytest.mark.parametrize("name", sorted(BASES))
def test_every_lane_and_lane_counts(name):
    """(b) and (c): test_fpq.check on every lane of every polynomial size the GPU test uses."""
    n_ctx, p, qs = BASES[name]
    rng = random.Random(3)
    for n in SIZES[name]:
        if n > n_ctx:
            continue
        c = consts(n, p, qs)
        A = F.boundary_poly(qs, p, n, 41)
        band = F.in_band(qs, p, A)
        for j, x in enumerate(A):
            Ta = [rng.randrange(2 * pa) for pa in c[0]]
            assert check([x % q for q in qs], Ta, p, qs, c) == (not band[j]), (name, n, j)
            if not F.boundary_lane(j, n):
                assert not band[j]
        assert sum(band) >= 32 and sum(not b for b in band[:64]) >= 16, (name, n, sum(band))
        # lanes 0..63: one wave with both paths
        assert 16 <= sum(band[:64]) <= 48


@pytest.mark.parametrize("which", ["c0c1", "c1c2"])
@pytest.mark.parametrize("name", sorted(BASES))
def test_closed_form_is_the_oracle(name, which):
    """(e): at n = 64 the Python oracle's bfv_mul_no_relin equals the closed form."""
    _, p, qs = BASES[name]
    prm = P.BfvParamsBuilder().ring_degree(64).plain_modulus(p).ct_moduli(qs).build()
    ct1, ct2, coeffs = F.bfv_case(prm, which)
    want = ct_to_np(obfv.bfv_mul_no_relin(np_to_ct(ct1[0], prm), np_to_ct(ct2[0], prm)))
    assert np.array_equal(F.closed_form(prm, coeffs, which)[0], want)


@pytest.mark.parametrize("name", sorted(BASES))
def test_aux_basis_keeps_the_special_path(name):
    """(f): K = L + 1 auxiliary primes, all in the special window, at every ring degree used."""
    n_ctx, p, qs = BASES[name]
    for n in SIZES[name]:
        if n > n_ctx:
            continue
        ps = aux_basis(n, p, qs)
        assert len(ps) == len(qs) + 1, (name, n, ps)
        assert min(ps) > F.WINDOW_LO and not set(ps) & set(qs)


def test_closed_form_is_the_oracle_above_schoolbook_size():
    """n = 128: the oracle's Kronecker product (n > 64) with ct2's zero component."""
    prm = P.cfg3_params(128)
    for which in ("c0c1", "c1c2"):
        ct1, ct2, coeffs = F.bfv_case(prm, which)
        want = ct_to_np(obfv.bfv_mul_no_relin(np_to_ct(ct1[0], prm), np_to_ct(ct2[0], prm)))
        assert np.array_equal(F.closed_form(prm, coeffs, which)[0], want)


@pytest.mark.parametrize("name", ["boundary_cfg5_dbfv", "boundary_low4_bfv"])
def test_digest_inputs_reproduce(name):
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "digests.json")) as f:
        spec = json.load(f)[name]
    prm, x, y, rlk = F.digest_inputs(name)
    assert x.shape[-1] == spec["n"] == 8192
    assert F.sha(np.concatenate([x.ravel(), y.ravel(), rlk.ravel()])) == spec["sha256_inputs"]
    assert len(spec["sha256_out"]) == 64


def test_dbfv_case_layout():
    dp = P.cfg4_params(64)
    a, b, rlk = F.dbfv_case(dp)
    prm = dp.bfv_params
    assert a.shape == b.shape == (1, dp.num_digits, 2, 3, 64) and rlk.shape == (prm.gadget_digits, 2, 3, 64)
    assert np.array_equal(a[0, 0, 0], a[0, 1, 1]) and np.array_equal(a[0, 0, 1], a[0, 1, 0])
    assert not np.array_equal(a[0, 0, 0], a[0, 0, 1])
    assert (b[0, :, 0] == 1).all() and (b[0, :, 1] == 0).all()

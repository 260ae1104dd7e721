"""The scale's CRT factors folded into the tensor's last inverse stage (EXACTO_CRT_FOLD) on the GPU, at the
smallest shape that reaches the folded kernels: n = 4096 over cfg3's three moduli, p = 65537, base 2^16.

The tensor's last stage leaves z_i = T_i p (Q / q_i)^-1 and T_a fpc_pq[a] in [0, 2q), which the scale reads
without its own products (kernels.hip fpq_y FOLD); a lane whose [p T]_Q lies within 2^-40 Q of +-Q/2 goes to
Garner over Q after one Shoup product back from z_i (fpc_y_garner FOLD).

bfv_mul_and_relin_dev and bfv_mul_no_relin against the C restatement of the reference (oracle.cref), B = 2
in one chunk and B = 5 in chunks of 2 (both lanes, a short last chunk), on
  (a) uniform inputs,
  (b) ct1 and ct2 whose coefficients sit on the input lift's centring boundary, +-floor(Q/2) and its
      neighbours, in the lanes fp_boundary.py uses (the lift is Garner over Q: both signs in one wave),
  (c) fp_boundary.bfv_case inputs: the scale's boundary, [p T]_Q next to +-Q/2; the CPU model
      (tests/test_fpq.py, whose band tests/test_crt_fold.py shows the folded form keeps) says that one wave
      holds lanes of both kinds.
One dbfv_mul at cfg4's parameters (d = 2): the psum readers of the tensor keep the unfolded form."""

import math
import random

import numpy as np
import pytest
import torch

from oracle import params as P, cref
from exacto_amd._ffi import HipContext, PATH_EXACT_RNS
from bridge import uniform_residues
import fp_boundary as F

pytestmark = pytest.mark.gpu

N, B = 4096, 5


def lift_boundary_poly(moduli, n, seed):
    """Centred coefficients: +-(floor(Q/2) - 3 .. floor(Q/2) + 3) mod Q, +-(floor(Q/2) - (Q >> e)) for
    fp_boundary's e = 45 and 38, then 0, 1, -1, cycled over the lanes of fp_boundary.boundary_lane; a uniform
    residue elsewhere."""
    Q = math.prod(moduli)
    h = Q // 2
    vals = [h + k for k in range(-3, 4)] + [h - (Q >> e) for e in (F.IN_BAND_E[0], F.FAST_E[-1])]
    vals = [v % Q for v in vals + [-v for v in vals]] + [0, 1, Q - 1]
    rng = random.Random(seed)
    out, nxt = [], 0
    for j in range(n):
        if F.boundary_lane(j, n):
            x = vals[nxt % len(vals)]
            nxt += 1
        else:
            x = rng.randrange(Q)
        out.append(F.centre(x, Q))
    return out


def to_ntt_lib(ctx, coeffs, moduli):
    """[..., n] centred integer polynomials -> [..., L, n] NTT-domain residues by the library's transform."""
    a = np.array([[[c % q for c in poly] for q in moduli] for poly in coeffs], dtype=np.uint64)
    for i in range(len(moduli)):
        a[:, i] = ctx.ntt_fwd(np.ascontiguousarray(a[:, i]), limb=i)
    return a


@pytest.fixture(scope="module")
def setup(gpu_available):
    prm = P.cfg3_params(N)
    assert prm.plain_modulus == 65537 and prm.gadget_base == 1 << 16
    q = prm.ct_basis.moduli
    ctx = HipContext.from_params(prm)
    assert ctx.path == PATH_EXACT_RNS and ctx.num_internal_aux == len(q) + 1
    rlk = F.uniform_key(prm)
    ctx.load_relin_key(rlk)
    rng = np.random.default_rng(77)
    cases = {}
    cases["uniform"] = (uniform_residues(rng, (B, 2), q, N), uniform_residues(rng, (B, 2), q, N))
    # (b) the lift's boundary in both operands
    polys = [lift_boundary_poly(q, N, 100 + k) for k in range(4 * B)]
    assert min(polys[0][:64]) < 0 < max(polys[0][:64]), "one wave must hold both signs"
    nt = to_ntt_lib(ctx, polys, q).reshape(2, B, 2, len(q), N)
    cases["lift"] = (np.ascontiguousarray(nt[0]), np.ascontiguousarray(nt[1]))
    # (c) the scale's boundary: T0 / T1, T1 / T2 on it, and uniform items between them
    u1, u2 = uniform_residues(rng, (B, 2), q, N), uniform_residues(rng, (B, 2), q, N)
    for k, (which, seed) in enumerate([("c0c1", 41), ("c1c2", 41), ("c0c1", 7), (None, 0), ("c1c2", 9)]):
        if which:
            a, b, coeffs = F.bfv_case(prm, which, seed)
            u1[k], u2[k] = a[0], b[0]
            band = F.in_band(q, prm.plain_modulus, coeffs[0][:64])
            assert any(band) and not all(band), "one wave must hold lanes of both kinds"
    cases["scale"] = (u1, u2)
    want = {k: (cref.bfv_mul_and_relin(prm, a, b, rlk, threads=8), cref.bfv_mul(prm, a, b, None, relin=False, threads=8))
            for k, (a, b) in cases.items()}
    return prm, ctx, cases, want


@pytest.mark.parametrize("batch,chunk", [(2, 0), (5, 2)])
@pytest.mark.parametrize("kind", ["uniform", "lift", "scale"])
def test_bfv_mul_folded(setup, kind, batch, chunk):
    prm, ctx, cases, want = setup
    ct1, ct2 = (np.ascontiguousarray(a[:batch]) for a in cases[kind])
    ctx.set_chunk(chunk if chunk else 512)
    dev = lambda a: torch.from_numpy(a.view(np.int64)).cuda()
    d1, d2 = dev(ct1), dev(ct2)
    out = torch.empty_like(d1)
    torch.cuda.synchronize()
    ctx.bfv_mul_and_relin_dev(d1, d2, out, batch)
    ctx.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want[kind][0][:batch])
    assert np.array_equal(ctx.bfv_mul_no_relin(ct1, ct2), want[kind][1][:batch])


def test_dbfv_mul_cfg4_keeps_psum_form(gpu_available):
    dp = P.cfg4_params(N)
    prm = dp.bfv_params
    q, d = prm.ct_basis.moduli, dp.num_digits
    assert d == 2
    rng = np.random.default_rng(78)
    a, b = uniform_residues(rng, (2, d, 2), q, N), uniform_residues(rng, (2, d, 2), q, N)
    a0, b0, rlk = F.dbfv_case(dp)
    a[0], b[0] = a0[0], b0[0]
    ctx = HipContext.from_params(prm)
    ctx.load_relin_key(rlk)
    out, _ = ctx.dbfv_mul(d, dp.base, dp.plain_modulus, a, b)
    assert np.array_equal(out, cref.dbfv_mul(dp, a, b, rlk, threads=8))

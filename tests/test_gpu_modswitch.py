"""Modulus switching on the GPU: exacto_bfv_mod_switch (csrc/ntt.hip ntt_dropprime_*_kernel).

Reference: tests/modswitch_ref.py (both modes in Python integers; the reference mode restates
bfv/modswitch.rs:37-87).  Every comparison is bit-exact.  Inputs are built from chosen coefficient values
with to_ntt, so each coefficient is an independent lane: remainders at the centring boundary and
quotients at both ends of [0, Q') sit at the edges of a thread's values, of a wave and of the row.
"""
import math
import random
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import bfv as obfv, params as P
from exacto_amd import _ffi
from exacto_amd._ffi import HipContext, ExactoError
from bridge import np_to_ct, np_to_rns, rns_to_np, uniform_residues
from worstcase import to_ntt
import modswitch_ref as M
import noise_ref

pytestmark = pytest.mark.gpu

KEY = [0x0123456789ABCDEF, 0x0FEDCBA987654321, 0x1111111122222222, 0x3333333344444444]
G2 = [1099509805057, 562949953443841]
SHAPES = {
    # name: (moduli, n, B, polys); B polys positions >= 28 boundary values
    "generic2_n16": (G2, 16, 3, 3),                       # one live thread; q above q_i
    "generic2_swapped_n16": (G2[::-1], 16, 3, 3),         # q below q_i
    "generic2_n1024": (G2, 1024, 2, 2),
    "generic2_swapped_n1024": (G2[::-1], 1024, 2, 2),
    "tiny_q0_n16": ([65537, 1099509805057], 16, 3, 3),    # q >> q_i: the re-reduction is a true remainder
    "cfg3_n1024": (P.Q3, 1024, 2, 2),                     # generic path, L = 3
    "cfg3_L2_n4096": (P.Q3[:2], 4096, 2, 2),              # hand-scheduled rounds
    "cfg3_n4096": (P.Q3, 4096, 2, 2),
    "cfg5_n8192": (P.Q4, 8192, 1, 3),
}


def _ctx(moduli, n, p=None):
    # the plain modulus does not enter the switch; 257 where 65537 is itself one of the primes
    return HipContext(n, moduli, plain_modulus=p or (257 if 65537 in moduli else 65537))


@pytest.mark.parametrize("which", list(SHAPES))
def test_boundary_placement_both_modes(gpu_available, which):
    moduli, n, B, polys = SHAPES[which]
    ct, xs = M.boundary_batch(moduli, n, B, polys, seed=len(which))
    q, Qp = moduli[-1], math.prod(moduli[:-1])
    # the inputs hold what they are meant to hold
    flat = [x for item in xs for poly in item for x in poly]
    assert {Qp * q - (q + 1) // 2, Qp * q - (q - 1) // 2, Qp * q - 1, 0, (q - 1) // 2, (q + 1) // 2} <= set(flat)
    ctx = _ctx(moduli, n)
    for mode in M.MODES:
        got = ctx.bfv_mod_switch(ct, mode=mode)
        want = M.drop_np(ct, moduli, n, mode)
        assert got.shape == (B, polys, len(moduli) - 1, n)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (which, mode, bad[:8].tolist(), len(bad))
    # the exact mode against the division form (an independent chain: CRT, one big-integer division, to_ntt)
    ys = [M.round_div(x, q, Qp) for x in xs[0][0]]
    assert M.drop_crt(xs[0][0], moduli, "round") == ys
    assert np.array_equal(ctx.bfv_mod_switch(ct[:1, :1])[0, 0], to_ntt(ys, moduli[:-1], n))


def test_levels_on_an_L3_context(gpu_available):
    n, moduli = 1024, P.Q3
    ctx = _ctx(moduli, n)
    rng = np.random.default_rng(21)
    for mode in M.MODES:
        # level 2 of an L = 3 context: prime 1 is dropped (with q_1^-1 mod q_0), not prime 2
        ct2, _ = M.boundary_batch(moduli[:2], n, 2, 2, seed=5)
        got = ctx.bfv_mod_switch(ct2, mode=mode)
        assert np.array_equal(got, M.drop_np(ct2, moduli[:2], n, mode))
        assert np.array_equal(got, _ctx(moduli[:2], n).bfv_mod_switch(ct2, mode=mode))
        # 3 -> 1 is two single calls
        ct3 = uniform_residues(rng, (3, 2), moduli, n)
        two = ctx.bfv_mod_switch(ct3, limbs_out=1, mode=mode)
        assert two.shape == (3, 2, 1, n)
        assert np.array_equal(two, ctx.bfv_mod_switch(ctx.bfv_mod_switch(ct3, mode=mode), mode=mode))
        assert np.array_equal(two, M.drop_np(ct3, moduli, n, mode, drops=2))


def test_four_levels_at_n8192(gpu_available):
    n, moduli = 8192, P.Q4
    ctx = _ctx(moduli, n, 1040407)
    ct, _ = M.boundary_batch(moduli, n, 1, 3, seed=8)
    for mode in M.MODES:
        got = ctx.bfv_mod_switch(ct, limbs_out=1, mode=mode)
        assert np.array_equal(got, M.drop_np(ct, moduli, n, mode, drops=3)), mode
        mid = ctx.bfv_mod_switch(ct, limbs_out=2, mode=mode)
        assert np.array_equal(ctx.bfv_mod_switch(mid, mode=mode), got)


@pytest.mark.parametrize("which", ["cfg3_n1024", "cfg3_n4096"])
def test_items_and_polys_are_isolated(gpu_available, which):
    import torch
    moduli, n = P.Q3, int(which.split("_n")[1])
    L, B, polys = 3, 3, 3
    ctx = _ctx(moduli, n)
    ct = uniform_residues(np.random.default_rng(33), (B, polys), moduli, n)
    want = {lo: {m: M.drop_np(ct, moduli, n, m, drops=L - lo) for m in M.MODES} for lo in (2, 1)}
    dev = torch.device("cuda:0")
    ct_d = torch.from_numpy(ct.view(np.int64)).to(dev)
    for chunk in (512, 1):
        ctx.set_chunk(chunk)
        for lo in (2, 1):
            for mode in M.MODES:
                out = torch.full((B, polys, lo, n), -1, dtype=torch.int64, device=dev)   # 0xFF: an unwritten row shows
                ctx.bfv_mod_switch_dev(ct_d, polys, L, lo, out, B, mode=mode)
                ctx.synchronize()
                got = out.cpu().numpy().view(np.uint64)
                assert np.array_equal(got, want[lo][mode]), (which, chunk, lo, mode)
                assert np.array_equal(ctx.bfv_mod_switch(ct, limbs_out=lo, mode=mode), got)
    # each (item, poly) alone gives its own rows
    ctx.set_chunk(512)
    one = ctx.bfv_mod_switch(ct[1:2, 2:3])
    assert np.array_equal(one[0, 0], want[2]["round"][1, 2])


@pytest.mark.parametrize("n", [1024, 4096])
@pytest.mark.parametrize("product", [False, True])
@pytest.mark.parametrize("key", ["ternary", "device"])
def test_end_to_end_on_the_device(gpu_available, n, product, key):
    """exacto_encrypt_sk -> (bfv_mul_and_relin) -> bfv_mod_switch -> exacto_bfv_decrypt / exacto_bfv_noise on a
    second context over moduli[:-1] with sk[:-1].  The noise bound is that of a ternary secret, so it is
    asserted with a ternary key (the oracle's).  The device's own gen_secret_key samples as the reference
    does (keygen.hip: a "-1" is q_0 - 1 in every limb, which is not a small value mod Q for L > 1): with it
    the plaintext and the exact noise are checked, not the bound."""
    prm = P.cfg3_params(n)
    moduli, p = prm.ct_basis.moduli, prm.plain_modulus
    q = moduli[-1]
    lower = M.lower_params(prm)
    ctx, lo = HipContext.from_params(prm), HipContext.from_params(lower)
    if key == "ternary":
        sk = rns_to_np(obfv.gen_secret_key(prm, random.Random(n + product)).poly)
    else:
        sk = ctx.gen_secret_key(KEY, stream=1)
    rng = np.random.default_rng(n)
    B = 2
    m1 = rng.integers(0, p, size=(B, n), dtype=np.uint64)
    ct = ctx.encrypt_sk(m1, sk, KEY, stream=2)
    want_pt = m1
    if product:
        ctx.gen_relin_key(sk, KEY, stream=3, resident=True)
        m2 = np.zeros((B, n), dtype=np.uint64)
        m2[:, 0] = [7, p - 1]
        ct = ctx.bfv_mul_and_relin(ct, ctx.encrypt_sk(m2, sk, KEY, stream=4))
        want_pt = m1 * m2[:, :1] % np.uint64(p)
    before = ctx.bfv_noise(ct, sk, expected=want_pt)
    out = ctx.bfv_mod_switch(ct)
    sk_lo = np.ascontiguousarray(sk[:-1])
    assert np.array_equal(lo.bfv_decrypt(out, sk_lo), want_pt), "the plaintext under moduli[:-1] and sk[:-1]"
    after = lo.bfv_noise(out, sk_lo, expected=want_pt)
    assert after == lo.bfv_noise(out, sk_lo), "the decrypted plaintext is the expected one"
    want = M.drop_np(ct, moduli, n, "round")
    assert np.array_equal(out, want)
    sk_or = SimpleNamespace(poly=np_to_rns(sk_lo, lower.ct_basis), params=lower)
    for i in range(B):
        bound = M.noise_bound(before[i], q, p, n)
        print(f"n={n} product={product} key={key} item {i}: noise {before[i]} -> {after[i]} (bound {bound})")
        if key == "ternary":
            assert after[i] <= bound
        assert after[i] == noise_ref.bfv_noise(np_to_ct(want[i], lower), sk_or, expected=[int(v) for v in want_pt[i]])
    # the reference mode's output is not a ciphertext of the smaller modulus
    ref = ctx.bfv_mod_switch(ct, mode="reference")
    assert not np.array_equal(lo.bfv_decrypt(ref, sk_lo), want_pt)


def test_dev_form_on_a_torch_stream(gpu_available):
    import torch
    n, moduli = 4096, P.Q3
    ctx = _ctx(moduli, n)
    ct = uniform_residues(np.random.default_rng(2), (2, 2), moduli, n)
    want = {m: ctx.bfv_mod_switch(ct, mode=m) for m in M.MODES}
    want1 = ctx.bfv_mod_switch(ct, limbs_out=1)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)
    try:
        with torch.cuda.stream(stream):
            ct_d = torch.from_numpy(ct.view(np.int64)).to(dev)
            outs = {m: torch.full((2, 2, 2, n), -1, dtype=torch.int64, device=dev) for m in M.MODES}
            out1 = torch.full((2, 2, 1, n), -1, dtype=torch.int64, device=dev)
            for m in M.MODES:
                ctx.bfv_mod_switch_dev(ct_d, 2, 3, 2, outs[m], 2, mode=m)
            ctx.bfv_mod_switch_dev(ct_d, 2, 3, 1, out1, 2)
        stream.synchronize()
        for m in M.MODES:
            assert np.array_equal(outs[m].cpu().numpy().view(np.uint64), want[m]), m
        assert np.array_equal(out1.cpu().numpy().view(np.uint64), want1)
    finally:
        ctx.set_stream(None)


def test_errors(gpu_available):
    import torch
    n, L = 64, 3
    ctx = _ctx(P.Q3, n)
    lib = ctx._lib
    buf = np.zeros((2, 3, L, n), dtype=np.uint64)
    out = np.zeros((2, 3, L, n), dtype=np.uint64)

    def host(polys, lin, lout, mode, B=1, ct=buf, o=out):
        _ffi.check(lib.exacto_bfv_mod_switch(ctx._h, ct.ctypes.data, polys, lin, lout, mode, o.ctypes.data, B))

    cases = [
        ((2, 1, 0, 0), "invalid parameter: cannot drop prime: only one modulus remaining"),
        ((2, 0, 0, 0), "invalid parameter: cannot drop prime: only one modulus remaining"),
        ((2, 1, 1, 0), "invalid parameter: cannot drop prime: only one modulus remaining"),
        ((2, 4, 3, 0), "invalid parameter: mod_switch: limbs_in = 4 exceeds the context's 3 ciphertext primes"),
        ((2, 3, 0, 0), "invalid parameter: mod_switch: limbs_out = 0 (at least one prime must remain)"),
        ((2, 3, 3, 0), "invalid parameter: mod_switch: limbs_out = 3 must be below limbs_in = 3"),
        ((2, 2, 3, 1), "invalid parameter: mod_switch: limbs_out = 3 must be below limbs_in = 2"),
        ((0, 3, 2, 0), "invalid parameter: mod_switch: ciphertext has no polynomials"),
        ((2, 3, 2, 2), "invalid parameter: mod_switch: unknown mode 2"),
        ((2, 3, 2, -1), "invalid parameter: mod_switch: unknown mode -1"),
    ]
    dev = torch.device("cuda:0")
    ct_d = torch.zeros((2 * 3 * L * n + 2,), dtype=torch.int64, device=dev)
    out_d = torch.zeros((2 * 3 * L * n + 2,), dtype=torch.int64, device=dev)

    def devcall(polys, lin, lout, mode, B=1, ct=None, o=None):
        _ffi.check(lib.exacto_bfv_mod_switch_dev(ctx._h, (ct_d if ct is None else ct).data_ptr(), polys, lin, lout, mode,
                                                 (out_d if o is None else o).data_ptr(), B))

    for args, text in cases:
        for call in (host, devcall):
            for B in (1, 0):     # the arguments are checked before the empty batch returns
                with pytest.raises(ExactoError) as e:
                    call(*args, B=B)
                assert e.value.variant == "InvalidParam" and str(e.value) == text, (args, call.__name__, B)
    # overlap (either way round) and misalignment
    for call, a, o in ((host, buf, buf), (devcall, ct_d, ct_d)):
        with pytest.raises(ExactoError) as e:
            call(2, 3, 2, 0, B=1, ct=a, o=o)
        assert e.value.variant == "InvalidParam" and str(e.value) == "invalid parameter: mod_switch: out overlaps ct"
    with pytest.raises(ExactoError) as e:
        devcall(1, 3, 2, 0, B=1, ct=ct_d, o=ct_d[2 * n:])     # out starts inside ct's last limb
    assert str(e.value) == "invalid parameter: mod_switch: out overlaps ct"
    with pytest.raises(ExactoError) as e:
        devcall(1, 2, 1, 0, B=1, ct=ct_d[n // 2:], o=ct_d)    # ct starts inside out
    assert str(e.value) == "invalid parameter: mod_switch: out overlaps ct"
    for a, o in ((ct_d[1:], out_d), (ct_d, out_d[1:])):
        with pytest.raises(ExactoError) as e:
            devcall(2, 3, 2, 0, B=1, ct=a, o=o)
        assert e.value.variant == "InvalidParam"
        assert str(e.value) == "invalid parameter: mod_switch: ct and out must be 16-byte aligned"
    # an empty batch with good arguments does nothing; the binding's own checks raise ValueError
    host(2, 3, 2, 0, B=0)
    devcall(2, 3, 2, 0, B=0)
    assert ctx.bfv_mod_switch(np.zeros((0, 2, L, n), dtype=np.uint64)).shape == (0, 2, L - 1, n)
    with pytest.raises(ValueError):
        ctx.bfv_mod_switch(np.zeros((1, 2, 1, n), dtype=np.uint64))
    # adjacent buffers do not overlap
    devcall(1, 3, 2, 0, B=1, ct=ct_d, o=ct_d[3 * n:])
    ctx.synchronize()

"""Hoisted rotations and linear transforms at every launch shape of their kernels: each case of
tests/hoist_shapes.py against tests/hoist_ref.py, np.array_equal over whole outputs, host and _dev forms,
output buffers pre-filled with -1.

Each case first asserts that its context takes the path, the digit count and the kernel shape it is listed
under (mac_block_shape / limbwise_kernel / launch_items restate the dispatch), so a change of the dispatch
that silently moves a case to another kernel fails here instead of leaving a shape uncovered.

  1. the rotations of every case;
  2. the linear transform of the cases marked for it (multi-item on both paths, R = 9, multi-lane);
  3. the multi-item cases again at set_chunk(1): the same bits one item per launch;
  4. the inputs of tests/variant_digest.py's hoist group: the library's digests are hoist_ref's.
"""
import numpy as np
import pytest

import hoist_ref
import hoist_shapes as HS
from exacto_amd._ffi import HipContext

pytestmark = pytest.mark.gpu


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


def _first_diff(got, want):
    """'' when equal, else the index of the first differing word (item, rotation, component, limb, position)."""
    if np.array_equal(got, want):
        return ""
    idx = np.unravel_index(int(np.argmax((got != want).ravel())), want.shape)
    return f"first difference at {tuple(int(i) for i in idx)} of {int((got != want).sum())} words"


def _context(name, chunk=None):
    """The case's context and key set, with the path and the kernel shape asserted."""
    c = HS.CASES[name]
    prm, elements, ct, gks, pts, want, want_lt = HS.case_data(name)
    n, L, R = prm.ring_degree, len(prm.ct_basis.moduli), len(elements)
    guse = HS.guse_of(name, prm)
    ctx = HipContext.from_params(prm)
    ctx.set_chunk(c.chunk if chunk is None else chunk)
    print(name, "ks32_primes", ctx.ks32_primes, "G", ctx.G, "guse", guse, "shape", c.shape)
    assert (ctx.ks32_primes > 0) == c.ks32
    assert ctx.G == prm.gadget_digits and gks.shape[1] == guse
    ks = ctx.galois_keyset(elements, gks)
    assert ks.R == R and ks.num_keys_used == guse and (ks.ks32_primes > 0) == c.ks32
    if c.ks32:
        assert HS.mac_block_shape(guse, L) == c.shape
    else:
        assert HS.limbwise_kernel(guse, L, n, False) == c.shape
    if c.launch and chunk is None:
        # the items of the first launch, as hoist_core computes them from this context's chunk and primes
        assert HS.launch_items(c.chunk, c.B, ctx.ks32_primes, False, L, n, R) == c.launch
    return ctx, ks


# ------------------------------------------------------------------ 1. rotations

@pytest.mark.parametrize("name", list(HS.CASES))
def test_rotations(gpu_available, name):
    c = HS.CASES[name]
    prm, elements, ct, gks, pts, want, _ = HS.case_data(name)
    n, R = prm.ring_degree, len(elements)
    ctx, ks = _context(name)
    got = ctx.bfv_rotate_hoisted(ct, ks)
    assert np.array_equal(got, want), "host form: " + _first_diff(got, want)
    # _dev forms: the set from device keys (released before use), the rotations into a -1 filled buffer
    gks_d, ct_d = _dev(gks), _dev(ct)
    out = _full((c.B, R, 2, ctx.L, n))
    _ready()
    ksd = ctx.galois_keyset_dev(elements, gks_d, gks.shape[1])
    del gks_d
    ctx.bfv_rotate_hoisted_dev(ct_d, ksd, out, c.B)
    ctx.synchronize()
    got = _host(out)
    assert np.array_equal(got, want), "_dev form: " + _first_diff(got, want)
    ks.close()
    ksd.close()


# ------------------------------------------------------------------ 2. linear transform

@pytest.mark.parametrize("name", [k for k, c in HS.CASES.items() if c.lt])
def test_linear_transform(gpu_available, name):
    c = HS.CASES[name]
    prm, elements, ct, gks, pts, _, want = HS.case_data(name)
    n, L = prm.ring_degree, len(prm.ct_basis.moduli)
    ctx, ks = _context(name)
    if c.ks32:
        print("items per launch", HS.launch_items(c.chunk, c.B, ctx.ks32_primes, True, L, n, len(elements)))
    else:
        assert HS.limbwise_kernel(ks.num_keys_used, L, n, True) == "plain"
    got = ctx.bfv_linear_transform(ct, ks, pts)
    assert np.array_equal(got, want), "host form: " + _first_diff(got, want)
    ct_d, pts_d, out = _dev(ct), _dev(pts), _full((c.B, 2, ctx.L, n))
    _ready()
    ctx.bfv_linear_transform_dev(ct_d, ks, pts_d, out, c.B)
    ctx.synchronize()
    got = _host(out)
    assert np.array_equal(got, want), "_dev form: " + _first_diff(got, want)
    ks.close()


# ------------------------------------------------------------------ 3. chunk invariance

@pytest.mark.parametrize("name", [k for k, c in HS.CASES.items() if c.chunk1])
def test_one_item_per_launch_gives_the_same_bits(gpu_available, name):
    c = HS.CASES[name]
    prm, elements, ct, gks, pts, want, want_lt = HS.case_data(name)
    ctx, ks = _context(name, chunk=1)
    assert HS.launch_items(1, c.B, ctx.ks32_primes, False, ctx.L, ctx.n, len(elements)) == 1
    got = ctx.bfv_rotate_hoisted(ct, ks)
    assert np.array_equal(got, want), _first_diff(got, want)
    if c.lt:
        got = ctx.bfv_linear_transform(ct, ks, pts)
        assert np.array_equal(got, want_lt), _first_diff(got, want_lt)
    ks.close()


# ------------------------------------------------------------------ 4. the digests of the variant runs

@pytest.mark.parametrize("n", [64, 4096])
def test_variant_digest_inputs_against_hoist_ref(gpu_available, n):
    """tests/test_gpu_variants.py compares each switch's digests of the hoist group with the default's; here
    the default's digests are those of hoist_ref on the same inputs."""
    import variant_digest as VD
    prm, elements, ct, gks, pts = VD.hoist_inputs(n)
    want = hoist_ref.rotate_hoisted(prm, ct, elements, gks, threads=4)
    want_lt = hoist_ref.linear_transform(prm, want, pts, threads=4)
    out = {}
    VD.hoist(out, sizes=(n,))
    assert out == {f"hoist_rotate_{n}": VD.sha(want), f"hoist_lt_{n}": VD.sha(want_lt)}

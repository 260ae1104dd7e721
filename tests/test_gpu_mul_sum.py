"""bfv_mul_sum: out[i][s] = sum over the terms (ia, ib, s) of bfv_mul_and_relin(a[i][ia], b[i][ib]) with
the sums taken before the key switch and the forward transform (exacto_bfv_mul_sum, context.hip
mul_group_run; the group sum of long sums is group_sum_kernel, dbfv_linear.hip).

Reference: bfv_mul_and_relin (src/bfv/eval.rs:73-82, keyswitch.rs:59-101) per product and bfv_add
(eval.rs:14-32) over the terms.  Residues are canonical, so the order of the additions does not matter
and everything here is bit-exact.  The yardstick is that composition through the library's own
bfv_mul_and_relin and bfv_add (both pinned to the oracle by test_gpu_bfv.py / test_gpu_ops.py); one
output per configuration is also compared against the C restatement of the reference summed mod q_l, and
at n = 16 the yardstick is the Python oracle itself.  Inputs are uniform residues and a uniform key, as in
test_gpu_psum.py.
"""

import numpy as np
import pytest

from oracle import bfv as obfv
from oracle import params as P, cref
from exacto_amd._ffi import HipContext, ExactoError, PATH_EXACT_RNS, PATH_HPS, PATH_SCHOOLBOOK
from bridge import ct_to_np, np_to_ct, np_to_rlk, uniform_residues

pytestmark = pytest.mark.gpu


def _inputs(prm, B, na, nb, seed):
    rng = np.random.default_rng(seed)
    q, n = prm.ct_basis.moduli, prm.ring_degree
    a = uniform_residues(rng, (B, na, 2), q, n)
    b = uniform_residues(rng, (B, nb, 2), q, n)
    rlk = uniform_residues(rng, (prm.gadget_digits, 2), q, n)
    return a, b, rlk


def _composition(ctx, a, b, terms, nslots):
    """The composition a caller has without bfv_mul_sum: one bfv_mul_and_relin over all products,
    bfv_add per term."""
    B = a.shape[0]
    lhs = np.concatenate([a[:, ia] for ia, _, _ in terms])
    rhs = np.concatenate([b[:, ib] for _, ib, _ in terms])
    prods = ctx.bfv_mul_and_relin(lhs, rhs).reshape((len(terms), B) + a.shape[2:])
    out = [None] * nslots
    for t, (_, _, s) in enumerate(terms):
        out[s] = prods[t] if out[s] is None else ctx.bfv_add(out[s], prods[t])
    return np.stack(out, axis=1)


def _cref_slot(prm, a, b, rlk, terms, item, s):
    """Slot s of one item from the C restatement of the reference: its products summed mod q_l."""
    Q = np.array(prm.ct_basis.moduli, dtype=object)[None, :, None]
    mine = [(ia, ib) for ia, ib, sl in terms if sl == s]
    lhs = np.stack([a[item, ia] for ia, _ in mine])
    rhs = np.stack([b[item, ib] for _, ib in mine])
    prods = cref.bfv_mul_and_relin(prm, lhs, rhs, rlk, threads=len(mine))   # one call: a thread per product
    acc = 0
    for p in prods:
        acc = (acc + p.astype(object)) % Q
    return acc


def _check_cref(prm, a, b, rlk, terms, got, item, s):
    if cref.available():
        assert np.array_equal(got[item, s].astype(object), _cref_slot(prm, a, b, rlk, terms, item, s))


# ---- 1. small n, all three multiplication paths: the yardstick is the Python oracle

def _small_params(which):
    if which == "exact":      # test_gpu_bfv.test_exact_cfg3_basis_small_n
        return P.cfg3_params(16), PATH_EXACT_RNS
    if which == "hps":        # test_gpu_bfv.test_hps_two_aux_small_n's basis at n = 16
        return (P.BfvParamsBuilder().ring_degree(16).plain_modulus(1040407).ct_moduli([1152921504606830593])
                .aux_moduli([18014398509998081, 36028797018972161]).gadget_base(256).build()), PATH_HPS
    return (P.BfvParamsBuilder().ring_degree(16).plain_modulus(17).ct_moduli([65537])   # test_schoolbook_path
            .gadget_base(4).build()), PATH_SCHOOLBOOK


@pytest.mark.parametrize("which", ["exact", "hps", "schoolbook"])
def test_small_n_all_paths_vs_oracle(gpu_available, which):
    prm, path = _small_params(which)
    B, terms = 2, [(0, 0, 0), (1, 1, 0), (2, 2, 0), (0, 2, 1)]
    a, b, rlk = _inputs(prm, B, 3, 3, 160 + len(which))
    ctx = HipContext.from_params(prm, device=0)
    assert ctx.path == path
    ctx.load_relin_key(rlk)
    got = ctx.bfv_mul_sum(a, b, terms, 2)
    key = np_to_rlk(rlk, prm)
    for i in range(B):
        want = [None, None]
        for ia, ib, s in terms:
            p = obfv.bfv_mul_and_relin(np_to_ct(a[i, ia], prm), np_to_ct(b[i, ib], prm), key)
            want[s] = p if want[s] is None else obfv.bfv_add(want[s], p)
        for s in range(2):
            assert np.array_equal(got[i, s], ct_to_np(want[s])), (which, i, s)
    assert np.array_equal(got, _composition(ctx, a, b, terms, 2))


# ---- 2. cfg3: the context's own limit, and long sums in groups of 2 and of 1

def test_cfg3_group_limits(gpu_available):
    prm = P.cfg3_params(4096)
    B, K = 2, 5
    terms = [(k, k, 0) for k in range(K)] + [(0, 4, 1)]
    a, b, rlk = _inputs(prm, B, K, K, 3030)
    ctx = HipContext.from_params(prm, device=0)
    ctx.load_relin_key(rlk)
    assert ctx.mul_sum_info()["last_mode"] == -1
    want = _composition(ctx, a, b, terms, 2)
    own = ctx.bfv_mul_sum(a, b, terms, 2)
    info_own = ctx.mul_sum_info()
    print("cfg3 own limit:", info_own)
    assert np.array_equal(own, want)
    _check_cref(prm, a, b, rlk, terms, own, B - 1, 0)
    ctx.set_mul_sum_group(2)   # output 0: groups of 2 + 2 + 1; output 1: a single product, no group sum
    got2 = ctx.bfv_mul_sum(a, b, terms, 2)
    info2 = ctx.mul_sum_info()
    print("cfg3 limit 2:", info2)
    assert np.array_equal(got2, want)
    # a long sum must stay on the summed key switch (not one key switch per product)
    assert info2["group_max"] == 2 and info2["last_mode"] in (1, 2)
    ctx.set_mul_sum_group(1)
    got1 = ctx.bfv_mul_sum(a, b, terms, 2)
    assert np.array_equal(got1, want)
    assert ctx.mul_sum_info()["group_max"] == 1
    ctx.set_mul_sum_group(0)
    assert ctx.mul_sum_info()["group_max"] == info_own["group_max"]
    # exacto_ctx_info's dbfv_key_switch is dbfv_mul's alone
    assert ctx.dbfv_key_switch == -1


# ---- 3. the dBFV index rule as a term list, and the two plan caches

def test_same_as_dbfv_mul_and_caches_do_not_leak(gpu_available):
    dp = P.cfg4_params(4096)
    prm = dp.bfv_params
    d, B = 2, 3
    terms = [(0, 0, 0), (0, 1, 1), (1, 0, 1)]
    a, b, rlk = _inputs(prm, B, d, d, 4040)
    ctx = HipContext.from_params(prm, device=0)
    ctx.load_relin_key(rlk)
    want = ctx.dbfv_mul(d, 256, 65536, a, b)[0]
    got = ctx.bfv_mul_sum(a, b, terms, d)
    assert np.array_equal(got, want)
    _check_cref(prm, a, b, rlk, terms, got, 1, 1)
    # dbfv_mul, bfv_mul_sum, dbfv_mul on one context: neither reuses the other's tables
    other = [(1, 1, 0), (0, 0, 1), (1, 0, 1)]
    first = ctx.dbfv_mul(d, 256, 65536, a, b)[0]
    mid = ctx.bfv_mul_sum(a, b, other, d)
    again = ctx.dbfv_mul(d, 256, 65536, a, b)[0]
    assert np.array_equal(first, want) and np.array_equal(again, first)
    assert np.array_equal(mid, _composition(ctx, a, b, other, d))
    assert np.array_equal(ctx.bfv_mul_sum(a, b, terms, d), want)


# ---- 4. matrix x vector: different operand counts

def test_matrix_vector(gpu_available):
    prm = P.cfg3_params(4096)
    B, R, C = 2, 2, 3
    terms = [(r * C + k, k, r) for r in range(R) for k in range(C)]
    a, b, rlk = _inputs(prm, B, R * C, C, 5050)
    ctx = HipContext.from_params(prm, device=0)
    ctx.load_relin_key(rlk)
    got = ctx.bfv_mul_sum(a, b, terms, R)
    assert np.array_equal(got, _composition(ctx, a, b, terms, R))
    _check_cref(prm, a, b, rlk, terms, got, 0, 1)


# ---- 5. a and b the same device buffer (sum of squares), through _dev

def test_same_device_buffer_sum_of_squares(gpu_available):
    import torch
    prm = P.cfg3_params(4096)
    B, K = 2, 3
    terms = [(k, k, 0) for k in range(K)]
    a, _, rlk = _inputs(prm, B, K, 1, 6060)
    ctx = HipContext.from_params(prm, device=0)
    ctx.load_relin_key(rlk)
    want = _composition(ctx, a, a, terms, 1)
    d_a = torch.from_numpy(a.view(np.int64)).cuda()
    L, n = prm.ct_basis.num_moduli(), prm.ring_degree
    d_out = torch.full((B + 1, 1, 2, L, n), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()   # the context's stream does not wait for torch's
    ctx.bfv_mul_sum_dev(d_a, K, d_a, K, terms, 1, d_out, B)
    ctx.bfv_mul_sum_dev(d_a, K, d_a, K, terms, 1, d_out, B)   # the same lists: the resident tables again
    ctx.synchronize()
    got = d_out.cpu().numpy()
    assert np.array_equal(got[:B].view(np.uint64), want)
    assert (got[B:] == -1).all()   # nothing written past the B outputs
    assert np.array_equal(d_a.cpu().numpy().view(np.uint64), a)   # inputs untouched
    _check_cref(prm, a, a, rlk, terms, got[:B].view(np.uint64), 1, 0)


# ---- 6. a batch across pipeline chunks and both lanes (test_psum_cfg4_matches_per_product's shape)

def test_batch_across_chunks(gpu_available):
    prm = P.cfg3_params(4096)
    B = 5
    terms = [(0, 0, 0), (0, 1, 1), (1, 0, 1)]
    a, b, rlk = _inputs(prm, B, 2, 2, 7070)
    ctx = HipContext.from_params(prm, device=0)
    ctx.set_chunk(4)
    ctx.load_relin_key(rlk)
    got = ctx.bfv_mul_sum(a, b, terms, 2)
    assert np.array_equal(got, _composition(ctx, a, b, terms, 2))
    _check_cref(prm, a, b, rlk, terms, got, B - 1, 1)


# ---- 7. n = 8192, int8 digits, a group limit of 2 on three products

def test_cfg5_int8_digits_grouped(gpu_available):
    prm = P.cfg5_params(8192).bfv_params
    terms = [(k, k, 0) for k in range(3)]
    a, b, rlk = _inputs(prm, 1, 3, 3, 8080)
    ctx = HipContext.from_params(prm, device=0)
    ctx.load_relin_key(rlk)
    want = _composition(ctx, a, b, terms, 1)
    ctx.set_mul_sum_group(2)
    got = ctx.bfv_mul_sum(a, b, terms, 1)
    info = ctx.mul_sum_info()
    print("cfg5 limit 2:", info)
    assert np.array_equal(got, want)
    assert info["group_max"] == 2 and info["last_mode"] in (1, 2)
    _check_cref(prm, a, b, rlk, terms, got, 0, 0)


# ---- 8. HPS at n = 4096 (the u64_dbfv BFV parameters)

def test_hps_4096(gpu_available):
    prm = P.u64_dbfv().bfv_params
    B = 2
    terms = [(k, k, 0) for k in range(3)]
    a, b, rlk = _inputs(prm, B, 3, 3, 9090)
    ctx = HipContext.from_params(prm, device=0)
    assert ctx.path == PATH_HPS
    ctx.load_relin_key(rlk)
    got = ctx.bfv_mul_sum(a, b, terms, 1)
    assert np.array_equal(got, _composition(ctx, a, b, terms, 1))
    _check_cref(prm, a, b, rlk, terms, got, 1, 0)


# ---- 9. errors

def test_errors(gpu_available):
    prm = P.cfg3_params(16)
    a, b, rlk = _inputs(prm, 1, 2, 3, 1)
    ctx = HipContext.from_params(prm, device=0)

    def err(terms, nslots, variant, text, x=a, y=b):
        with pytest.raises(ExactoError) as e:
            ctx.bfv_mul_sum(x, y, terms, nslots)
        assert e.value.variant == variant, str(e.value)
        assert text in str(e.value), str(e.value)

    # the parameter checks come before the key check
    err([], 1, "InvalidParam", "nterms = 0")
    err([(2, 0, 0)], 1, "InvalidParam", "left index 2 >= na = 2")
    err([(0, 3, 0)], 1, "InvalidParam", "right index 3 >= nb = 3")
    err([(0, 0, 0), (1, 1, 0)], 2, "InvalidParam", "output slot 1 has no term")
    # a slot >= nslots: the wrapper refuses it first (test_mul_sum_host.py); the library's own check
    ia = np.array([0], dtype=np.uint32)
    sl = np.array([4], dtype=np.uint32)
    out = np.zeros((1, 2, 2, 3, 16), dtype=np.uint64)
    rc = ctx._lib.exacto_bfv_mul_sum(ctx.handle, a.ctypes.data, 2, b.ctypes.data, 3, ia.ctypes.data, ia.ctypes.data,
                                     sl.ctypes.data, 1, 2, out.ctypes.data, 1)
    from exacto_amd._ffi import last_error
    assert rc == 1 and "slot 4 >= nslots = 2" in last_error()
    # no resident key: bfv_mul_and_relin's error
    with pytest.raises(ExactoError) as e0:
        ctx.bfv_mul_and_relin(a[:, 0], b[:, 0])
    err([(0, 0, 0)], 1, "MissingKey", str(e0.value))
    ctx.load_relin_key(rlk)
    # batch = 0 returns without touching out
    out[:] = 7
    rc = ctx._lib.exacto_bfv_mul_sum(ctx.handle, a.ctypes.data, 2, b.ctypes.data, 3, ia.ctypes.data, ia.ctypes.data,
                                     ia.ctypes.data, 1, 1, out.ctypes.data, 0)
    assert rc == 0 and (out == 7).all()
    # and the call works once the key is there
    got = ctx.bfv_mul_sum(a, b, [(0, 0, 0), (1, 2, 0)], 1)
    assert np.array_equal(got, _composition(ctx, a, b, [(0, 0, 0), (1, 2, 0)], 1))


def test_deferred_parameter_error(gpu_available):
    """A context whose parameters carry a deferred error returns it, as bfv_mul_and_relin does
    (test_gpu_bfv._guard_case: the schoolbook overflow guard, the single aux prime that is too small)."""
    q = 18014398509506561
    for aux, variant, text in (([], "NotImplemented", "schoolbook BFV multiplication can overflow i128"),
                               ([36028797018972161], "InvalidParam", "single aux prime too small")):
        ctx = HipContext(4096, [q], aux, 1040407, 256)
        rng = np.random.default_rng(101)
        ct = uniform_residues(rng, (1, 1, 2), [q], 4096)
        ctx.load_relin_key(uniform_residues(rng, (ctx.G, 2), [q], 4096))
        with pytest.raises(ExactoError) as e:
            ctx.bfv_mul_sum(ct, ct, [(0, 0, 0)], 1)
        assert e.value.variant == variant and text in str(e.value)

"""Squares on the one-operand pipeline: bfv_square_no_relin, bfv_square_and_relin, dbfv_square and the
square hook of eval_poly, bit for bit the two-operand call on the same buffer.

The yardstick is the library's own two-operand call, which tests/test_gpu_dispatch_matrix.py pins to
oracle/c for every case of tests/dispatch_cases.py; two cases additionally go straight against
cref.bfv_mul(prm, a, a) (sweep_exact_n16, p60_below_n4096: 0.9 s of CPU).  Every comparison is
np.array_equal over the whole output.

  1. every dispatch case (every launch_it instantiation, both HPS auxiliary counts), the schoolbook
     context, and sweep_exact_n2048 with EXACTO_KS32=0 (the limb-wise MAC);
  2. chunks and lanes at cfg3, the _dev form on a caller's stream at an offset inside a larger buffer;
  3. the work is halved: the profiling records' transform counts and the tensor kernel's name;
  4. dBFV: cfg4, u64_dbfv, cfg5 at n = 8192, a d = 3 set at n = 16, the plan cache key, depth guard, chunks;
  5. errors;
  6. eval_poly with square baby steps against the Python oracle.

The d = 3, p = 2^16, base 256 set has 256^3 = 0 mod 2^16, so its reps rows are zero and the limbs >= d
fold to nothing: it covers the odd d.  Reps coefficients other than 1 come from a second d = 3 set with
p = 65537 (256^3 = 65281 = (1, 255, 0) in base 256), which also turns the summed key switch off.
"""

import functools
import os
import zlib

import numpy as np
import pytest

import dispatch_cases as D
from dispatch_cases import BY_NAME, CASES
from exacto_amd._ffi import HipContext, ExactoError, PATH_SCHOOLBOOK
from oracle import bootstrap as ob, cref, params as P
from bridge import ct_to_np, np_to_ct, np_to_rlk, uniform_residues

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)
PK_FWD, PK_INV, PK_TENSOR = 0, 1, 2


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """The matrix test's recipe: uniform residues, item 0's c1 = q - 1 on every limb, a uniform key."""
    c = BY_NAME[name]
    prm = D.params_of(c)
    q = prm.ct_basis.moduli
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    a = uniform_residues(rng, (c.B, 2), q, c.n)
    a[0, 1] = np.array(q, dtype=np.uint64)[:, None] - 1
    rlk = uniform_residues(rng, (prm.gadget_digits, 2), q, c.n)
    return (prm,) + _frozen(a, rlk)


def _env_ctx(make, **env):
    """A context created with the environment switches `env` set around its creation only."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return make()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _check_square(ctx, a, rlk, tag):
    ctx.load_relin_key(rlk)
    got3, want3 = ctx.bfv_square_no_relin(a), ctx.bfv_mul_no_relin(a, a)
    assert np.array_equal(got3, want3), (tag, "bfv_square_no_relin")
    got2, want2 = ctx.bfv_square_and_relin(a), ctx.bfv_mul_and_relin(a, a)
    assert np.array_equal(got2, want2), (tag, "bfv_square_and_relin")
    return got3, got2


# ------------------------------------------------------------------ 1. every dispatch case

@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_every_dispatch_case(gpu_available, name):
    case = BY_NAME[name]
    prm, a, rlk = _inputs(name)
    ctx = HipContext(case.n, case.ct, case.aux, case.plain, case.gbase, device=0)
    assert ctx.path == case.expect.path
    got3, got2 = _check_square(ctx, a, rlk, name)
    if name in ("sweep_exact_n16", "p60_below_n4096"):
        assert cref.available(), "oracle/c/liboracle.so is not built: run build() of __graft_entry__.py"
        assert np.array_equal(got3, cref.bfv_mul(prm, a, a, None, relin=False, threads=THREADS)), name
        assert np.array_equal(got2, cref.bfv_mul(prm, a, a, rlk, relin=True, threads=THREADS)), name
    if name == "sweep_exact_n2048":      # the limb-wise 60-bit MAC
        ctx0 = _env_ctx(lambda: HipContext(case.n, case.ct, case.aux, case.plain, case.gbase, device=0),
                        EXACTO_KS32="0")
        assert ctx0.ks32_primes == 0
        _check_square(ctx0, a, rlk, name + " ks32=0")


def test_schoolbook(gpu_available):
    from test_gpu_mul_sum import _small_params
    prm, path = _small_params("schoolbook")
    assert path == PATH_SCHOOLBOOK
    q, n = prm.ct_basis.moduli, prm.ring_degree
    rng = np.random.default_rng(17)
    a = uniform_residues(rng, (2, 2), q, n)
    a[0, 1] = np.array(q, dtype=np.uint64)[:, None] - 1
    rlk = uniform_residues(rng, (prm.gadget_digits, 2), q, n)
    ctx = HipContext.from_params(prm, device=0)
    assert ctx.path == PATH_SCHOOLBOOK
    _check_square(ctx, a, rlk, "schoolbook")


# ------------------------------------------------------------------ 2. chunks and lanes at cfg3

@functools.lru_cache(maxsize=None)
def _cfg3(B):
    prm = P.cfg3_params(4096)
    q = prm.ct_basis.moduli
    rng = np.random.default_rng(3000 + B)
    a = uniform_residues(rng, (B, 2), q, 4096)
    a[0, 1] = np.array(q, dtype=np.uint64)[:, None] - 1
    rlk = uniform_residues(rng, (prm.gadget_digits, 2), q, 4096)
    return (prm,) + _frozen(a, rlk)


@pytest.mark.parametrize("B,chunk", [(5, 2), (130, 0), (1, 0)])
def test_cfg3_chunks_and_lanes(gpu_available, B, chunk):
    """B = 5, chunk 2: three chunks on two lanes, a short last one; B = 130: one chunk split into halves of
    65 on two lanes (P >= 128); B = 1."""
    prm, a, rlk = _cfg3(B)
    ctx = HipContext.from_params(prm, device=0)
    if chunk:
        ctx.set_chunk(chunk)
    _check_square(ctx, a, rlk, (B, chunk))


def test_cfg3_dev_form_on_a_stream_at_an_offset(gpu_available):
    import torch
    prm, a, rlk = _cfg3(5)
    B, L, n = 5, 3, 4096
    ctx = HipContext.from_params(prm, device=0)
    ctx.load_relin_key(rlk)
    want3, want2 = ctx.bfv_mul_no_relin(a, a), ctx.bfv_mul_and_relin(a, a)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)
    try:
        with torch.cuda.stream(stream):
            words, lead = B * 2 * L * n, 3 * n + 8          # the input starts 3 n + 8 words into the buffer
            big = torch.full((lead + words + n,), -1, dtype=torch.int64, device=dev)
            big[lead:lead + words] = torch.from_numpy(np.array(a).view(np.int64).reshape(-1)).to(dev)
            out3 = torch.full((B, 3, L, n), -1, dtype=torch.int64, device=dev)
            out2 = torch.full((B, 2, L, n), -1, dtype=torch.int64, device=dev)
            src = big.data_ptr() + 8 * lead
            ctx.bfv_square_no_relin_dev(src, out3, B)
            ctx.bfv_square_and_relin_dev(src, out2, B)
        stream.synchronize()
        assert np.array_equal(out3.cpu().numpy().view(np.uint64), want3)
        assert np.array_equal(out2.cpu().numpy().view(np.uint64), want2)
        host = big.cpu().numpy()
        assert (host[:lead] == -1).all() and (host[lead + words:] == -1).all()
        assert np.array_equal(host[lead:lead + words].view(np.uint64), a.reshape(-1))
    finally:
        ctx.set_stream(None)


# ------------------------------------------------------------------ 3. the work is halved

def _profiled(ctx, call):
    call()                               # key conversion and workspace growth stay outside the records
    ctx.prof_enable(True)
    try:
        call()
        polys = {k: ctx.prof_read(k)["polys"] for k in (PK_FWD, PK_INV, PK_TENSOR)}
        return polys, [nm for nm, _, _ in ctx.prof_kernels(PK_TENSOR)]
    finally:
        ctx.prof_enable(False)


def test_cfg3_work_is_halved(gpu_available):
    """run_mul's scopes per product: 4K -> 2K extended forward transforms and 4L -> 2L input inverses; the
    tensor's and the key switch's transforms are other kinds, the results' forward transforms are the same
    in both.  So the forward family is smaller by 2 K B and the inverse family by 2 L B."""
    prm, a, rlk = _cfg3(2)
    B, L = 2, 3
    ctx = HipContext.from_params(prm, device=0)
    K = ctx.num_internal_aux
    assert K == L + 1
    ctx.load_relin_key(rlk)
    mul, mul_t = _profiled(ctx, lambda: ctx.bfv_mul_and_relin(a, a))
    sq, sq_t = _profiled(ctx, lambda: ctx.bfv_square_and_relin(a))
    print("mul", mul, mul_t, "square", sq, sq_t)
    assert mul[PK_FWD] - sq[PK_FWD] == 2 * K * B, (mul, sq)
    assert mul[PK_INV] - sq[PK_INV] == 2 * L * B, (mul, sq)
    assert mul[PK_TENSOR] == sq[PK_TENSOR]
    # the square instantiation: the two-operand kernel's name with its last template argument (SQ) set
    assert len(mul_t) == 1 and len(sq_t) == 1 and mul_t[0].endswith(", false>"), (mul_t, sq_t)
    assert sq_t[0] == mul_t[0][:-len("false>")] + "true>", (mul_t, sq_t)


# ------------------------------------------------------------------ 4. dBFV

def _d3_params(plain):
    bfv = P.BfvParamsBuilder().ring_degree(16).plain_modulus(260111).ct_moduli(P.Q3).build()
    return P.DbfvParams(bfv, 256, 3, plain)


DBFV = {
    "cfg4": (lambda: P.cfg4_params(4096), 3),
    "u64_dbfv": (P.u64_dbfv, 2),
    "cfg5_n8192": (lambda: P.cfg5_params(8192), 1),
    "d3_p2_16_n16": (lambda: _d3_params(65536), 2),
    "d3_p65537_n16": (lambda: _d3_params(65537), 2),
}


def _dbfv_inputs(dp, B, seed):
    prm = dp.bfv_params
    q, n, d = prm.ct_basis.moduli, prm.ring_degree, dp.num_digits
    rng = np.random.default_rng(seed)
    a = uniform_residues(rng, (B, d, 2), q, n)
    a[0, 0, 1] = np.array(q, dtype=np.uint64)[:, None] - 1
    b = uniform_residues(rng, (B, d, 2), q, n)
    rlk = uniform_residues(rng, (prm.gadget_digits, 2), q, n)
    return a, b, rlk


@pytest.mark.parametrize("which", sorted(DBFV))
def test_dbfv_square(gpu_available, which):
    make, B = DBFV[which]
    dp = make()
    prm, d = dp.bfv_params, dp.num_digits
    a, _, rlk = _dbfv_inputs(dp, B, zlib.crc32(which.encode()))
    depth = np.zeros(B, dtype=np.uint32)
    ref = HipContext.from_params(prm, device=0)
    ref.load_relin_key(rlk)
    want, want_depth = ref.dbfv_mul(d, dp.base, dp.plain_modulus, a, a, depth, depth)
    ctx = HipContext.from_params(prm, device=0)
    ctx.load_relin_key(rlk)
    got, got_depth = ctx.dbfv_square(d, dp.base, dp.plain_modulus, a, depth)
    print(which, "dbfv_key_switch", ctx.dbfv_key_switch)
    assert np.array_equal(got, want), which
    assert np.array_equal(got_depth, want_depth) and (got_depth == 1).all()
    assert ctx.dbfv_key_switch == ref.dbfv_key_switch, which
    # ... and the other way round on one context
    got2, _ = ref.dbfv_square(d, dp.base, dp.plain_modulus, a)
    assert np.array_equal(got2, want), which
    assert ref.dbfv_key_switch == ctx.dbfv_key_switch


def test_dbfv_square_depth_guard(gpu_available):
    dp = _d3_params(65536)
    a, _, rlk = _dbfv_inputs(dp, 2, 5)
    ctx = HipContext.from_params(dp.bfv_params, device=0)
    ctx.load_relin_key(rlk)
    errs = []
    for call in (lambda: ctx.dbfv_square(3, dp.base, dp.plain_modulus, a, [0, 1]),
                 lambda: ctx.dbfv_mul(3, dp.base, dp.plain_modulus, a, a, [0, 1], [0, 1])):
        with pytest.raises(ExactoError) as e:
            call()
        errs.append((e.value.variant, str(e.value)))
    assert errs[0] == errs[1] and errs[0][0] == "NotImplemented"
    assert "chained dBFV multiplication requires ciphertext-level lattice reduction" in errs[0][1]
    # DbfvParams::new's checks
    for args in ((3, 1, 65536), (0, 256, 65536), (1, 256, 65536)):
        errs = []
        for call in (lambda: ctx.dbfv_square(*args, a), lambda: ctx.dbfv_mul(*args, a, a)):
            with pytest.raises(ExactoError) as e:
                call()
            errs.append((e.value.variant, str(e.value)))
        assert errs[0] == errs[1] and errs[0][0] == "InvalidParam", errs


def test_dbfv_plan_cache_key(gpu_available):
    """A product plan, the square plan and the product plan again of the same (B, d, base, p) on one
    context."""
    dp = P.cfg4_params(4096)
    a, b, rlk = _dbfv_inputs(dp, 2, 77)
    ref = HipContext.from_params(dp.bfv_params, device=0)
    ref.load_relin_key(rlk)
    want_ab = ref.dbfv_mul(2, dp.base, dp.plain_modulus, a, b)[0]
    want_aa = ref.dbfv_mul(2, dp.base, dp.plain_modulus, a, a)[0]
    ctx = HipContext.from_params(dp.bfv_params, device=0)
    ctx.load_relin_key(rlk)
    assert np.array_equal(ctx.dbfv_mul(2, dp.base, dp.plain_modulus, a, b)[0], want_ab)
    assert np.array_equal(ctx.dbfv_square(2, dp.base, dp.plain_modulus, a)[0], want_aa)
    assert np.array_equal(ctx.dbfv_mul(2, dp.base, dp.plain_modulus, a, b)[0], want_ab)
    assert np.array_equal(ctx.dbfv_square(2, dp.base, dp.plain_modulus, a)[0], want_aa)


def test_dbfv_square_two_chunks(gpu_available):
    """B = 5 at cfg4 with the chunk at one item's products (cfg4 needs (0, 0), (0, 1), (1, 0): the symmetric
    plan's two), so the summed scale's chunks hold one whole item each and the batch spans both lanes."""
    dp = P.cfg4_params(4096)
    a, _, rlk = _dbfv_inputs(dp, 5, 78)
    ref = HipContext.from_params(dp.bfv_params, device=0)
    ref.load_relin_key(rlk)
    want = ref.dbfv_mul(2, dp.base, dp.plain_modulus, a, a)[0]
    ctx = HipContext.from_params(dp.bfv_params, device=0)
    ctx.set_chunk(2)
    ctx.load_relin_key(rlk)
    assert ctx.psum_max >= 2
    assert np.array_equal(ctx.dbfv_square(2, dp.base, dp.plain_modulus, a)[0], want)
    assert ctx.dbfv_key_switch == ref.dbfv_key_switch


# ------------------------------------------------------------------ 5. errors

def _err(call):
    with pytest.raises(ExactoError) as e:
        call()
    return e.value.variant, str(e.value)


def test_errors(gpu_available):
    import torch
    prm = P.cfg3_params(16)
    q, n, L = prm.ct_basis.moduli, 16, 3
    rng = np.random.default_rng(9)
    a = uniform_residues(rng, (2, 2), q, n)
    a3 = uniform_residues(rng, (2, 3), q, n)
    ctx = HipContext.from_params(prm, device=0)
    # polys = 3
    assert _err(lambda: ctx.bfv_square_no_relin(a3)) == _err(lambda: ctx.bfv_mul_no_relin(a3, a3))
    assert _err(lambda: ctx.bfv_square_no_relin(a3))[0] == "InvalidParam"
    # no key
    assert _err(lambda: ctx.bfv_square_and_relin(a)) == _err(lambda: ctx.bfv_mul_and_relin(a, a))
    assert _err(lambda: ctx.bfv_square_and_relin(a))[0] == "MissingKey"
    assert np.array_equal(ctx.bfv_square_no_relin(a), ctx.bfv_mul_no_relin(a, a))   # needs no key
    # batch = 0
    empty = np.zeros((0, 2, L, n), dtype=np.uint64)
    assert ctx.bfv_square_no_relin(empty).shape == (0, 3, L, n)
    lib, h = ctx._lib, ctx._h
    assert lib.exacto_bfv_square_no_relin_dev(h, None, 2, None, 0) == 0
    ctx.load_relin_key(uniform_residues(rng, (prm.gadget_digits, 2), q, n))
    assert lib.exacto_bfv_square_and_relin_dev(h, None, None, 0) == 0
    assert lib.exacto_dbfv_square_dev(h, 2, 256, 65536, None, None, 0, None, None) == 0
    # out overlapping ct in the _dev form
    buf = torch.zeros((4, 3, L, n), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    w = 8 * L * n
    for call in (lambda: ctx.bfv_square_and_relin_dev(buf.data_ptr(), buf.data_ptr(), 2),
                 lambda: ctx.bfv_square_and_relin_dev(buf.data_ptr() + 2 * w, buf.data_ptr(), 2),
                 lambda: ctx.bfv_square_no_relin_dev(buf.data_ptr() + 5 * w, buf.data_ptr(), 2),
                 lambda: ctx.dbfv_square_dev(2, 256, 65536, buf.data_ptr() + 2 * w, buf.data_ptr(), 1)):
        variant, text = _err(call)
        assert variant == "InvalidParam" and "overlap" in text, (variant, text)
    ctx.synchronize()


def test_deferred_parameter_error(gpu_available):
    """The schoolbook overflow guard of test_gpu_bfv.py: the context's deferred error, as mul returns it."""
    q = 18014398509506561
    ctx = HipContext(4096, [q], [], 1040407, 256)
    rng = np.random.default_rng(101)
    ct = uniform_residues(rng, (1, 2), [q], 4096)
    ctx.load_relin_key(uniform_residues(rng, (ctx.G, 2), [q], 4096))
    for sq, mul in ((lambda: ctx.bfv_square_and_relin(ct), lambda: ctx.bfv_mul_and_relin(ct, ct)),
                    (lambda: ctx.bfv_square_no_relin(ct), lambda: ctx.bfv_mul_no_relin(ct, ct))):
        got = _err(sq)
        assert got == _err(mul)
        assert got[0] == "NotImplemented" and "schoolbook BFV multiplication can overflow i128" in got[1]


# ------------------------------------------------------------------ 6. eval_poly

@pytest.mark.parametrize("degree", [4, 9])
def test_eval_poly_square_steps(gpu_available, degree):
    """Degree 4: k = 3, a square at i = 2; degree 9: k = 4, squares at i = 2 and 4."""
    prm = P.cfg3_params(16)
    n, q = prm.ring_degree, prm.ct_basis.moduli
    rng = np.random.default_rng(60 + degree)
    coeffs = [int(v) for v in rng.integers(1, prm.plain_modulus, size=degree + 1)]
    ct = uniform_residues(rng, (2, 2), q, n)
    rlk = uniform_residues(rng, (prm.gadget_digits, 2), q, n)
    ctx = HipContext.from_params(prm, device=0)
    ctx.load_relin_key(rlk)
    got = ctx.eval_poly(ct, coeffs)
    off = HipContext.from_params(prm, device=0)
    off.set_square_hook(False)
    off.load_relin_key(rlk)
    assert np.array_equal(off.eval_poly(ct, coeffs), got)
    orlk = np_to_rlk(rlk, prm)
    for b in range(2):
        want = ob.eval_poly_homomorphic(np_to_ct(ct[b], prm), coeffs, orlk)
        assert np.array_equal(got[b], ct_to_np(want)), (degree, b)

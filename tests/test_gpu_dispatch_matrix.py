"""Every ring degree and prime class of the multiply path against oracle/c (cref), bit-exact, and the
kernels that ran against the selection tests/dispatch_cases.py writes next to each case.

  a. exact path at n = 16 .. 16384 (every launch_ntt / launch_inv_tensor instantiation, logn = 4 .. 14, with
     the suite's other sizes): bfv_mul_no_relin, relinearize of its output, bfv_mul_and_relin; at n = 2048
     and 16384 also with EXACTO_KS32=0, the limb-wise MAC's own oracle check there;
  b. HPS with one and two auxiliary primes at n = 128 .. 2048;
  c. class C primes (2^24 < 2^60 - q < 2^32) at n = 4096 / 8192, where they change kernels: the standalone
     transforms, the fused products, the multiply over all-C and mixed bases, the modulus switch, a dBFV
     product;
  d. the two nearest usable primes on either side of each threshold (2^60 - 2^32, 2^60 - 2^24, 2^60 on the
     exact path at n = 4096; the gen_qb boundaries 2^50 at n = 1024 and 2^56 at n = 4096 on the HPS path
     with one ciphertext prime and two auxiliary primes of the same side: a single auxiliary prime of q's
     size is refused, P <= n q / 2);
  e. primes >= 2^60 at n = 4096;
  f. for every case of c - e, one call under the library's profiling records: the kernel names of the
     forward-NTT, tensor, scale and key-switch families are the ones the table expects, so a later dispatch
     change cannot turn these cases into repeats of cfg3 unnoticed.

Every comparison is np.array_equal over the whole output.  The reference is oracle/c's exact O(n^2)
tensor; measured on 8 CPU threads (one product on all threads): L = 2 at n = 16384 4.0 s per call (28 s on
one thread), L = 3 at n = 8192 B = 2 2.9 s, L = 3 at n = 4096 B = 2 0.9 s, HPS cases 0.02 s; each
reference is computed once and shared.  Nothing here reads outside the repository tree.
"""

import functools
import math
import os
import zlib

import numpy as np
import pytest

import dispatch_cases as D
import modswitch_ref as M
from dispatch_cases import BY_NAME, CASES
from exacto_amd._ffi import HipContext, PATH_EXACT_RNS, PATH_HPS
from oracle import cref, params as P
from bridge import uniform_residues

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)
PK_FWD, PK_INV, PK_TENSOR, PK_POLYMUL, PK_SCALE, PK_KS_CRT, PK_RELIN_MAC, PK_HPS_SCALE, PK_MODSWITCH = 0, 1, 2, 3, 5, 8, 15, 16, 18
PIN = "exacto::ntt_fwd_pin_kernel<"


def _cref():
    assert cref.available(), "oracle/c/liboracle.so is not built: run build() of __graft_entry__.py"
    return cref


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """(params, ct1, ct2, rlk) of a case: uniform residues, item 0's c1 = q - 1 on every limb (a large third
    component)."""
    c = BY_NAME[name]
    prm = D.params_of(c)
    q = prm.ct_basis.moduli
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    ct1 = uniform_residues(rng, (c.B, 2), q, c.n)
    ct2 = uniform_residues(rng, (c.B, 2), q, c.n)
    ct1[0, 1] = np.array(q, dtype=np.uint64)[:, None] - 1
    rlk = uniform_residues(rng, (prm.gadget_digits, 2), q, c.n)
    return (prm,) + _frozen(ct1, ct2, rlk)


@functools.lru_cache(maxsize=None)
def _want(name, relin):
    prm, ct1, ct2, rlk = _inputs(name)
    return _frozen(_cref().bfv_mul(prm, ct1, ct2, rlk if relin else None, relin=relin, threads=THREADS))[0]


def _ctx(case, ks32=None):
    old = os.environ.get("EXACTO_KS32")
    if ks32 is not None:
        os.environ["EXACTO_KS32"] = "1" if ks32 else "0"
    try:
        ctx = HipContext(case.n, case.ct, case.aux, case.plain, case.gbase, device=0)
    finally:
        if ks32 is not None:
            if old is None:
                del os.environ["EXACTO_KS32"]
            else:
                os.environ["EXACTO_KS32"] = old
    return ctx


def _check_products(name, ctx, no_relin=True):
    """bfv_mul_no_relin, relinearize of its output and bfv_mul_and_relin of the case against cref."""
    _, ct1, ct2, rlk = _inputs(name)
    ctx.load_relin_key(rlk)
    if no_relin:
        got3 = ctx.bfv_mul_no_relin(ct1, ct2)
        assert np.array_equal(got3, _want(name, False)), (name, "bfv_mul_no_relin")
        assert np.array_equal(ctx.relinearize(got3), _want(name, True)), (name, "relinearize")
    assert np.array_equal(ctx.bfv_mul_and_relin(ct1, ct2), _want(name, True)), (name, "bfv_mul_and_relin")


def _profiled(ctx, call, kinds):
    """{kind: (launches, [kernel names])} of one `call` (made once before: key conversion and workspace
    growth stay outside the records)."""
    call()
    ctx.prof_enable(True)
    try:
        call()
        recs = {k: ctx.prof_read(k)["launches"] for k in kinds}
        return {k: (recs[k], [nm for nm, _, _ in ctx.prof_kernels(k)]) for k in kinds}
    finally:
        ctx.prof_enable(False)


def _check_kernels(case, ctx):
    """f: the kernels one bfv_mul_and_relin launched are the ones the table expects."""
    e, logn = case.expect, case.n.bit_length() - 1
    _, ct1, ct2, rlk = _inputs(case.name)
    ctx.load_relin_key(rlk)
    rec = _profiled(ctx, lambda: ctx.bfv_mul_and_relin(ct1, ct2),
                    (PK_FWD, PK_TENSOR, PK_SCALE, PK_HPS_SCALE, PK_KS_CRT, PK_RELIN_MAC))
    print(case.name, {k: v for k, v in rec.items() if v[0]})
    # forward NTTs.  Each scope holds one launch.  On the exact path the library's own auxiliary primes are
    # special primes, so their batch is pinned at these sizes whatever the ciphertext primes are.
    fwd = rec[PK_FWD][1]
    assert fwd, case.name
    other = [nm for nm in fwd if not nm.startswith(PIN)]
    if e.fwd_pinned:
        assert not other, (case.name, fwd)
        assert all(nm.startswith(f"{PIN}{logn},") for nm in fwd), fwd
    else:
        want = (f"exacto::ntt_fwd_gen_kernel<{logn}, {e.fwd_qb}>" if e.fwd_qb is not None
                else f"exacto::ntt_fwd_kernel<{logn}, false>")
        assert other and all(nm == want for nm in other), (case.name, fwd, want)
        if e.path == PATH_HPS:
            assert other == fwd, (case.name, fwd)
    # tensor: one scope, one launch per chunk
    n_t, tensor = rec[PK_TENSOR]
    assert n_t >= 1 and len(tensor) == 1, (case.name, tensor)
    is_asm = "tensor_pin_kernel" in tensor[0] or tensor[0].startswith(f"exacto::ntt_inv_tensor_kernel<{logn}, true, true,")
    assert is_asm == e.tensor_asm, (case.name, tensor)
    if not e.tensor_asm:
        want = (f"exacto::ntt_inv_tensor_kernel<{logn}, true, false, 0, true, {e.tensor_qb}," if e.tensor_qb is not None
                else f"exacto::ntt_inv_tensor_kernel<{logn}, false, false,")
        assert tensor[0].startswith(want), (case.name, tensor, want)
    # scale
    if e.path == PATH_HPS:
        assert rec[PK_SCALE][0] == 0 and rec[PK_HPS_SCALE][1] and \
            all(nm.startswith("exacto::hps_scale_kernel<") for nm in rec[PK_HPS_SCALE][1]), (case.name, rec)
    else:
        scale = rec[PK_SCALE][1]
        want = "exacto::exact_scale_sp_kernel<" if e.scale_sp else "exacto::exact_scale_kernel<"
        assert len(scale) == 1 and scale[0].startswith(want), (case.name, scale)
    # key switch
    assert (ctx.ks32_primes > 0) == e.ks32, (case.name, ctx.ks32_primes)
    if e.ks32:
        assert rec[PK_RELIN_MAC][0] == 0 and rec[PK_KS_CRT][1][0].startswith(f"exacto::ks32_crt_kernel<{logn},"), rec
    else:
        assert rec[PK_KS_CRT][0] == 0 and rec[PK_RELIN_MAC][0] >= 1, (case.name, rec)
    return rec


def _group(*groups):
    return [c.name for c in CASES if c.group in groups]


# ------------------------------------------------------------------ a. ring-degree sweep, exact path

@pytest.mark.parametrize("name", _group("sweep_exact"))
def test_sweep_exact(gpu_available, name):
    """n = 16384: two oracle calls of one product each, 4.0 s per call on 8 threads."""
    case = BY_NAME[name]
    ctx = _ctx(case)
    assert ctx.path == PATH_EXACT_RNS == case.expect.path
    assert (ctx.ks32_primes > 0) == case.expect.ks32, ctx.ks32_primes
    _check_products(name, ctx)
    if case.n in (2048, 16384):       # the limb-wise 60-bit MAC at the sizes only the 31-bit basis ran at
        ctx0 = _ctx(case, ks32=False)
        assert ctx0.ks32_primes == 0
        _check_products(name, ctx0)


# ------------------------------------------------------------------ b. ring-degree sweep, HPS

@pytest.mark.parametrize("name", _group("sweep_hps"))
def test_sweep_hps(gpu_available, name):
    case = BY_NAME[name]
    ctx = _ctx(case)
    assert ctx.path == PATH_HPS == case.expect.path and ctx.ks32_primes == 0
    _check_products(name, ctx)


# ------------------------------------------------------------------ c. class C at n = 4096 / 8192

def _ntt_rows(rng, n, q):
    top = np.full(n, q - 1, dtype=np.uint64)
    alt = np.where(np.arange(n) % 2 == 0, q - 1, 0).astype(np.uint64)
    return np.concatenate([rng.integers(0, q, size=(3, n), dtype=np.uint64), np.stack([top, alt, top[::-1].copy()])])


@pytest.mark.parametrize("n", [4096, 8192])
@pytest.mark.parametrize("q", D.CLASS_C4)
def test_classC_standalone_ntt(gpu_available, n, q):
    """ntt_fwd / ntt_inv over one class C prime (the pinned kernels at d up to 2^32 - 2^20) against
    cref.ntt: random rows, all q - 1, alternating 0 / q - 1, and the inverse of all-(q - 1) evaluations."""
    _cref()
    logn = n.bit_length() - 1
    ctx = HipContext(n, [q], plain_modulus=257)
    a = _ntt_rows(np.random.default_rng(q % 1000 + n), n, q)
    want_f, want_i = cref.ntt(n, q, a), cref.ntt(n, q, a, inverse=True)
    assert np.array_equal(ctx.ntt_fwd(a), want_f)
    assert np.array_equal(ctx.ntt_inv(a), want_i)      # rows 3 .. 5: extreme evaluations, all q - 1 among them
    assert np.array_equal(ctx.ntt_inv(want_f), a)
    rec = _profiled(ctx, lambda: (ctx.ntt_fwd(a), ctx.ntt_inv(a)), (PK_FWD, PK_INV))
    assert rec[PK_FWD] == (1, [f"{PIN}{logn}, 0, false>"]), rec
    assert rec[PK_INV] == (1, [f"exacto::ntt_inv_pin_kernel<{logn}>"]), rec


@pytest.mark.parametrize("n", [4096, 8192])
def test_classC_fused_products(gpu_available, n):
    """exacto_rns_mul_inv_dev and exacto_rns_polymul_dev over the four class C primes against cref.polymul,
    in place and out of place.  Items: random and extreme NTT-domain operands, extreme coefficient-domain
    operands.  Class C takes the composition (pinned forward NTTs, C++ product + inverse), never the fused
    special-prime kernel."""
    import torch
    _cref()
    qs, L, B = D.CLASS_C4, 4, 4
    rng = np.random.default_rng(n)
    qcol = np.array(qs, dtype=np.uint64)[None, :, None]
    a = uniform_residues(rng, (B,), qs, n)             # NTT domain
    b = uniform_residues(rng, (B,), qs, n)
    a[1] = qcol[0] - 1
    b[1, :, ::2] = qcol[0, :, 0:1] - 1
    inv = lambda x: np.stack([cref.ntt(n, q, x[:, i], inverse=True) for i, q in enumerate(qs)], axis=1)
    fwd = lambda x: np.stack([cref.ntt(n, q, x[:, i]) for i, q in enumerate(qs)], axis=1)
    A, Bc = inv(a), inv(b)                             # coefficient domain
    A[2] = qcol[0] - 1
    Bc[2] = 0
    Bc[2, :, 1::2] = qcol[0, :, 0:1] - 1
    a, b = fwd(A), fwd(Bc)
    want = np.stack([cref.polymul(n, q, A[:, i], Bc[:, i]) for i, q in enumerate(qs)], axis=1)
    ctx = HipContext(n, qs, plain_modulus=257)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()
    host = lambda t: t.cpu().numpy().view(np.uint64)
    da, db, dA, dB = dev(a), dev(b), dev(A), dev(Bc)
    out = torch.empty_like(da)
    torch.cuda.synchronize()
    ctx.rns_mul_inv_dev(da, db, out, B)
    ctx.synchronize()
    assert np.array_equal(host(out), want), "rns_mul_inv_dev out of place"
    ctx.rns_mul_inv_dev(da, db, da, B)
    ctx.synchronize()
    assert np.array_equal(host(da), want), "rns_mul_inv_dev in place"
    out.zero_()
    torch.cuda.synchronize()

    def polymul():
        ctx.rns_polymul_dev(dA, dB, out, B)
        ctx.synchronize()
    rec = _profiled(ctx, polymul, (PK_POLYMUL, PK_FWD))
    assert np.array_equal(host(out), want), "rns_polymul_dev out of place"
    ctx.rns_polymul_dev(dA, dB, dB, B)
    ctx.synchronize()
    assert np.array_equal(host(dB), want), "rns_polymul_dev in place"
    logn = n.bit_length() - 1
    assert rec[PK_POLYMUL][0] == 0, rec                # not the fused special-prime kernel
    assert rec[PK_FWD][0] == 2 and rec[PK_FWD][1] == [f"{PIN}{logn}, 0, false>"], rec


@pytest.mark.parametrize("name", _group("classC"))
def test_classC_multiply(gpu_available, name):
    """All-C and mixed bases: n = 8192, L = 3, B = 2 is two oracle calls of 2.9 s on 8 threads."""
    case = BY_NAME[name]
    ctx = _ctx(case)
    assert ctx.path == PATH_EXACT_RNS and ctx.ks32_primes == 0
    _check_products(name, ctx)
    _check_kernels(case, ctx)


@pytest.mark.parametrize("n", [4096, 8192])
@pytest.mark.parametrize("basis", sorted(D.MODSWITCH_BASES))
def test_classC_mod_switch(gpu_available, basis, n):
    """bfv_mod_switch in both modes against modswitch_ref.drop_np on boundary inputs; the drop runs the
    hand-scheduled kernel (every prime involved lies in the 2^32 window)."""
    _cref()
    moduli = D.MODSWITCH_BASES[basis]
    B, polys = 2, 2
    ct, xs = M.boundary_batch(moduli, n, B, polys, seed=n + len(moduli))
    q, Qp = moduli[-1], math.prod(moduli[:-1])
    flat = {x for item in xs for poly in item for x in poly}
    assert {Qp * q - (q + 1) // 2, Qp * q - (q - 1) // 2, Qp * q - 1, 0, (q - 1) // 2, (q + 1) // 2} <= flat
    ctx = HipContext(n, moduli, plain_modulus=65537)
    for mode in M.MODES:
        got = ctx.bfv_mod_switch(ct, mode=mode)
        assert np.array_equal(got, M.drop_np(ct, moduli, n, mode)), (basis, n, mode)
        if len(moduli) == 3:
            assert np.array_equal(ctx.bfv_mod_switch(ct, limbs_out=1, mode=mode),
                                  M.drop_np(ct, moduli, n, mode, drops=2)), (basis, n, mode, "two drops")
    rec = _profiled(ctx, lambda: ctx.bfv_mod_switch(ct), (PK_MODSWITCH,))
    logn = n.bit_length() - 1
    assert rec[PK_MODSWITCH][0] >= 1 and rec[PK_MODSWITCH][1] == [f"exacto::ntt_dropprime_asm_kernel<{logn}, true>"], rec


def test_classC_dbfv_mul(gpu_available):
    """cfg4's digits (d = 2, base 256, t = 260111) over the mixed basis, B = 2, against cref.dbfv_mul
    (8 products: 2.3 s on 8 threads).  No 31-bit key switch and no summed tensors here: per-product scale,
    limb-wise MAC."""
    _cref()
    m = D.DBFV_MIXED
    prm = P.BfvParamsBuilder().ring_degree(m["n"]).plain_modulus(m["plain"]).ct_moduli(m["ct"]).gadget_base(m["gbase"]).build()
    dp = P.DbfvParams(prm, m["base"], m["d"], m["dplain"])
    q, n = m["ct"], m["n"]
    rng = np.random.default_rng(260111)
    a = uniform_residues(rng, (m["B"], m["d"], 2), q, n)
    b = uniform_residues(rng, (m["B"], m["d"], 2), q, n)
    a[0, 0, 1] = np.array(q, dtype=np.uint64)[:, None] - 1
    rlk = uniform_residues(rng, (prm.gadget_digits, 2), q, n)
    ctx = HipContext.from_params(prm)
    assert ctx.path == PATH_EXACT_RNS and ctx.ks32_primes == 0
    ctx.load_relin_key(rlk)
    got, _ = ctx.dbfv_mul(m["d"], m["base"], m["dplain"], a, b)
    assert ctx.dbfv_key_switch == 0, ctx.dbfv_key_switch      # per product: nothing to sum the digits in
    assert np.array_equal(got, cref.dbfv_mul(dp, a, b, rlk, threads=THREADS))


# ------------------------------------------------------------------ d. threshold neighbours, e. primes >= 2^60

@pytest.mark.parametrize("name", _group("edge", "big"))
def test_threshold_neighbours(gpu_available, name):
    """bfv_mul_and_relin (and bfv_mul_no_relin, relinearize) with the two nearest primes on one side of a
    threshold, and the kernels that ran.  HPS cases: q and two auxiliary primes of the same side."""
    case = BY_NAME[name]
    ctx = _ctx(case)
    assert ctx.path == case.expect.path
    _check_products(name, ctx)
    _check_kernels(case, ctx)

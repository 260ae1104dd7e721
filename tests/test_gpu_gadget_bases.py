"""Every gadget-digit path of the device across gadget bases: odd bases, bases that are no power of two,
bases above 2^16 and above a ciphertext prime, and the standalone decomposition of the C ABI.

Reference: gadget_decompose (src/bfv/keyswitch.rs:11-52, `base: u64` taken literally), relinearize
(keyswitch.rs:59-101), bfv_mul_and_relin (eval.rs:73-82), bfv_apply_automorphism (eval.rs:512-561),
dbfv_mul (dbfv/eval.rs:82-149), through the Python restatement (oracle/) at small sizes and its C
restatement (oracle/c) at n >= 1024.  Integer work: everything is bit-exact.

The device code this reaches (exacto_amd/csrc/kernels.hip):
  * gadget_digits with gshift == -1: a multiword / B and % B per digit (every base that is no power of
    two);
  * u64 digit residues for bases above 2^16, reduced mod q_i where the base exceeds a ciphertext prime
    (digit_small == 0), with the limb-wise MAC and no key switch over 31-bit primes;
  * the generic int16 digits feeding the 31-bit key switch (bases 2^s with s not dividing 32, and every
    other base <= 2^16, at n >= 1024);
  * HPS with a base that is not 2^1 .. 2^16 (gadget_digits<false, 1, DT> in hps_scale_kernel), int8
    digits of base 255 summed per output limb;
  * exacto_gadget_decompose_dev itself.
Each test asserts which path ran (ks32_primes, ks32_lazy, bfv_mul_sum's last_mode, dbfv_key_switch)
before it compares.

The last two tests run the two limits that the digit bound ceil(B/2) decides (DESIGN.md §4,
tests/test_gadget_bounds.py): int16 sums of three digits of base 21845, and the 31-bit basis at the
most products it sums for base 711.
"""

import math
import os

import numpy as np
import pytest

from oracle import bfv as obfv, dbfv as odbfv, params as P, cref
from oracle.bfv import gadget_decompose_coeff
from exacto_amd._ffi import HipContext, ExactoError, PATH_EXACT_RNS, PATH_HPS, PATH_SCHOOLBOOK
from bridge import ct_to_np, np_to_ct, np_to_rlk, uniform_residues
import worstcase as W

pytestmark = pytest.mark.gpu

Q40 = [1099509805057]
Q2 = [65537, 1099509805057]
HPS_Q, HPS_AUX = [1152921504606830593], [18014398509998081, 36028797018972161]


def params(n, moduli, plain, base, aux=()):
    b = P.BfvParamsBuilder().ring_degree(n).plain_modulus(plain).ct_moduli(moduli).gadget_base(base)
    return (b.aux_moduli(list(aux)) if aux else b).build()


SMALL = {   # name: (n, ciphertext primes, plain modulus, auxiliary primes, multiplication path)
    "schoolbook": (16, Q40, 17, (), PATH_SCHOOLBOOK),
    "q2": (16, Q2, 257, (), PATH_EXACT_RNS),
    "cfg3": (64, P.Q3, 65537, (), PATH_EXACT_RNS),
    "hps": (64, HPS_Q, 1040407, HPS_AUX, PATH_HPS),
}


def small_params(which, base):
    n, q, plain, aux, _ = SMALL[which]
    return params(n, q, plain, base, aux)


# ------------------------------------------------------------------ a. the standalone decomposition

DECOMPOSE_BASES = [2, 3, 8, 10, 255, 1000, 21845, 65535, 65536, 65537, 1 << 20, 10 ** 6 + 3, 1 << 32,
                   (1 << 32) + 15, 1 << 40, 1 << 63, (1 << 64) - 1]


def decompose_rows(rng, moduli, n, base, G):
    """[3][n] values mod Q as Python ints: uniform, with the crafted values of worstcase.crafted_values
    dealt over the three rows (each row keeps uniform entries)."""
    Q = math.prod(moduli)
    crafted = W.crafted_values(Q, base, G)
    assert len(crafted) <= 2 * n
    rows = [[int.from_bytes(rng.bytes(32), "little") % Q for _ in range(n)] for _ in range(3)]
    for k, v in enumerate(crafted):      # spread over the rows: every row has crafted and uniform entries
        rows[k % 3][k // 3] = v
    return rows


@pytest.mark.parametrize("which", ["schoolbook", "q2", "cfg3"])
@pytest.mark.parametrize("base", DECOMPOSE_BASES)
def test_gadget_decompose_dev(gpu_available, which, base):
    import torch
    n, q, plain, _, _ = SMALL[which]
    G = P.compute_gadget_digits(q, base)
    if G > 64:
        with pytest.raises(ExactoError) as e:
            HipContext(n, q, (), plain, base)
        assert e.value.variant == "InvalidParam" and "gadget digit count exceeds 64" in str(e.value)
        return
    ctx = HipContext(n, q, (), plain, base)
    assert ctx.G == G and ctx.gadget_base == base
    Q, L = math.prod(q), len(q)
    rows = decompose_rows(np.random.default_rng(base % 1000 + n), q, n, base, G)
    coeffs = np.array([[[v % qi for v in row] for qi in q] for row in rows], dtype=np.uint64)   # [3][L][n]
    want = np.empty((3, G, L, n), dtype=np.uint64)
    for b, row in enumerate(rows):
        for j, v in enumerate(row):
            for g, d in enumerate(gadget_decompose_coeff(v, Q, base, G)):
                for i, qi in enumerate(q):
                    want[b, g, i, j] = d % qi
    d_in = torch.from_numpy(coeffs.view(np.int64)).cuda()
    SENT = -0x0123456789ABCDEF
    for num_digits in sorted({1, max(G - 1, 1), G, G + 3}):
        guse = min(G, num_digits)
        # room for num_digits digits per item: what lies past [3][guse][L][n] must stay untouched
        d_out = torch.full((3 * (G + 3) * L * n,), SENT, dtype=torch.int64, device="cuda")
        ctx.gadget_decompose_dev(d_in, d_out, 3, num_digits)
        ctx.synchronize()
        out = d_out.cpu().numpy().view(np.uint64)
        used = 3 * guse * L * n
        got = out[:used].reshape(3, guse, L, n)
        assert np.array_equal(got, want[:, :guse]), (which, base, num_digits)
        assert (out[used:].view(np.int64) == SENT).all(), (which, base, num_digits)


# ------------------------------------------------------------------ b. every consumer, small sizes

def oracle_dbfv_mul(dp, a, b, rlk):
    prm = dp.bfv_params
    key = np_to_rlk(rlk, prm)
    out = []
    for i in range(a.shape[0]):
        x = odbfv.DbfvCiphertext([np_to_ct(l, prm) for l in a[i]], dp.num_digits, 0, dp)
        y = odbfv.DbfvCiphertext([np_to_ct(l, prm) for l in b[i]], dp.num_digits, 0, dp)
        out.append(np.stack([ct_to_np(l) for l in odbfv.dbfv_mul(x, y, key).limbs]))
    return np.stack(out)


def consumers_vs_oracle(prm, path, nkeys, seed):
    """bfv_mul_and_relin, relinearize, bfv_apply_automorphism, dbfv_mul (d = 2) and bfv_mul_sum (two
    terms in one slot) of one context against the Python oracle, with a key of nkeys rows."""
    n, q = prm.ring_degree, prm.ct_basis.moduli
    rng = np.random.default_rng(seed)
    ctx = HipContext.from_params(prm)
    assert ctx.path == path and ctx.G == prm.gadget_digits and ctx.ks32_primes == 0
    B = 3
    ct1, ct2 = uniform_residues(rng, (B, 2), q, n), uniform_residues(rng, (B, 2), q, n)
    ct1[0, 1] = np.array(q, dtype=np.uint64)[:, None] - 1          # extreme c1 -> a large third component
    rlk = uniform_residues(rng, (nkeys, 2), q, n)
    key = np_to_rlk(rlk, prm)
    ctx.load_relin_key(rlk)
    got = ctx.bfv_mul_and_relin(ct1, ct2)
    prods = [obfv.bfv_mul_and_relin(np_to_ct(ct1[i], prm), np_to_ct(ct2[i], prm), key) for i in range(B)]
    for i in range(B):
        assert np.array_equal(got[i], ct_to_np(prods[i])), ("mul_and_relin", i)
    ct3 = uniform_residues(rng, (B, 3), q, n)
    got = ctx.relinearize(ct3)
    for i in range(B):
        assert np.array_equal(got[i], ct_to_np(obfv.relinearize(np_to_ct(ct3[i], prm), key))), ("relinearize", i)
    for element in (3, 2 * n - 1):
        gk = uniform_residues(rng, (nkeys, 2), q, n)
        got = ctx.bfv_apply_automorphism(ct1, element, gk)
        keyset = obfv.GaloisKey(np_to_rlk(gk, prm).keys, element, prm)
        for i in (0, B - 1):
            want = ct_to_np(obfv.bfv_apply_automorphism(np_to_ct(ct1[i], prm), keyset))
            assert np.array_equal(got[i], want), ("automorphism", element, i)
    dp = P.DbfvParams(prm, 16, 2, 256)
    a, b = uniform_residues(rng, (2, 2, 2), q, n), uniform_residues(rng, (2, 2, 2), q, n)
    out, _ = ctx.dbfv_mul(2, dp.base, dp.plain_modulus, a, b)
    assert ctx.dbfv_key_switch == 0                                  # one key switch per product
    assert np.array_equal(out, oracle_dbfv_mul(dp, a, b, rlk)), "dbfv_mul"
    got = ctx.bfv_mul_sum(ct1[:, None], ct2[:, None], [(0, 0, 0), (0, 0, 0)], 1)
    assert ctx.mul_sum_info()["last_mode"] == 0
    for i in range(B):
        assert np.array_equal(got[i, 0], ct_to_np(obfv.bfv_add(prods[i], prods[i]))), ("mul_sum", i)


SMALL_CASES = (
    [("q2", b, None) for b in (3, 1000, 65535, 65537, 1 << 20, (1 << 32) + 15)] + [("q2", 1000, 2)] +
    # cfg3's Q ~ 2^180: bases 3 and 5 need G = 114 and 78 > 64; 9 (G = 57) is the smallest odd square
    [("cfg3", b, None) for b in (9, 1000, 65535, 65537, 1 << 20, (1 << 32) + 15)] + [("cfg3", 65537, 5)] +
    [("schoolbook", b, None) for b in (3, 1000)] +
    [("hps", b, None) for b in (255, 1000, 65535, 1 << 20)]
)


@pytest.mark.parametrize("which,base,nkeys", SMALL_CASES)
def test_every_digit_consumer_small(gpu_available, which, base, nkeys):
    prm = small_params(which, base)
    assert prm.gadget_digits <= 64
    consumers_vs_oracle(prm, SMALL[which][4], nkeys or prm.gadget_digits, base % 997 + (nkeys or 0))


# ------------------------------------------------------------------ c. production kernels, n = 1024

def ks32_ctx(prm, on: bool):
    old = os.environ.get("EXACTO_KS32")
    os.environ["EXACTO_KS32"] = "1" if on else "0"
    try:
        return HipContext.from_params(prm, device=0)
    finally:
        if old is None:
            del os.environ["EXACTO_KS32"]
        else:
            os.environ["EXACTO_KS32"] = old


@pytest.mark.parametrize("base,ks32", [(32, True), (1000, True), (21845, True), (65535, True),
                                       (65537, False), (1 << 20, False)])
def test_production_kernels_n1024(gpu_available, base, ks32):
    n, B = 1024, 3
    prm = params(n, P.Q3, 65537, base)
    q = prm.ct_basis.moduli
    rng = np.random.default_rng(base % 1009)
    ctx = HipContext.from_params(prm)
    assert (ctx.ks32_primes > 0) == ks32 and ctx.G == prm.gadget_digits
    ct1, ct2 = uniform_residues(rng, (B, 2), q, n), uniform_residues(rng, (B, 2), q, n)
    ct1[0, 1] = np.array(q, dtype=np.uint64)[:, None] - 1
    rlk = uniform_residues(rng, (prm.gadget_digits, 2), q, n)
    ctx.load_relin_key(rlk)
    got = ctx.bfv_mul_and_relin(ct1, ct2)
    assert np.array_equal(got, cref.bfv_mul_and_relin(prm, ct1, ct2, rlk, threads=B))
    dp = P.DbfvParams(prm, 16, 2, 256)
    a, b = uniform_residues(rng, (B, 2, 2), q, n), uniform_residues(rng, (B, 2, 2), q, n)
    out, _ = ctx.dbfv_mul(2, dp.base, dp.plain_modulus, a, b)
    # 31-bit basis: limb 1's two products are key-switched as one sum (1: primary, 2: wide basis)
    assert (ctx.dbfv_key_switch in (1, 2)) if ks32 else ctx.dbfv_key_switch == 0
    assert np.array_equal(out, cref.dbfv_mul(dp, a, b, rlk, threads=B))
    # relinearize and the automorphism: against the limb-wise 60-bit MAC, item 0 against the oracle
    ref = ks32_ctx(prm, False)
    assert ref.ks32_primes == 0
    ref.load_relin_key(rlk)
    ct3 = uniform_residues(rng, (B, 3), q, n)
    got = ctx.relinearize(ct3)
    assert np.array_equal(got, ref.relinearize(ct3))
    assert np.array_equal(got[0], ct_to_np(obfv.relinearize(np_to_ct(ct3[0], prm), np_to_rlk(rlk, prm))))
    for element in (3, 2 * n - 1):
        gk = uniform_residues(rng, (prm.gadget_digits, 2), q, n)
        got = ctx.bfv_apply_automorphism(ct1, element, gk)
        assert np.array_equal(got, ref.bfv_apply_automorphism(ct1, element, gk)), element
        if element == 3:
            keyset = obfv.GaloisKey(np_to_rlk(gk, prm).keys, element, prm)
            assert np.array_equal(got[0], ct_to_np(obfv.bfv_apply_automorphism(np_to_ct(ct1[0], prm), keyset)))


@pytest.mark.parametrize("base", [255, 1000])
def test_hps_compact_other_bases(gpu_available, base):
    """compact_bfv (n = 1024, one auxiliary prime) with a gadget base that is no power of two."""
    c = P.compact_bfv()
    prm = params(c.ring_degree, c.ct_basis.moduli, c.plain_modulus, base, c.aux_basis.moduli)
    n, q = prm.ring_degree, prm.ct_basis.moduli
    rng = np.random.default_rng(base)
    ctx = HipContext.from_params(prm)
    assert ctx.path == PATH_HPS and ctx.G == prm.gadget_digits
    ct1, ct2 = uniform_residues(rng, (3, 2), q, n), uniform_residues(rng, (3, 2), q, n)
    rlk = uniform_residues(rng, (prm.gadget_digits, 2), q, n)
    ctx.load_relin_key(rlk)
    got = ctx.bfv_mul_and_relin(ct1, ct2)
    key = np_to_rlk(rlk, prm)
    for i in range(3):
        want = obfv.bfv_mul_and_relin(np_to_ct(ct1[i], prm), np_to_ct(ct2[i], prm), key)
        assert np.array_equal(got[i], ct_to_np(want)), i


def test_hps_digit_sums_base_255(gpu_available):
    """u64_dbfv's parameters with gadget base 255: the HPS digit-sum path (n >= 1024: the products' int8
    digits from the generic routine, summed per output limb before one MAC)."""
    u = P.u64_dbfv()
    c = u.bfv_params
    prm = params(c.ring_degree, c.ct_basis.moduli, c.plain_modulus, 255, c.aux_basis.moduli)
    dp = P.DbfvParams(prm, u.base, u.num_digits, u.plain_modulus)
    n, q, d = prm.ring_degree, prm.ct_basis.moduli, dp.num_digits
    rng = np.random.default_rng(255)
    ctx = HipContext.from_params(prm)
    assert ctx.path == PATH_HPS and ctx.G == prm.gadget_digits == 8
    a, b = uniform_residues(rng, (2, d, 2), q, n), uniform_residues(rng, (2, d, 2), q, n)
    rlk = uniform_residues(rng, (prm.gadget_digits, 2), q, n)
    ctx.load_relin_key(rlk)
    out, _ = ctx.dbfv_mul(d, dp.base, dp.plain_modulus, a, b)
    assert np.array_equal(out, cref.dbfv_mul(dp, a, b, rlk, threads=8))


# ------------------------------------------------------------------ d. the limits ceil(B/2) decides

def times(ct, m, q):
    """m * ct mod q_l per limb ([..][L][n] canonical residues)."""
    qs = np.array(q, dtype=object)[:, None]
    return ((m * ct.astype(object)) % qs).astype(np.uint64)


def int16_sum_case(n=1024, base=21845):
    prm = params(n, P.Q3, 65537, base)
    q, G = prm.ct_basis.moduli, prm.gadget_digits
    ct1, ct2, _, gp = W.digit_case_bfv(q, prm.plain_modulus, base, G, n, seed=21)
    assert (G, gp) == (13, 12)                 # every coefficient of c2: twelve digits of -10923
    rlk = uniform_residues(np.random.default_rng(22), (G, 2), q, n)
    return prm, ct1, ct2, rlk


def test_int16_digit_sums_base_21845_mul_sum(gpu_available):
    """Three products whose every digit is -10923 = -ceil(21845/2), key-switched as one sum: the
    summed digits are -32769, outside int16 (3 * floor(21845/2) = 32766 is inside).  With floor(B/2) in
    the library's int16 test the sums were stored as +32767: last_mode 1 and all 6144 coefficients
    wrong for three products, none for one or two (measured on an MI355X)."""
    prm, ct1, ct2, rlk = int16_sum_case()
    q = prm.ct_basis.moduli
    ctx = HipContext.from_params(prm)
    assert ctx.ks32_primes > 0
    ctx.load_relin_key(rlk)
    assert ctx.mul_sum_info()["group_max"] >= 3
    got = ctx.bfv_mul_sum(ct1[:, None], ct2[:, None], [(0, 0, 0)] * 3, 1)
    mode = ctx.mul_sum_info()["last_mode"]
    print("base 21845, three products in one slot: last_mode", mode)
    assert mode in (1, 2)                      # the three really were key-switched as one sum
    want = times(cref.bfv_mul_and_relin(prm, ct1, ct2, rlk), 3, q)
    print("coefficients that differ:", int((got[:, 0] != want).sum()), "of", want.size)
    assert np.array_equal(got[:, 0], want)


def test_int16_digit_sums_base_21845_dbfv(gpu_available):
    """The same through dbfv_mul with d = 3 and all limbs alike: limb 2 sums three products' digits
    (with floor(B/2): dbfv_key_switch 1, limbs 0 and 1 exact, all 6144 coefficients of limb 2 wrong)."""
    prm, ct1, ct2, rlk = int16_sum_case()
    q = prm.ct_basis.moduli
    dp = P.DbfvParams(prm, 16, 3, 4096)
    a, b = np.repeat(ct1[:, None], 3, axis=1), np.repeat(ct2[:, None], 3, axis=1)
    ctx = HipContext.from_params(prm)
    ctx.load_relin_key(rlk)
    out, _ = ctx.dbfv_mul(3, dp.base, dp.plain_modulus, a, b)
    print("base 21845, dbfv_mul d = 3: dbfv_key_switch", ctx.dbfv_key_switch)
    assert ctx.dbfv_key_switch in (1, 2)
    want = cref.dbfv_mul(dp, a, b, rlk, threads=4)
    print("coefficients that differ:", int((out != want).sum()), "of", want.size)
    assert np.array_equal(out, want)


def basis_bound_case(n=8192, base=711):
    prm = params(n, P.Q3, 65537, base)
    q, G = prm.ct_basis.moduli, prm.gadget_digits
    ct1, ct2, rlk, gp = W.digit_case_bfv(q, prm.plain_modulus, base, G, n, seed=31)
    assert G == gp == 19                       # all 19 digits of every coefficient of c2 are -356
    return prm, ct1, ct2, rlk


def test_basis_bound_base_711_at_the_limit(gpu_available):
    """cfg3's moduli, n = 8192, base 711, every digit -356 and the key sign-aligned: coefficient 0 of
    one product's key switch is 19 * 8192 * 356 * floor(q/2).  The primary (narrow) basis runs sums of
    at most m products, m its own limit from prod p > 2 m G n ceil(B/2) floor(q/2) (45; with floor(B/2)
    the rule said 46, whose sum exceeds prod p / 2).  Sums of m are exact on the primary basis, a sum
    of m + 1 goes to the wide basis, or with the limit set to m, to groups of m and 1.
    group_max reports 64 here, the wide basis' limit (primes up to 2^31); the primary basis' own limit
    shows in last_mode.  Measured on an MI355X with floor(B/2) in the library: 45 products exact, 46
    last_mode 1 and all 49152 coefficients wrong, 47 and 64 last_mode 2 and exact."""
    prm, ct1, ct2, rlk = basis_bound_case()
    n, q, G, base = prm.ring_degree, prm.ct_basis.moduli, prm.gadget_digits, prm.gadget_base
    basis = W.ks32_basis(n, max(q), base, G, (1 << 32) // 3)
    m = W.ks32_sum_max(basis, n, max(q), base, G)
    u0 = G * n * W.digit_max(base) * (max(q) // 2)
    assert 2 * m * u0 < math.prod(basis) < 2 * (m + 1) * u0      # m products lift, m + 1 would wrap
    ctx = HipContext.from_params(prm)
    assert ctx.ks32_primes == len(basis) == 3
    ctx.load_relin_key(rlk)
    info = ctx.mul_sum_info()
    print("base 711: group_max", info["group_max"], "restated primary limit", m)
    assert info["group_max"] >= m
    one = cref.bfv_mul_and_relin(prm, ct1, ct2, rlk, threads=1)
    a, b = ct1[:, None], ct2[:, None]

    got = ctx.bfv_mul_sum(a, b, [(0, 0, 0)] * m, 1)
    assert not ctx.ks32_lazy                   # the aligned key's norms exceed the lazy basis' bound
    assert ctx.mul_sum_info()["last_mode"] == 1
    assert np.array_equal(got[:, 0], times(one, m, q)), "m products on the primary basis"

    got = ctx.bfv_mul_sum(a, b, [(0, 0, 0)] * (m + 1), 1)
    # one more than the primary basis lifts: the wide basis where the context has one, else groups
    mode = ctx.mul_sum_info()["last_mode"]
    print("base 711: m + 1 products, last_mode", mode)
    assert mode == (2 if info["group_max"] > m else 1)
    assert np.array_equal(got[:, 0], times(one, m + 1, q)), "m + 1 products"

    ctx.set_mul_sum_group(m)
    assert ctx.mul_sum_info()["group_max"] == m
    got = ctx.bfv_mul_sum(a, b, [(0, 0, 0)] * (m + 1), 1)
    assert ctx.mul_sum_info()["last_mode"] == 1
    assert np.array_equal(got[:, 0], times(one, m + 1, q)), "m + 1 products in groups of m and 1"

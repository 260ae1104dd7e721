"""The dispatch-matrix table (tests/dispatch_cases.py) is what it says it is: its primes are the nearest
usable primes on the stated side of each threshold, its cases cover both sides of every threshold and
every ring degree, the selection written next to each case follows from the library's conditions, and the
reference the GPU matrix compares against (oracle/c) agrees with the Python restatement on a small
product of every prime class."""

import os

import numpy as np
import pytest

import dispatch_cases as D
from dispatch_cases import CASES, EDGE, STEP, T60, THRESHOLDS
from test_fpc_crt import is_prime
from oracle import bfv as obfv, cref, params as P
from bridge import ct_to_np, np_to_ct, np_to_rlk, uniform_residues

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _all_primes(case):
    return list(case.ct) + list(case.aux)


def test_every_prime_is_prime_and_fits_its_ring():
    for c in CASES:
        for q in _all_primes(c):
            assert is_prime(q), (c.name, q)
            assert q % (2 * c.n) == 1, (c.name, q)
        assert len(set(_all_primes(c))) == len(_all_primes(c)), c.name
    for name, sides in EDGE.items():
        for side, ps in sides.items():
            assert all(is_prime(q) and q % STEP == 1 for q in ps), (name, side)
    assert is_prime(D.BIG62) and D.BIG62 % STEP == 1 and D.BIG62 >= T60


@pytest.mark.parametrize("name", sorted(THRESHOLDS))
def test_edge_primes_are_the_nearest_on_their_side(name):
    thr = THRESHOLDS[name]
    for side in ("below", "above"):
        found = D.edge_primes(STEP, thr, side, 3)
        assert found == EDGE[name][side], (name, side, found)
        # the stated side, nearest first, and nothing usable in between
        dist = [thr - q if side == "below" else q - thr for q in found]
        assert all(x > 0 for x in dist) and dist == sorted(dist)
        lo, hi = (found[-1], thr) if side == "below" else (thr, found[-1])
        between = [q for q in range(lo // STEP * STEP + 1, hi + 1, STEP) if lo <= q <= hi and q != thr and is_prime(q)]
        assert sorted(between) == sorted(found), (name, side)


def test_issue_cross_check_values():
    """d = 2^60 - q of the nearest primes, as found independently when the matrix was specified."""
    d = lambda name, side: [T60 - q for q in EDGE[name][side][:2]]
    assert d("w32", "below") == [4295065599, 4295786495] and d("w32", "above") == [4294082559, 4293328895]
    assert d("w24", "below") == [16908287, 18776063] and d("w24", "above") == [15826943, 15630335]
    assert d("p60", "below") == [98303, 163839] and d("p60", "above") == [-491521, -1900545]


def test_prime_classes():
    cls = lambda ps: {D.prime_class(q) for q in ps}
    assert cls(EDGE["w32"]["below"]) == {"generic"} and cls(EDGE["w32"]["above"]) == {"C"}
    assert cls(EDGE["w24"]["below"]) == {"C"} and cls(EDGE["w24"]["above"]) == {"special"}
    assert cls(EDGE["p60"]["below"]) == {"special"} and cls(EDGE["p60"]["above"]) == {"big"}
    assert cls(D.CLASS_C4) == {"C"} and len(set(D.CLASS_C4)) == 4
    # class C spans its window: d just below 2^32 and d just above 2^24
    ds = sorted(T60 - q for q in D.CLASS_C4)
    assert ds[0] < (1 << 24) + (1 << 22) and ds[-1] > (1 << 32) - (1 << 21)


def test_every_threshold_has_a_case_on_each_side():
    for name, thr in THRESHOLDS.items():
        below = [c.name for c in CASES if c.group == "edge" and all(q < thr for q in _all_primes(c))
                 and set(_all_primes(c)) <= set(EDGE[name]["below"])]
        above = [c.name for c in CASES if c.group == "edge" and all(q > thr for q in _all_primes(c))
                 and set(_all_primes(c)) <= set(EDGE[name]["above"])]
        assert below and above, (name, below, above)
        for nm in below + above:          # ... and uses the nearest primes, nearest first
            c, side = D.BY_NAME[nm], "below" if nm in below else "above"
            assert _all_primes(c) == EDGE[name][side][:len(_all_primes(c))], nm
    # the two sides of a threshold differ in what they select
    for name in THRESHOLDS:
        n = 1024 if name == "g50" else 4096
        assert D.BY_NAME[f"{name}_below_n{n}"].expect != D.BY_NAME[f"{name}_above_n{n}"].expect, name


def test_every_logn_has_a_multiply_case():
    assert {c.n.bit_length() - 1 for c in CASES} >= set(range(4, 15))
    assert len({c.name for c in CASES}) == len(CASES)
    # the sizes the suite multiplied at nowhere else, on the exact path and on HPS
    assert {c.n for c in CASES if c.group == "sweep_exact"} >= {32, 128, 512, 2048, 16384}
    assert {c.n for c in CASES if c.group == "sweep_hps" and len(c.aux) == 1} == {128, 512, 2048}
    assert {c.n for c in CASES if c.group == "sweep_hps" and len(c.aux) == 2} == {512, 2048}
    assert all(c.B <= 2 for c in CASES)


def test_expectations_follow_from_the_conditions():
    for c in CASES:
        assert D.select(c.n, c.ct, c.aux, c.plain, c.gbase) == c.expect, c.name
    # the mixed path the 2^32 window exists for: pinned forward NTT, generic tensor and scale, limb-wise MAC
    for nm in ("classC_L2_n4096", "mixed_L3_n8192", "classC_L3_n4096", "w24_below_n4096", "w32_above_n4096"):
        e = D.BY_NAME[nm].expect
        assert e.fwd_pinned and not e.tensor_asm and not e.ks32 and not e.scale_sp, nm
    # one class C prime among special ones flips every all-primes condition
    assert D.BY_NAME["mixed_L3_n4096"].expect == D.BY_NAME["classC_L3_n4096"].expect
    assert [D.prime_class(q) for q in D.BY_NAME["mixed_L3_n4096"].ct] == ["special", "special", "C"]
    assert D.DBFV_MIXED["ct"] == D.BY_NAME["mixed_L3_n4096"].ct


def test_hps_cases_satisfy_the_reference_bounds():
    """bfv_mul_hps (eval.rs:157-413): a single auxiliary prime must exceed n q / 2.  compact_bfv's auxiliary
    prime is 1 mod 2048 but not mod 4096 and below n q / 2 at n = 2048: no context exists for that pair
    there, which is why sweep_hps1_n2048 keeps compact_bfv's q and takes u64_dbfv's 2^55 prime."""
    for c in CASES:
        if c.expect.path == D.PATH_HPS and len(c.aux) == 1:
            assert c.aux[0] > c.n * c.ct[0] // 2, c.name
    assert D.COMPACT_AUX <= 2048 * D.COMPACT_Q // 2 and D.COMPACT_AUX % 4096 != 1
    assert D.BY_NAME["sweep_hps1_n2048"].ct == [D.COMPACT_Q]
    # same-size primes can never be a single-aux pair: the gen_qb neighbours take two auxiliary primes
    for nm in ("g50_below_n1024", "g56_below_n4096"):
        c = D.BY_NAME[nm]
        assert c.aux[0] <= c.n * c.ct[0] // 2 and len(c.aux) == 2


@pytest.mark.parametrize("name", ["p60_below_n4096", "w24_below_n4096", "w32_below_n4096", "p60_above_n4096",
                                  "mixed_L3_n4096", "big_L2_n4096", "g50_below_n1024", "g56_above_n4096",
                                  "sweep_hps1_n128", "sweep_hps2_n512"])
def test_cref_matches_python_oracle_per_class(name):
    """The reference of the GPU matrix is itself pinned: oracle/c == the Python restatement on a product
    over each class's primes (special, C, generic, big, mixed, both HPS forms) at n = 16."""
    assert cref.available(), "oracle/c/liboracle.so is not built: run build() of __graft_entry__.py"
    c = D.BY_NAME[name]
    n = 16
    prm = (P.BfvParamsBuilder().ring_degree(n).plain_modulus(c.plain).ct_moduli(c.ct).aux_moduli(c.aux)
           .gadget_base(c.gbase).build())
    q = prm.ct_basis.moduli
    rng = np.random.default_rng(len(name))
    ct1 = uniform_residues(rng, (2, 2), q, n)
    ct2 = uniform_residues(rng, (2, 2), q, n)
    ct1[0, 1] = np.array(q, dtype=np.uint64)[:, None] - 1
    rlk = uniform_residues(rng, (prm.gadget_digits, 2), q, n)
    got3 = cref.bfv_mul(prm, ct1, ct2, relin=False)
    got2 = cref.bfv_mul(prm, ct1, ct2, rlk, relin=True)
    for i in range(2):
        a, b = np_to_ct(ct1[i], prm), np_to_ct(ct2[i], prm)
        assert np.array_equal(got3[i], ct_to_np(obfv.bfv_mul_no_relin(a, b))), (name, i)
        assert np.array_equal(got2[i], ct_to_np(obfv.bfv_mul_and_relin(a, b, np_to_rlk(rlk, prm)))), (name, i)


@pytest.mark.parametrize("name", ["sweep_exact_n256", "mixed_L3_n4096", "big_L2_n4096"])
def test_cref_threaded_product_equals_serial(name):
    """oracle_bfv_mul with more threads than products splits each schoolbook over the threads by output
    coefficient; the result is the serial one bit for bit (n = 256: both wrap directions, every limb count
    of the matrix)."""
    assert cref.available(), "oracle/c/liboracle.so is not built: run build() of __graft_entry__.py"
    c = D.BY_NAME[name]
    n = 256
    prm = P.BfvParamsBuilder().ring_degree(n).plain_modulus(c.plain).ct_moduli(c.ct).gadget_base(c.gbase).build()
    q = prm.ct_basis.moduli
    rng = np.random.default_rng(n + len(q))
    ct1 = uniform_residues(rng, (2, 2), q, n)
    ct2 = uniform_residues(rng, (2, 2), q, n)
    ct1[0, 1] = np.array(q, dtype=np.uint64)[:, None] - 1
    rlk = uniform_residues(rng, (prm.gadget_digits, 2), q, n)
    for relin in (False, True):
        serial = cref.bfv_mul(prm, ct1, ct2, rlk, relin=relin, threads=1)
        assert np.array_equal(cref.bfv_mul(prm, ct1, ct2, rlk, relin=relin, threads=2), serial)    # per product
        assert np.array_equal(cref.bfv_mul(prm, ct1, ct2, rlk, relin=relin, threads=5), serial)    # per coefficient


def test_design_table_matches_the_cases():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    assert D.design_table() in text, "DESIGN.md's dispatch matrix differs from dispatch_cases.design_table()"

"""The largest balanced gadget digit is ceil(B/2), not floor(B/2), and what follows from it (CPU).

keyswitch.rs:24-44 balances a truncating remainder with `rem >= half_base -> rem -= base`,
half_base = B / 2 truncated: a positive remainder equal to floor(B/2) becomes -(B - floor(B/2)), which
for an odd base is -(B+1)/2.  Every exactness limit the library derives from the digit size (the
31-bit key-switch basis and the products it may sum before one lift, the int16 digit sums;
DESIGN.md §4) therefore has to use ceil(B/2).  With floor(B/2) in its place two limits are wrong for
odd bases, shown here on the restated rules of tests/worstcase.py and on the GPU in
tests/test_gpu_gadget_bases.py:

* the basis rule allows 46 summed products at cfg3's moduli, n = 8192, base 711, whose worst case
  exceeds prod p / 2: the centred lift wraps;
* three summed digits of base 21845 are classed as fitting int16, and reach -32769.
"""

import math
import random

import pytest

from oracle.bfv import gadget_decompose_coeff
from oracle.params import Q3, compute_gadget_digits
import worstcase as W

Q40 = [1099509805057]
Q2 = [65537, 1099509805057]            # the two-prime Q < 2^64 of test_gpu_galois.py
MODULI = {"q40": Q40, "q2": Q2, "cfg3": Q3}
ODD = [3, 5, 9, 255, 711, 1923, 21845, 65535]
EVEN = [4, 10, 1000, 65536]
PMAX = (1 << 32) // 3                  # the primary (narrow) 31-bit basis


def centred(d, Q):
    return d - Q if d > Q // 2 else d


@pytest.mark.parametrize("which", sorted(MODULI))
@pytest.mark.parametrize("base", ODD + EVEN)
def test_largest_digit_is_ceil_half_base_and_attained(which, base):
    Q = math.prod(MODULI[which])
    G = compute_gadget_digits(MODULI[which], base)
    hi = (base + 1) // 2
    assert W.digit_max(base) == hi
    rng = random.Random(base)
    values = W.crafted_values(Q, base, G) + [rng.randrange(Q) for _ in range(10_000)]
    worst, lowest = 0, 0
    for v in values:
        digits = [centred(d, Q) for d in gadget_decompose_coeff(v, Q, base, G)]
        worst = max(worst, max(abs(d) for d in digits))
        lowest = min(lowest, min(digits))
        assert max(digits) <= base - hi        # [-ceil(B/2), floor(B/2)]: only the negative side reaches hi
    assert worst == hi and lowest == -hi


@pytest.mark.parametrize("which", sorted(MODULI))
@pytest.mark.parametrize("base", [b for b in range(5, 400, 2)] + [711, 1001, 1923, 9363, 21845, 32767, 65535]
                         + [4, 10, 256, 1000, 65536])
def test_digit_target_has_every_low_digit_at_minus_hi(which, base):
    Q = math.prod(MODULI[which])
    G = compute_gadget_digits(MODULI[which], base)
    x, gp = W.digit_target(Q, base, G)
    hi = W.digit_max(base)
    assert 0 < abs(x) <= Q // 2 and G - 2 <= gp <= G
    digits = [centred(d, Q) for d in gadget_decompose_coeff(x % Q, Q, base, G)]
    assert digits[:gp] == [-hi] * gp
    if gp < G:   # even: nothing above the target; odd: the 1 the target was built from
        assert digits[gp:] == [base % 2] + [0] * (G - gp - 1)
    # one more digit does not fit: the next value of the construction leaves [-Q/2, Q/2]
    if gp < G:
        assert (x * base - hi if base % 2 else -x * base + hi) > Q // 2


def test_digit_target_even_bases_unchanged():
    # the even-base targets test_worstcase_bounds.py and the committed worst-case digests were built from
    for q, base, G in ((Q3, 1 << 16, 12), (Q3 + [1152921504606601217], 256, 30)):
        Q = math.prod(q)
        x, gp = W.digit_target(Q, base, G)
        assert gp == G - 1 and x == -(base // 2) * (base ** gp - 1) // (base - 1)


def worst_u0(moduli, n, base, G, m=1):
    """Coefficient 0 of the summed key switch of m products of digit_inputs with aligned_key, the
    largest over the limbs: every digit below G' is -hi, digit G' (odd base, G' < G) is +1."""
    Q = math.prod(moduli)
    x, gp = W.digit_target(Q, base, G)
    digits = [centred(d, Q) for d in gadget_decompose_coeff(x % Q, Q, base, G)]
    return m * -sum(digits) * n * (max(moduli) // 2)


def test_basis_rule_with_floor_half_base_lets_the_lift_wrap():
    """cfg3's moduli, n = 8192, base 711 (G = 19): a value <= Q/2 has all 19 digits at -356.  The rule
    with floor(711/2) = 355 picks three narrow primes and takes them to lift 46 summed products, whose
    worst case exceeds prod p / 2."""
    n, base, qmax = 8192, 711, max(Q3)
    G = compute_gadget_digits(Q3, base)
    assert G == 19 and W.digit_target(math.prod(Q3), base, G)[1] == G
    floor_basis = W.ks32_basis(n, qmax, base, G, PMAX, hi=base // 2)
    assert len(floor_basis) == 3
    assert W.ks32_sum_max(floor_basis, n, qmax, base, G, hi=base // 2) == 46
    u0 = worst_u0(Q3, n, base, G, m=46)
    assert u0 == 46 * 19 * 8192 * 356 * (qmax // 2)
    assert 2 * u0 > math.prod(floor_basis)
    assert W.lift_centred(u0, floor_basis) != u0


def test_basis_rule_lifts_its_own_limit_for_odd_bases():
    """The rule as the library states it (tests/worstcase.py ks32_basis / ks32_sum_max) lifts the worst
    case of as many summed products as it allows, at the margins found for odd bases."""
    Q4 = Q3 + [1152921504606601217]
    for moduli, n, base in ((Q3, 8192, 711), (Q4, 4096, 777), (Q4, 4096, 1385), (Q3, 1024, 21845),
                            (Q3[1:], 1024, 1923)):
        qmax = max(moduli)
        G = compute_gadget_digits(moduli, base)
        basis = W.ks32_basis(n, qmax, base, G, PMAX)
        assert basis is not None
        m = W.ks32_sum_max(basis, n, qmax, base, G)
        assert m >= 1
        u0 = worst_u0(moduli, n, base, G, m)
        assert W.lift_centred(u0, basis) == u0, (n, base, m)
        assert W.lift_centred(-u0, basis) == -u0, (n, base, m)
    # base 711: one product fewer than the floor rule allowed
    G = compute_gadget_digits(Q3, 711)
    basis = W.ks32_basis(8192, max(Q3), 711, G, PMAX)
    assert W.ks32_sum_max(basis, 8192, max(Q3), 711, G) == 45


def test_int16_digit_sums_of_odd_bases():
    """m digits of -ceil(B/2) leave int16 where m floor(B/2) does not: such sums are kept as int32."""
    for m, base in ((3, 21845), (5, 13107), (6, 10923), (7, 9363)):
        assert m * (base // 2) <= 32767 < 32768 < m * W.digit_max(base)
        assert not W.int16_sums_wide(m, base, hi=base // 2)     # the rule with floor(B/2): int16
        assert W.int16_sums_wide(m, base)                       # the rule: int32
    # cfg3's moduli, n = 1024, base 21845 (G = 13): three products are key-switched as one sum
    G = compute_gadget_digits(Q3, 21845)
    basis = W.ks32_basis(1024, max(Q3), 21845, G, PMAX)
    assert G == 13 and len(basis) == 3 and W.ks32_sum_max(basis, 1024, max(Q3), 21845, G) >= 3
    # even bases: nothing changes (cfg5 sums 8 digits of base 256, cfg4 two of base 2^16)
    for m, base in ((8, 256), (2, 1 << 16), (1, 1 << 16), (64, 1024)):
        assert W.int16_sums_wide(m, base) == W.int16_sums_wide(m, base, hi=base // 2)

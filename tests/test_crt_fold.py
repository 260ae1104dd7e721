"""CPU check of the scale's CRT factors folded into the tensor's last inverse stage (EXACTO_CRT_FOLD:
context.hip PrimeConst::fold_*, ntt.hip make_asmk_inv_fold, kernels.hip fpq_y / fpc_y_garner FOLD).

The folding tensor kernel leaves z_i = T_i p (Q / q_i)^-1 mod q_i and t_a = T_a fpc_pq[a] mod p_a, both in
[0, 2q) (its lazy last stage).  fpq_y then takes the z_i as they are: f = the fused multiply-adds
z0_i fl(1 / q_i) + z1_i fl(2^30 / q_i) over their 30-bit halves, beta = rint(f) (up to 2 L: a z_i of q_i
more raises it by one), and wherever |f - beta| <= 1/2 - 2^-40
  sum_i z_i (Q / q_i) - beta Q = s, the centred [p T]_Q, and
  y_a = t_a + sum_i z_i fpq_c[i][a] + beta Pi_a  (mod p_a)
by one 30-bit-limb dot with t_a in its a0 column; elsewhere the lane recovers u_i = z_i (Q / q_i) mod q_i
= p T_i and takes Garner over Q.  Checked against exact integers and against the Garner path's y_a, with
every column of the dot held against its 64-bit register, for cfg3's moduli (L = 3) and L = 1, 2, 4, 5.

A Python restatement of the device arithmetic (each fp64 operation correctly rounded), not the kernels;
those run the same boundary in tests/test_gpu_crt_fold.py and tests/test_gpu_fp_boundary.py."""
import random

import pytest

from test_fpc_crt import Q3, Q4
from test_fpq import LIM, M30, fma, rint, consts, garner_s

N, PLAIN = 4096, 65537
U64 = 1 << 64


def bases():
    from fp_boundary import low_window_primes
    return {1: Q3[:1], 2: Q3[:2], 3: Q3, 4: Q4, 5: Q4 + low_window_primes(16384, 1)}


def float_sum(z, qs):
    f = 0.0
    for v, q in zip(z, qs):
        assert v >> 30 < 1 << 32
        f = fma(float(v & M30), 1.0 / q, f)
        f = fma(float(v >> 30), float(1 << 30) / float(q), f)
    return f, rint(f)


def dot30(a0, terms, q):
    """dot30_mac over (x, c) terms on top of a0, then dot30_fold and reduce_near60: every column and every
    partial sum is held against its 64-bit register; returns the canonical residue."""
    a1 = a2 = 0
    for x, c in terms:
        x0, x1, c0, c1 = x & M30, x >> 30, c & M30, c >> 30
        assert x1 < 1 << 32 and c1 < 1 << 32
        a0 += x0 * c0
        a1 += x0 * c1 + x1 * c0
        a2 += x1 * c1
        assert max(a0, a1, a2) < U64
    d = (1 << 60) - q
    H = a2 + (a1 >> 30)
    assert H < U64
    F = (H >> 32) * d
    assert F >> 28 < 1 << 32
    x = a0
    for t in ((H & 0xFFFFFFFF) * d, (a1 & M30) << 30, (F & ((1 << 28) - 1)) << 32, (F >> 28) * d):
        x += t
        assert x < U64
    r = (x & ((1 << 60) - 1)) + (x >> 60) * d
    assert r < 2 * q
    return r - q if r >= q else r


def folded_scale(T, Ta, lazy, qs, c):
    """fpq_y FOLD on the tensor's outputs for residues T (mod q_i) and Ta (mod p_a); lazy[i] / lazy[L + a]
    say which of them the last stage left in [q, 2q).  True when the float sum was taken."""
    ps, Q, pi, pz, fq, pq, fqpq = c
    L = len(qs)
    s, v, negs = garner_s(T, PLAIN, qs)
    z = [t * w % q + (q if lz else 0) for t, w, q, lz in zip(T, pz, qs, lazy)]
    ta = [t * w % pa + (pa if lz else 0) for t, w, pa, lz in zip(Ta, pq, ps, lazy[L:])]
    want = [(Ta[a] * pq[a] + sum(vk * fqpq[k][a] for k, vk in enumerate(v)) + (pi[a] if negs else 0)) % pa
            for a, pa in enumerate(ps)]
    f, b = float_sum(z, qs)
    if abs(f - b) > LIM:
        # the band: one Shoup product by (Q / q_i) takes z_i back to u_i = p T_i, then Garner as before
        assert [zi * ((Q // q) % q) % q for zi, q in zip(z, qs)] == [PLAIN * t % q for t, q in zip(T, qs)]
        got = [dot30((pi[a] if negs else 0) + ta[a], [(vk, fqpq[k][a]) for k, vk in enumerate(v)], pa)
               for a, pa in enumerate(ps)]
        assert got == want
        return False
    beta = int(b)
    assert 0 <= beta <= 2 * L
    assert sum(zi * (Q // q) for zi, q in zip(z, qs)) - beta * Q == s        # beta is exact
    got = [dot30(ta[a], [(beta, pi[a])] + [(zi, fq[i][a]) for i, zi in enumerate(z)], pa) for a, pa in enumerate(ps)]
    assert got == want
    return True


@pytest.mark.parametrize("L", [1, 2, 3, 4, 5])
def test_folded_scale_matches_garner(L):
    qs = bases()[L]
    c = consts(N, PLAIN, qs)
    ps, Q = c[0], c[1]
    rng = random.Random(31 + L)
    pinv = pow(PLAIN, -1, Q)
    h = Q // 2
    res = lambda x: [x % q for q in qs]
    some = lambda: [rng.random() < 0.5 for _ in range(L + len(ps))]
    top, low = [True] * (L + len(ps)), [False] * (L + len(ps))
    aux = lambda: [rng.randrange(pa) for pa in ps]
    # s next to +-floor(Q/2) and 2^-45 Q from it: the float sum cannot centre it, the band must say so
    for s in [h + k for k in range(-3, 5)] + [h - (Q >> 45), h + 1 + (Q >> 45)]:
        for lazy in (low, top, some()):
            assert folded_scale(res(s * pinv % Q), aux(), lazy, qs, c) is False, s
    # 2^-38 Q from it: outside the band, whatever the last stage left lazy
    for s in (h - (Q >> 38), h + 1 + (Q >> 38)):
        for lazy in (low, top, some()):
            assert folded_scale(res(s * pinv % Q), aux(), lazy, qs, c) is True, s
    # zeros, Q - 1, every residue q_i - 1 and p_a - 1, and every z_i and t_a at the top of [0, 2q)
    ztop = [(q - 1) * pow(w, -1, q) % q for q, w in zip(qs, c[3])]          # z_i = q_i - 1 (+ q_i when lazy)
    ttop = [(pa - 1) * pow(w, -1, pa) % pa for pa, w in zip(ps, c[5])]
    for T, Ta in ((res(0), [0] * len(ps)), (res(Q - 1), aux()), ([q - 1 for q in qs], [pa - 1 for pa in ps]),
                  (ztop, ttop)):
        for lazy in (low, top):
            folded_scale(T, Ta, lazy, qs, c)
    taken = sum(folded_scale([rng.randrange(q) for q in qs], aux(), some(), qs, c) for _ in range(2500))
    assert taken == 2500          # a uniform value falls in the band with probability 2^-39


@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_band_catches_every_inexact_lane(L):
    """s swept across +-Q/2 at distances 2^-k Q, every z_i lazy or none: wherever rint(f) is not the exact
    quotient, |f - beta| > lim; inside 2^-41 Q always, outside 2^-39 Q never."""
    qs = bases()[L]
    ps, Q, pi, pz = consts(N, PLAIN, qs)[:4]
    pinv = pow(PLAIN, -1, Q)
    h = Q // 2
    for k in range(30, 60):
        for base in (h, h + 1):
            for sg in (1, -1):
                s = (base + sg * (Q >> k)) % Q
                x = s * pinv % Q
                for add in (0, 1):
                    z = [x % q * w % q + add * q for q, w in zip(qs, pz)]
                    f, b = float_sum(z, qs)
                    exact = sum(v * (Q // q) for v, q in zip(z, qs)) - int(b) * Q == (s - Q if s > h else s)
                    if not exact or k >= 41:
                        assert abs(f - b) > LIM, (L, k, sg, add)
                    if k <= 39:
                        assert exact and abs(f - b) <= LIM, (L, k, sg, add)


def fourth_root(q):
    g = 2
    while pow(g, (q - 1) // 2, q) != q - 1:
        g += 1
    r = pow(g, (q - 1) // 4, q)
    assert r * r % q == q - 1
    return r


@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_folded_constants_multiply_out(L):
    """n^-1 c and last_w c (last_w = psi^-(n/2) n^-1: a fourth root of unity times n^-1) times c^-1 are the
    unfolded constants, for c = p (Q / q_i)^-1 mod q_i and c = fpc_pq[a]; and (Q / q_i) takes z_i back."""
    qs = bases()[L]
    ps, Q, pi, pz, fq, pq, fqpq = consts(N, PLAIN, qs)
    for q, cf in list(zip(qs, pz)) + list(zip(ps, pq)):
        n_inv = pow(N, -1, q)
        last_w = pow(fourth_root(q), -1, q) * n_inv % q
        cinv = pow(cf, -1, q)
        assert n_inv * cf % q * cinv % q == n_inv
        assert last_w * cf % q * cinv % q == last_w
    for q, w in zip(qs, pz):
        assert w * ((Q // q) % q) % q == PLAIN % q            # fpc_y_garner FOLD: u_i = z_i (Q / q_i) = p T_i

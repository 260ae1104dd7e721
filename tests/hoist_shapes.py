"""The launch shapes of the hoisted rotations (hoist.hip, ks32.hip's ks32_mac_hoist_kernel, hoist_core in
context.hip) and a table of cases that reaches each of them at the smallest ring (test helper, no GPU use;
tests/test_hoist_shapes.py holds the table against the dispatch, tests/test_gpu_hoist_shapes.py runs it).

mac_block_shape, limbwise_kernel and launch_items restate the library's selection, so a case can say which
kernel instantiation it exists for and the GPU test can assert that the context it built takes that one.
"""

from __future__ import annotations

import functools
from typing import Callable, NamedTuple

import numpy as np

from bridge import uniform_residues
from oracle import params as P

KS_LS = 64        # ks32.hip: positions per block of the 31-bit MAC
HO_LS = 64        # hoist.hip: positions per block of hoist_mac_lds_kernel
HO_IG = 64        # ... and its items per block
HO_GMAX = 32      # ... and the digits it stages in LDS
HO_TPB = 256      # hoist.hip: threads per block of the plain kernels
RUN = 12          # products per reduction of the narrow and lazy 31-bit forms (7 in the wide form)


def mac_block_shape(guse: int, L: int) -> tuple[int, int]:
    """(CLB limb pairs per block, NW waves) of ks32_mac_hoist_kernel: ks32_mac_hoist in ks32.hip.  CLB is the
    largest divisor of 2L whose key slice (guse * CLB rows of 64 ints) fits 64 KiB of LDS; more than 32 KiB
    takes eight waves.  A block owns 4 * NW items."""
    CL = 2 * L
    CLB = CL
    while CLB > 1 and (CL % CLB != 0 or guse * CLB * KS_LS * 4 > 65536):
        CLB -= 1
    return CLB, (8 if guse * CLB * KS_LS * 4 > 32768 else 4)


def limbwise_kernel(guse: int, L: int, n: int, lt: bool) -> str:
    """launch_hoist_mac in hoist.hip: "lds" is hoist_mac_lds_kernel, "plain" is hoist_mac_kernel<lt> (the
    linear transform has no LDS form)."""
    if not lt and 0 < guse <= HO_GMAX and (L * n) % HO_LS == 0:
        return "lds"
    return "plain"


def launch_items(chunk: int, B: int, S: int, lt: bool, L: int, n: int, R: int) -> int:
    """C of hoist_core (context.hip): the items of one launch.  S is the context's count of 31-bit primes, 0
    on the limb-wise path.  The chunk is clipped to B BEFORE the 31-bit path scales it by 2 / (S + 2 lt), so
    with S >= 3 (every eligible parameter set: the bound holds n q_max) one launch never holds a whole batch
    of more than one item, whatever the chunk: a launch of m items needs B >= ceil(m (S + 2 lt) / 2)."""
    C = min(chunk, B)
    if S > 0:
        C = max(1, C * 2 // (S + (2 if lt else 0)))
    nblk = (L * n + 255) // 256
    return max(1, min(C, (1 << 30) // (nblk * R)))


class Case(NamedTuple):
    params: Callable[[], object]
    B: int
    chunk: int
    elements: Callable[[int], list]      # n -> the Galois elements
    num_keys: int | None                 # keys per element handed to the set (None: every gadget digit)
    ks32: bool                           # the context takes the 31-bit key switch
    shape: object                        # (CLB, NW) on the 31-bit path, "lds" / "plain" on the limb-wise one
    lt: bool = False                     # also run bfv_linear_transform
    chunk1: bool = False                 # also compare with the same call at set_chunk(1)
    launch: int = 0                      # items the first launch of the rotations must hold (0: not asserted)


def _bfv(n, moduli, base=0, plain=65537):
    return lambda: P.BfvParamsBuilder().ring_degree(n).plain_modulus(plain).ct_moduli(moduli).gadget_base(base).build()


def _hps(n):
    u = P.u64_dbfv().bfv_params
    return lambda: (P.BfvParamsBuilder().ring_degree(n).plain_modulus(u.plain_modulus).ct_moduli(u.ct_basis.moduli)
                    .aux_moduli(u.aux_basis.moduli).gadget_base(u.gadget_base).build())


def _three(n):
    return [3, 1, 2 * n - 1]


def _nine(n):
    """The identity first, in the middle (as 2n + 1) and last, and element 3 twice."""
    return [1, 3, 5, 3, 2 * n + 1, 2 * n - 1, 7, 9, 1]


Q2 = P.Q3[:2]

# (CLB, NW) pairs of mac_block_shape that no context reaches, with the reason.
UNREACHABLE = {
    (2, 4): "CL = 2 is one ciphertext prime, and a one-prime context multiplies on the HPS or the schoolbook "
            "path (exacto_ctx_create's dispatcher), never exact RNS: setup_ks32 builds no 31-bit basis for it",
}

CASES = {
    # ---- 31-bit path, n = 1024 (setup_ks32's smallest ring): one case per reachable (CLB, NW)
    "k32_6x4_run": Case(_bfv(1024, P.Q3), 3, 2, _three, None, True, (6, 4)),           # G = 12 = RUN
    "k32_6x4_run_keys": Case(_bfv(1024, P.Q3, 128), 3, 2, _three, RUN, True, (6, 4)),   # G = 26, 12 keys
    "k32_6x4_run_plus1": Case(_bfv(1024, P.Q3, 128), 3, 2, _three, RUN + 1, True, (6, 4)),
    "k32_6x8_two_runs_plus1": Case(_bfv(1024, P.Q3, 128), 3, 2, _three, 2 * RUN + 1, True, (6, 8)),
    "k32_6x8": Case(_bfv(1024, P.Q3, 256), 3, 2, _three, None, True, (6, 8)),           # G = 23
    "k32_3x8": Case(_bfv(1024, P.Q3, 8), 3, 2, _three, None, True, (3, 8)),             # G = 60
    "k32_8x4": Case(_bfv(1024, P.Q4), 3, 2, _three, None, True, (8, 4)),                # G = 15
    "k32_8x8": Case(_bfv(1024, P.Q4, 256), 3, 2, _three, None, True, (8, 8)),           # G = 30
    "k32_4x8_four_limbs": Case(_bfv(1024, P.Q4, 16), 3, 2, _three, None, True, (4, 8)),  # G = 60
    "k32_4x4": Case(_bfv(1024, Q2), 3, 2, _three, None, True, (4, 4)),                  # G = 8
    "k32_4x8_two_limbs": Case(_bfv(1024, Q2, 8), 3, 2, _three, None, True, (4, 8)),     # G = 40
    # ---- 31-bit path: 2 IG + 5 items in one launch (three item groups, the last clipped to five).  With S = 3
    # that launch is the first of two (launch_items): B = ceil(3 (2 IG + 5) / 2).
    "k32_items_4waves": Case(_bfv(1024, P.Q3), 56, 64, _three, None, True, (6, 4), lt=True, chunk1=True, launch=37),
    "k32_items_8waves": Case(_bfv(1024, P.Q3, 256), 104, 128, _three, 22, True, (6, 8), chunk1=True, launch=69),
    # three launches of 3, 3 and 1 items over two lanes (the linear transform: 2, 2, 2, 1)
    "k32_lanes": Case(_bfv(1024, P.Q3), 7, 5, _three, None, True, (6, 4), lt=True, launch=3),
    "k32_nine": Case(_bfv(1024, P.Q3), 3, 2, _nine, None, True, (6, 4), lt=True),
    # ---- limb-wise path
    # a second item group clipped to 6 items, waves 2 and 3 on a second pass
    "lw_items": Case(_bfv(64, P.Q3), 70, 128, _three, None, False, "lds", lt=True, chunk1=True, launch=70),
    "lw_n16_four_limbs": Case(_bfv(16, P.Q4), 3, 4, _three, None, False, "lds"),        # one LDS block, four limbs
    "lw_n32_two_limbs": Case(_bfv(32, Q2), 3, 4, _three, None, False, "lds"),
    # G = 60 > HO_GMAX, L n = 768: three blocks per (item, rotation) of the plain kernel
    "lw_plain_blocks": Case(_bfv(256, P.Q3, 8), 5, 8, _three, None, False, "plain", launch=5),
    "lw_keys_1": Case(_bfv(64, P.Q3, 32), 3, 4, _three, 1, False, "lds"),               # G = 36
    "lw_keys_4": Case(_bfv(64, P.Q3, 32), 3, 4, _three, 4, False, "lds"),
    "lw_keys_5": Case(_bfv(64, P.Q3, 32), 3, 4, _three, 5, False, "lds"),
    "lw_keys_32": Case(_bfv(64, P.Q3, 32), 3, 4, _three, 32, False, "lds"),
    "lw_keys_33": Case(_bfv(64, P.Q3, 32), 3, 4, _three, 33, False, "plain"),
    # hoist_mac_kernel<true> with five items in one launch and three blocks per item
    "lw_lt_blocks": Case(_bfv(256, P.Q3), 5, 8, _three, None, False, "lds", lt=True, launch=5),
    "lw_hps": Case(_hps(64), 3, 4, _three, None, False, "lds"),                          # one limb, two aux primes
}


def guse_of(name: str, prm=None) -> int:
    c = CASES[name]
    prm = prm or c.params()
    return prm.gadget_digits if c.num_keys is None else min(prm.gadget_digits, c.num_keys)


def make_inputs(name: str):
    """(params, elements, ct [B][2][L][n], gks [R][num_keys][2][L][n], pts [R][n]): uniform residues, with item 0
    every residue q_l - 1, item 1 a zero c1 under a uniform c0 (zero digits: its rotations are the permuted c0
    alone), and, from four items on, a last item that is zero altogether."""
    c = CASES[name]
    prm = c.params()
    n, q = prm.ring_degree, prm.ct_basis.moduli
    elements = c.elements(n)
    rng = np.random.default_rng(sum(map(ord, name)))
    ct = uniform_residues(rng, (c.B, 2), q, n)
    ct[0] = (np.array(q, dtype=np.uint64) - np.uint64(1))[None, :, None]
    ct[1, 1] = 0
    if c.B >= 4:
        ct[-1] = 0
    gks = uniform_residues(rng, (len(elements), guse_of(name, prm), 2), q, n)
    pts = rng.integers(0, prm.plain_modulus, size=(len(elements), n), dtype=np.uint64)
    pts[0, :3] = [2**64 - 1, prm.plain_modulus, 2**63]      # any u64, lifted as bfv_plain_mul lifts it
    return prm, elements, ct, gks, pts


@functools.lru_cache(maxsize=None)
def case_data(name: str):
    """make_inputs and hoist_ref's rotations (and, for lt cases, its linear transform), computed once and
    shared read-only."""
    import hoist_ref
    prm, elements, ct, gks, pts = make_inputs(name)
    want = hoist_ref.rotate_hoisted(prm, ct, elements, gks, threads=4)
    want_lt = hoist_ref.linear_transform(prm, want, pts, threads=4) if CASES[name].lt else None
    for a in (ct, gks, pts, want, want_lt):
        if a is not None:
            a.setflags(write=False)
    return prm, elements, ct, gks, pts, want, want_lt

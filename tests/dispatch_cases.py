"""The multiply path's kernel choices as a table of cases (test helper, CPU only).

Every kernel on the multiply path is chosen by the ring degree n, the class of the RNS primes by how far
they sit below 2^60 (d = 2^60 - q) and the path (exact or HPS).  The thresholds, as csrc/context.hip and
csrc/ntt.hip compare them (q is never equal to a threshold: a threshold is 0 mod 2n, a usable prime 1):

  w32  q > 2^60 - 2^32   run_ntt, run_ntt_fwd2, run_drop_prime: the pinned hand-scheduled NTT rounds at
                         n = 4096 / 8192 (with q < 2^60)
  w24  q > 2^60 - 2^24   setup_ks32, CrtTables.special, tensor_asm, exacto_rns_mul_inv_dev,
                         exacto_rns_polymul_dev, the two psum decisions: special-prime tensor and scale,
                         fused products, the 31-bit key switch
  p60  q < 2^60          lazy kernels; at and above 2^60 the non-lazy ones
  g56  q < 2^56          gen_qb<12>(): the generated generic rounds with fewer reductions at n = 4096
  g50  q < 2^50          gen_qb<10>(): the same at n = 1024

Classes: "special" d < 2^24, "C" 2^24 < d < 2^32, "generic" q < 2^60 - 2^32, "big" q >= 2^60.

`EDGE` pins the primes == 1 mod 32768 nearest to each threshold on either side (usable at every
n <= 16384), as `edge_primes` must find them; `CASES` names the parameter sets the GPU matrix
(tests/test_gpu_dispatch_matrix.py) runs, each with the selection it is expected to take, written out by
hand; `select` restates the library's conditions and tests/test_dispatch_cases.py holds the two together.
"""

from __future__ import annotations

import math
from collections import namedtuple

from test_fpc_crt import aux_basis, is_prime

T60 = 1 << 60
STEP = 32768
THRESHOLDS = {"w32": T60 - (1 << 32), "w24": T60 - (1 << 24), "p60": T60, "g56": 1 << 56, "g50": 1 << 50}

PATH_EXACT_RNS, PATH_HPS, PATH_SCHOOLBOOK = 0, 1, 2    # exacto_amd._ffi


def edge_primes(step: int, threshold: int, side: str, count: int) -> list[int]:
    """The `count` primes == 1 mod step nearest to `threshold`, nearest first: side "below" the largest
    ones < threshold, side "above" the smallest ones > threshold."""
    assert side in ("below", "above") and step > 1 and count >= 0
    cand = threshold // step * step + 1
    out = []
    if side == "below":
        while cand >= threshold:
            cand -= step
        while len(out) < count and cand > 1:
            if is_prime(cand):
                out.append(cand)
            cand -= step
    else:
        while cand <= threshold:
            cand += step
        while len(out) < count:
            if is_prime(cand):
                out.append(cand)
            cand += step
    assert len(out) == count, (step, threshold, side, out)
    return out


# edge_primes(STEP, THRESHOLDS[name], side, 3), pinned
EDGE = {
    "w32": {"below": [1152921500311781377, 1152921500311060481, 1152921500309323777],     # generic
            "above": [1152921500312764417, 1152921500313518081, 1152921500313911297]},    # class C
    "w24": {"below": [1152921504589938689, 1152921504588070913, 1152921504587612161],     # class C
            "above": [1152921504591020033, 1152921504591216641, 1152921504592429057]},    # special
    "p60": {"below": [1152921504606748673, 1152921504606683137, 1152921504606584833],     # special
            "above": [1152921504607338497, 1152921504608747521, 1152921504609239041]},    # big
    "g56": {"below": [72057594037370881, 72057594037338113, 72057594036879361],
            "above": [72057594038321153, 72057594038747137, 72057594039205889]},
    "g50": {"below": [1125899904679937, 1125899903991809, 1125899903827969],
            "above": [1125899908022273, 1125899908612097, 1125899909038081]},
}

TOP3 = EDGE["p60"]["below"]            # the three top special primes == 1 mod 32768
BIG62 = 4611686018427322369            # a 62-bit prime == 1 mod 32768 (tests/test_gpu_ntt.py)
C_TOP = EDGE["w24"]["below"]           # class C, d just above 2^24
C_LOW = EDGE["w32"]["above"]           # class C, d just below 2^32
CLASS_C4 = C_LOW[:2] + C_TOP[:2]       # the standalone transforms' primes

COMPACT_Q, COMPACT_AUX = 1099509805057, 562949953443841             # compact_bfv (oracle/params.py)
U64_Q, U64_AUX = 1152921504606830593, [18014398509998081, 36028797018972161]   # u64_dbfv


def prime_class(q: int) -> str:
    if q >= T60:
        return "big"
    if q > THRESHOLDS["w24"]:
        return "special"
    if q > THRESHOLDS["w32"]:
        return "C"
    return "generic"


# What a case is expected to select.
#   path         ctx.path
#   fwd_pinned   the forward NTTs over the ciphertext primes are ntt_fwd_pin_kernel
#   tensor_asm   the tensor is the asm one (tensor_pin_kernel at n = 8192, ntt_inv_tensor_kernel<12, true, true..>)
#   ks32         ctx.ks32_primes > 0
#   scale_sp     the exact scale is exact_scale_sp_kernel (CrtTables.special with K = L + 1)
#   fwd_qb       QB of ntt_fwd_gen_kernel<LOGN, QB> over the ciphertext primes (None: not that kernel)
#   tensor_qb    QB of the generated generic tensor ntt_inv_tensor_kernel<LOGN, true, false, 0, true, QB..>
Expect = namedtuple("Expect", "path fwd_pinned tensor_asm ks32 scale_sp fwd_qb tensor_qb")
Case = namedtuple("Case", "name group n ct aux plain gbase B expect")


def library_primes(n, ct, aux, plain):
    """exacto_ctx_create's prime list: the ciphertext primes, then the caller's auxiliary primes (HPS) or
    the exact path's own (primes == 1 mod 2n below 2^60, largest first, until P > 4 p n Q)."""
    if len(ct) > 1:
        return list(ct) + aux_basis(n, plain, list(ct))
    return list(ct) + list(aux)


def select(n, ct, aux, plain, gbase) -> Expect:
    """The library's conditions restated (context.hip setup_ks32, build_crt_tables, run_ntt, tensor_asm;
    ntt.hip launch_ntt, launch_it, gen_small)."""
    logn = n.bit_length() - 1
    L = len(ct)
    path = PATH_EXACT_RNS if L > 1 else PATH_HPS if aux else PATH_SCHOOLBOOK
    primes = library_primes(n, ct, aux, plain)
    K = len(primes) - L
    base = gbase or (1 << 16)
    in32 = lambda q: THRESHOLDS["w32"] < q < T60
    in24 = lambda q: THRESHOLDS["w24"] < q < T60
    hand = logn in (12, 13)                                    # the hand-scheduled kernels' sizes
    fwd_pinned = hand and all(in32(q) for q in ct)
    tensor_asm = hand and all(in24(q) for q in primes)
    ks32 = (path == PATH_EXACT_RNS and base <= 65536 and 10 <= logn <= 14 and L <= 4 and all(in24(q) for q in ct))
    special = max(primes) < 2 * min(primes) and max(primes) < T60 and min(primes) > THRESHOLDS["w24"]
    scale_sp = path == PATH_EXACT_RNS and special and K == L + 1 and L <= 6
    gen = {10: 50, 12: 56, 13: 60}                             # gen_qb<LOGN>() where the generated rounds exist

    def qb(ps):
        if logn not in gen or max(ps) >= T60:
            return None
        return gen[logn] if gen[logn] < 60 and max(ps).bit_length() <= gen[logn] else 60

    fwd_qb = None if fwd_pinned else qb(ct)
    tensor_qb = None if tensor_asm else qb(primes)
    return Expect(path, fwd_pinned, tensor_asm, ks32, scale_sp, fwd_qb, tensor_qb)


E, H = PATH_EXACT_RNS, PATH_HPS
G16 = 1 << 16

CASES = [
    # ---- a. ring-degree sweep, exact path: the top special primes (no hand-scheduled kernel below n = 4096
    # or at 16384; the 31-bit key switch from n = 1024).  n = 16, 64, 256 complete logn = 4 .. 14.
    Case("sweep_exact_n16", "sweep_exact", 16, TOP3, [], 65537, G16, 2, Expect(E, False, False, False, True, None, None)),
    Case("sweep_exact_n32", "sweep_exact", 32, TOP3, [], 65537, G16, 2, Expect(E, False, False, False, True, None, None)),
    Case("sweep_exact_n64", "sweep_exact", 64, TOP3, [], 65537, G16, 2, Expect(E, False, False, False, True, None, None)),
    Case("sweep_exact_n128", "sweep_exact", 128, TOP3, [], 65537, G16, 2, Expect(E, False, False, False, True, None, None)),
    Case("sweep_exact_n256", "sweep_exact", 256, TOP3, [], 65537, G16, 2, Expect(E, False, False, False, True, None, None)),
    Case("sweep_exact_n512", "sweep_exact", 512, TOP3, [], 65537, G16, 2, Expect(E, False, False, False, True, None, None)),
    Case("sweep_exact_n2048", "sweep_exact", 2048, TOP3, [], 65537, G16, 2, Expect(E, False, False, True, True, None, None)),
    Case("sweep_exact_n16384", "sweep_exact", 16384, TOP3[:2], [], 65537, G16, 1, Expect(E, False, False, True, True, None, None)),
    # ---- b. ring-degree sweep, HPS: one auxiliary prime (compact_bfv's pair; at n = 2048 its auxiliary prime
    # is neither 1 mod 4096 nor above the centring bound n q / 2, so u64_dbfv's 2^55 prime stands in), two
    # (u64_dbfv's)
    Case("sweep_hps1_n128", "sweep_hps", 128, [COMPACT_Q], [COMPACT_AUX], 257, G16, 2, Expect(H, False, False, False, False, None, None)),
    Case("sweep_hps1_n512", "sweep_hps", 512, [COMPACT_Q], [COMPACT_AUX], 257, G16, 2, Expect(H, False, False, False, False, None, None)),
    Case("sweep_hps1_n2048", "sweep_hps", 2048, [COMPACT_Q], [U64_AUX[1]], 257, G16, 2, Expect(H, False, False, False, False, None, None)),
    Case("sweep_hps2_n512", "sweep_hps", 512, [U64_Q], U64_AUX, 1040407, 256, 2, Expect(H, False, False, False, False, None, None)),
    Case("sweep_hps2_n2048", "sweep_hps", 2048, [U64_Q], U64_AUX, 1040407, 256, 2, Expect(H, False, False, False, False, None, None)),
    # ---- c. class C where it changes kernels: the pinned forward NTT with the generated generic tensor, the
    # generic scale and the limb-wise key switch
    Case("classC_L2_n4096", "classC", 4096, [C_LOW[0], C_TOP[0]], [], 65537, G16, 2, Expect(E, True, False, False, False, None, 60)),
    Case("classC_L2_n8192", "classC", 8192, [C_LOW[0], C_TOP[0]], [], 65537, G16, 2, Expect(E, True, False, False, False, None, 60)),
    Case("mixed_L3_n4096", "classC", 4096, TOP3[:2] + [C_LOW[0]], [], 65537, G16, 2, Expect(E, True, False, False, False, None, 60)),
    Case("mixed_L3_n8192", "classC", 8192, TOP3[:2] + [C_LOW[0]], [], 65537, G16, 2, Expect(E, True, False, False, False, None, 60)),
    Case("classC_L3_n4096", "classC", 4096, C_LOW[:2] + [C_TOP[0]], [], 65537, G16, 2, Expect(E, True, False, False, False, None, 60)),
    Case("classC_L3_n8192", "classC", 8192, C_LOW[:2] + [C_TOP[0]], [], 65537, G16, 2, Expect(E, True, False, False, False, None, 60)),
    # ---- d. the neighbours of each threshold: the two nearest primes on either side (n = 4096, L = 2); the
    # gen_qb boundaries on the HPS path, one ciphertext prime and two auxiliary primes of the same side
    # (a single auxiliary prime of q's size fails the centring bound P > n q / 2)
    Case("w32_below_n4096", "edge", 4096, EDGE["w32"]["below"][:2], [], 65537, G16, 2, Expect(E, False, False, False, False, 60, 60)),
    Case("w32_above_n4096", "edge", 4096, EDGE["w32"]["above"][:2], [], 65537, G16, 2, Expect(E, True, False, False, False, None, 60)),
    Case("w24_below_n4096", "edge", 4096, EDGE["w24"]["below"][:2], [], 65537, G16, 2, Expect(E, True, False, False, False, None, 60)),
    Case("w24_above_n4096", "edge", 4096, EDGE["w24"]["above"][:2], [], 65537, G16, 2, Expect(E, True, True, True, True, None, None)),
    Case("p60_below_n4096", "edge", 4096, EDGE["p60"]["below"][:2], [], 65537, G16, 2, Expect(E, True, True, True, True, None, None)),
    Case("p60_above_n4096", "edge", 4096, EDGE["p60"]["above"][:2], [], 65537, G16, 2, Expect(E, False, False, False, False, None, None)),
    Case("g50_below_n1024", "edge", 1024, EDGE["g50"]["below"][:1], EDGE["g50"]["below"][1:], 65537, G16, 2, Expect(H, False, False, False, False, 50, 50)),
    Case("g50_above_n1024", "edge", 1024, EDGE["g50"]["above"][:1], EDGE["g50"]["above"][1:], 65537, G16, 2, Expect(H, False, False, False, False, 60, 60)),
    Case("g56_below_n4096", "edge", 4096, EDGE["g56"]["below"][:1], EDGE["g56"]["below"][1:], 65537, G16, 2, Expect(H, False, False, False, False, 56, 56)),
    Case("g56_above_n4096", "edge", 4096, EDGE["g56"]["above"][:1], EDGE["g56"]["above"][1:], 65537, G16, 2, Expect(H, False, False, False, False, 60, 60)),
    # ---- e. primes >= 2^60 at full size: the non-lazy kernels
    Case("big_L2_n4096", "big", 4096, [BIG62, EDGE["p60"]["above"][0]], [], 65537, G16, 1, Expect(E, False, False, False, False, None, None)),
]

BY_NAME = {c.name: c for c in CASES}
PROFILED_GROUPS = ("classC", "edge", "big")     # the cases whose kernels the GPU test reads back

# the dBFV product of group c: cfg4's digits over the mixed basis
DBFV_MIXED = dict(n=4096, ct=TOP3[:2] + [C_LOW[0]], plain=260111, gbase=G16, d=2, base=256, dplain=65536, B=2)

# mod-switch bases of group c (the dropped prime is the last): every prime of both lies in the 2^32 window,
# so the drop runs the hand-scheduled kernel (ntt_dropprime_asm_kernel) at n = 4096 / 8192
MODSWITCH_BASES = {"mixed_L3": TOP3[:2] + [C_LOW[0]], "classC_L2": [C_LOW[0], C_TOP[0]]}


def params_of(case):
    from oracle.params import BfvParamsBuilder
    return (BfvParamsBuilder().ring_degree(case.n).plain_modulus(case.plain).ct_moduli(case.ct)
            .aux_moduli(case.aux).gadget_base(case.gbase).build())


# ------------------------------------------------------------------ DESIGN.md's dispatch matrix

def _ntt_cell(e: Expect, logn: int, cls: str) -> str:
    if e.fwd_pinned:
        return "`ntt_fwd_pin_kernel`"
    if e.fwd_qb is not None:
        return f"`ntt_fwd_gen_kernel<{logn}, {e.fwd_qb}>`"
    return "`ntt_fwd_kernel`, " + ("non-lazy" if cls == "big" else "lazy")


def _tensor_cell(e: Expect, logn: int, cls: str) -> str:
    if e.tensor_asm:
        return "asm (`tensor_pin` at 8192)"
    if e.tensor_qb is not None:
        return f"generated, QB = {e.tensor_qb}"
    return "C++, " + ("non-lazy" if cls == "big" else "lazy")


def design_table() -> str:
    """The dispatch matrix of DESIGN.md §4, one row per (logn, prime class, path) that a case covers."""
    rows = {}
    for c in CASES:
        logn = c.n.bit_length() - 1
        order = ["generic", "C", "special", "big"]
        cls = min((prime_class(q) for q in c.ct), key=order.index) if max(c.ct) < T60 else "big"
        e = c.expect
        path = "exact" if e.path == PATH_EXACT_RNS else "HPS"
        scale = "`hps_scale_kernel`" if e.path == PATH_HPS else "`exact_scale_sp_kernel`" if e.scale_sp else "`exact_scale_kernel`"
        ks = "31-bit basis (`ks32_*`)" if e.ks32 else "limb-wise `relin_mac`"
        key = (logn, cls, path, _ntt_cell(e, logn, cls), _tensor_cell(e, logn, cls), scale, ks)
        rows.setdefault(key, []).append(c.name)
    lines = ["| logn | primes | path | forward NTT (ct primes) | tensor | scale | key switch | cases |",
             "|---|---|---|---|---|---|---|---|"]
    for key in sorted(rows, key=lambda k: (k[0], k[2], k[1])):
        lines.append("| " + " | ".join(str(x) for x in key) + " | " + ", ".join(f"`{n}`" for n in rows[key]) + " |")
    return "\n".join(lines)


if __name__ == "__main__":
    print(design_table())

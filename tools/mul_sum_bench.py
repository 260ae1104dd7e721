#!/usr/bin/env python3
"""Standalone benchmark of exacto_bfv_mul_sum_dev (dot products of ciphertext vectors, one key switch per
sum) against the best composition a caller has without it, in the same process on the same GPU:

  composition : ONE exacto_bfv_mul_and_relin_dev over the B*K pairs gathered contiguously (term-major,
                [K][B], so that each later pass is contiguous too), then K - 1 exacto_bfv_add_dev passes.

Shapes: the cfg3 parameters (n = 4096, 3 x 60-bit, base 2^16) with dot products of length K = 2, 8, 32 and
B*K = 1024 products (the product count of the cfg3 bench batch), and the cfg5 parameters (n = 8192,
4 x 60-bit, base 256) with K = 8, B = 8.

HIP events on the library's stream.  One warm-up call of each (then two more untimed of each, so
that buffers and clocks have settled), then --windows timed windows of --reps calls each, the two
alternating, so both see the same machine state; the spread of the composition's windows is the noise
a difference has to exceed.  Then one profiled call (exacto_prof_enable: one lane,
HIP events around every launch) for the per-kernel split, group_max / last_mode, and the achieved bytes/s
of the group-sum kernel next to the exact lift's in the same run.  One JSON line per shape.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from exacto_amd._ffi import HipContext  # noqa: E402

Q4 = [1152921504606830593, 1152921504606748673, 1152921504606683137, 1152921504606601217]
SHAPES = {
    "cfg3_k2": dict(n=4096, q=Q4[:3], t=65537, gbase=0, B=512, K=2),
    "cfg3_k8": dict(n=4096, q=Q4[:3], t=65537, gbase=0, B=128, K=8),
    "cfg3_k32": dict(n=4096, q=Q4[:3], t=65537, gbase=0, B=32, K=32),
    "cfg5_k8": dict(n=8192, q=Q4, t=1040407, gbase=256, B=8, K=8),
}
# profiled kernel families (runtime.hpp ProfKind)
KINDS = {0: "fwd_ntt", 1: "inv_ntt", 2: "tensor", 4: "lift", 5: "scale", 6: "ks_digits", 7: "ks_mac", 8: "ks_crt",
         9: "pairsum", 10: "psum_scale", 12: "digit_sum", 13: "combine", 17: "group_sum"}

ap = argparse.ArgumentParser()
ap.add_argument("--shape", choices=list(SHAPES) + ["all"], default="all")
ap.add_argument("--reps", type=int, default=50, help="calls per timed window")
ap.add_argument("--windows", type=int, default=7, help="timed windows per variant (alternating)")
ap.add_argument("--group", type=int, default=0, help="exacto_ctx_set_mul_sum_group (0: the context's own limit)")
args = ap.parse_args()

dev = torch.device("cuda", 0)
s = torch.cuda.current_stream()


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(reps):
        fn()
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def stats(v):
    v = sorted(v)
    return {"min": round(v[0], 4), "median": round(v[len(v) // 2], 4), "max": round(v[-1], 4)}


def run(name, sh):
    n, q, B, K = sh["n"], sh["q"], sh["B"], sh["K"]
    L = len(q)
    ctx = HipContext(n, q, plain_modulus=sh["t"], gadget_base=sh["gbase"])
    ctx.set_stream(s.cuda_stream)
    ctx.set_mul_sum_group(args.group)
    g = torch.Generator(device=dev)
    g.manual_seed(11)

    def uniform(*prefix):
        return torch.stack([torch.randint(0, qi, (*prefix, 2, n), generator=g, dtype=torch.int64, device=dev)
                            for qi in q], dim=len(prefix) + 1).contiguous()       # [..][2][L][n]
    a, b = uniform(B, K), uniform(B, K)
    rlk = uniform(ctx.G)
    torch.cuda.synchronize()
    ctx.load_relin_key_dev(rlk, ctx.G)
    terms = [(k, k, 0) for k in range(K)]
    out = torch.zeros((B, 1, 2, L, n), dtype=torch.int64, device=dev)

    def mul_sum():
        ctx.bfv_mul_sum_dev(a, K, b, K, terms, 1, out, B)

    # the composition's inputs gathered term-major once, outside the timed windows
    ak, bk = a.permute(1, 0, 2, 3, 4).contiguous(), b.permute(1, 0, 2, 3, 4).contiguous()   # [K][B][2][L][n]
    prod = torch.zeros((K, B, 2, L, n), dtype=torch.int64, device=dev)
    acc = torch.zeros((B, 2, L, n), dtype=torch.int64, device=dev)

    def composed():
        ctx.bfv_mul_and_relin_dev(ak, bk, prod, K * B)
        ctx.bfv_add_dev(prod[0], 2, prod[1], 2, acc, B)
        for k in range(2, K):
            ctx.bfv_add_dev(acc, 2, prod[k], 2, acc, B)

    mul_sum()
    composed()
    torch.cuda.synchronize()
    same = bool(torch.equal(out[:, 0], acc))
    for _ in range(2):
        composed()
        mul_sum()
    t_sum, t_comp = [], []
    for _ in range(args.windows):
        t_comp.append(window(composed, args.reps))
        t_sum.append(window(mul_sum, args.reps))
    st_sum, st_comp = stats(t_sum), stats(t_comp)
    spread = (st_comp["max"] - st_comp["min"]) / st_comp["median"]

    # one profiled call (its own pass: profiling keeps one lane and one stream)
    ctx.prof_enable(True)
    mul_sum()
    ctx.synchronize()
    split = {}
    for kind, label in KINDS.items():
        r = ctx.prof_read(kind)
        if r["launches"]:
            split[label] = {"launches": r["launches"], "ms": round(r["ms"], 4),
                            "TBs": round(r["bytes"] / (r["ms"] * 1e-3) / 1e12, 3) if r["ms"] > 0 else None}
    ctx.prof_enable(False)
    info = ctx.mul_sum_info()
    print(json.dumps({
        "shape": name, "n": n, "L": L, "B": B, "K": K, "products": B * K,
        "mul_sum_ms": st_sum, "composition_ms": st_comp, "composition_spread": round(spread, 4),
        "ratio_composition_over_mul_sum": round(st_comp["median"] / st_sum["median"], 3),
        "faster_by_more_than_spread": bool(st_sum["median"] < st_comp["median"] * (1 - spread)),
        "equal": same, "group_max": info["group_max"], "last_mode": info["last_mode"],
        "groups_per_output": -(-K // info["group_max"]),
        "profiled_split": split,
        "group_sum_TBs": split.get("group_sum", {}).get("TBs"), "lift_TBs": split.get("lift", {}).get("TBs"),
    }), flush=True)
    ctx.close()


for name in (SHAPES if args.shape == "all" else [args.shape]):
    run(name, SHAPES[name])

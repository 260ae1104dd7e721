#!/usr/bin/env python3
"""Standalone benchmark of exacto_bfv_mod_switch_dev (one drop, exact mode) against a stand-in built from
entry points the library had before it, moving the rows an unfused version would, in the same process on
the same GPU:

  stand-in : exacto_ntt_inv_dev on the last limb's rows, then on the L - 1 remaining limbs (a context
             over moduli[:-1]) exacto_rns_fwd_dev, exacto_rns_sub_dev and exacto_rns_scalar_mul_dev.
             It omits the centring, the re-reduction of delta per prime and its replication into L - 1
             rows, so it under-counts what an unfused version costs.

Shapes: cfg3 (n = 4096, L = 3, polys 2, B = 1024) and cfg5's basis (n = 8192, L = 4, polys 2, B = 256).

HIP events on the library's stream.  One warm-up call of each (then two more untimed of each), then
--windows timed windows of --reps calls each, the two alternating, so both see the same machine state; the
spread of the stand-in's windows is the noise a difference has to exceed.  Then one profiled call
(exacto_prof_enable) for the kernel that ran and its achieved bytes/s against the algorithmic
(2 L - 1) 8 n bytes per polynomial.  One JSON line per shape.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from exacto_amd._ffi import HipContext  # noqa: E402

Q4 = [1152921504606830593, 1152921504606748673, 1152921504606683137, 1152921504606601217]
SHAPES = {
    "cfg3": dict(n=4096, q=Q4[:3], t=65537, polys=2, B=1024),
    "cfg5": dict(n=8192, q=Q4, t=1040407, polys=2, B=256),
}
PK_MODSWITCH = 18   # runtime.hpp ProfKind

ap = argparse.ArgumentParser()
ap.add_argument("--shape", choices=list(SHAPES) + ["all"], default="all")
ap.add_argument("--reps", type=int, default=50, help="calls per timed window")
ap.add_argument("--windows", type=int, default=7, help="timed windows per variant (alternating)")
ap.add_argument("--mode", choices=["round", "reference"], default="round")
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
    n, q, B, polys = sh["n"], sh["q"], sh["B"], sh["polys"]
    L = len(q)
    rows = B * polys
    ctx = HipContext(n, q, plain_modulus=sh["t"])
    lo = HipContext(n, q[:-1], plain_modulus=sh["t"])
    ctx.set_stream(s.cuda_stream)
    lo.set_stream(s.cuda_stream)
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    ct = torch.stack([torch.randint(0, qi, (B, polys, n), generator=g, dtype=torch.int64, device=dev) for qi in q],
                     dim=2).contiguous()                                   # [B][polys][L][n]
    out = torch.zeros((B, polys, L - 1, n), dtype=torch.int64, device=dev)

    def fused():
        ctx.bfv_mod_switch_dev(ct, polys, L, L - 1, out, B, mode=args.mode)

    # the stand-in's rows, laid out once outside the timed windows
    last = ct[:, :, L - 1].reshape(rows, n).contiguous()
    c_lo = ct[:, :, :L - 1].reshape(rows, L - 1, n).contiguous()
    delta = c_lo.clone()
    tmp, out2 = torch.zeros_like(c_lo), torch.zeros_like(c_lo)
    scalar = pow(q[-1], -1, q[0])

    def standin():
        ctx.ntt_inv_dev(last, rows, limb=L - 1)
        lo.rns_fwd_dev(delta, rows)
        lo.rns_sub_dev(c_lo, delta, tmp, rows)
        lo.rns_scalar_mul_dev(tmp, scalar, out2, rows)

    fused()
    standin()
    torch.cuda.synchronize()
    for _ in range(2):
        standin()
        fused()
    t_f, t_s = [], []
    for _ in range(args.windows):
        t_s.append(window(standin, args.reps))
        t_f.append(window(fused, args.reps))
    st_f, st_s = stats(t_f), stats(t_s)
    spread = (st_s["max"] - st_s["min"]) / st_s["median"]
    alg_bytes = (2 * L - 1) * 8 * n * rows

    ctx.prof_enable(True)
    fused()
    ctx.synchronize()
    r = ctx.prof_read(PK_MODSWITCH)
    kernels = ctx.prof_kernels(PK_MODSWITCH)
    ctx.prof_enable(False)
    print(json.dumps({
        "shape": name, "n": n, "L": L, "B": B, "polys": polys, "mode": args.mode,
        "fused_ms": st_f, "standin_ms": st_s, "standin_spread": round(spread, 4),
        "ratio_standin_over_fused": round(st_s["median"] / st_f["median"], 3),
        "faster_by_more_than_spread": bool(st_f["median"] < st_s["median"] * (1 - spread)),
        "algorithmic_bytes": alg_bytes,
        "fused_TBs": round(alg_bytes / (st_f["median"] * 1e-3) / 1e12, 3),
        "profiled": {"launches": r["launches"], "ms": round(r["ms"], 4),
                     "TBs": round(r["bytes"] / (r["ms"] * 1e-3) / 1e12, 3) if r["ms"] > 0 else None,
                     "kernels": [k[0] for k in kernels]},
    }), flush=True)
    ctx.close()
    lo.close()


for name in (SHAPES if args.shape == "all" else [args.shape]):
    run(name, SHAPES[name])

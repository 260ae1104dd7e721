#!/usr/bin/env python3
"""Standalone benchmark of exacto_batch_encode_dev / exacto_batch_decode_dev (the 32-bit slot transforms mod
the plaintext prime t, batch.hip) against a stand-in built from entry points the library had before them,
in the same process on the same GPU and the same [B][n] buffer:

  stand-in : exacto_ntt_inv_dev (for encode) / exacto_ntt_fwd_dev (for decode) on a second context created
             with ct_moduli = [t]: the 64-bit transform mod the same prime.  It omits the slot permutation
             (a second pass over the buffer, or a strided gather), so it under-counts a two-pass version.

Shapes: t = 65537 at n = 4096 (B = 4096) and n = 8192 (B = 2048), and the 31-bit t = 2147377153 at n = 4096
(128 MiB buffers: resident in the 256 MiB Infinity Cache), and t = 65537 and the 32-bit t = 4294828033 at
n = 4096 with B = 32768 (1 GiB: from HBM).

HIP events on the library's stream.  One warm-up call of each (then two more untimed of each), then
--windows timed windows of --reps calls each, the two alternating, so both see the same machine state; the
spread of the stand-in's windows is the noise a difference has to exceed.  TB/s counts the algorithmic
16 n bytes per polynomial (8 n read, 8 n written) over the median time.  One JSON line per shape and direction.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from exacto_amd._ffi import HipContext  # noqa: E402

Q3 = [1152921504606830593, 1152921504606748673, 1152921504606683137]
SHAPES = {
    "t17_n4096": dict(n=4096, t=65537, B=4096),
    "t17_n8192": dict(n=8192, t=65537, B=2048),
    "t31_n4096": dict(n=4096, t=2147377153, B=4096),
    # the three shapes above are 128 MiB buffers, which stay resident in the 256 MiB Infinity Cache between
    # the in-place calls: their TB/s is not an HBM rate.  This one (1 GiB) streams from HBM.
    "t17_n4096_hbm": dict(n=4096, t=65537, B=32768),
    # the strict arithmetic (2^31 <= t < 2^32: 64-bit carries), from HBM as well
    "t32_n4096_hbm": dict(n=4096, t=4294828033, B=32768),
}

ap = argparse.ArgumentParser()
ap.add_argument("--shape", choices=list(SHAPES) + ["all"], default="all")
ap.add_argument("--reps", type=int, default=20, help="calls per timed window")
ap.add_argument("--windows", type=int, default=7, help="timed windows per variant (alternating)")
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
    n, t, B = sh["n"], sh["t"], sh["B"]
    ctx = HipContext(n, Q3, plain_modulus=t)
    wide = HipContext(n, [t], plain_modulus=257)          # the plaintext prime as a 64-bit transform's prime
    ctx.set_stream(s.cuda_stream)
    wide.set_stream(s.cuda_stream)
    ctx.batch_info()                                       # tables resident before anything is timed
    g = torch.Generator(device=dev)
    g.manual_seed(13)
    buf = torch.randint(0, t, (B, n), generator=g, dtype=torch.int64, device=dev)
    alg_bytes = 16 * n * B
    pairs = {
        "encode": (lambda: ctx.batch_encode_dev(buf, buf, B), lambda: wide.ntt_inv_dev(buf, B)),
        "decode": (lambda: ctx.batch_decode_dev(buf, buf, B), lambda: wide.ntt_fwd_dev(buf, B)),
    }
    for direction, (new, standin) in pairs.items():
        new()
        standin()
        torch.cuda.synchronize()
        for _ in range(2):
            standin()
            new()
        t_n, t_s = [], []
        for _ in range(args.windows):
            t_s.append(window(standin, args.reps))
            t_n.append(window(new, args.reps))
        st_n, st_s = stats(t_n), stats(t_s)
        spread = (st_s["max"] - st_s["min"]) / st_s["median"]
        print(json.dumps({
            "shape": name, "direction": direction, "n": n, "t": t, "B": B,
            "batch_ms": st_n, "standin_ms": st_s, "standin_spread": round(spread, 4),
            "ratio_standin_over_batch": round(st_s["median"] / st_n["median"], 3),
            "faster_by_more_than_spread": bool(st_n["median"] < st_s["median"] * (1 - spread)),
            "algorithmic_bytes": alg_bytes,
            "batch_TBs": round(alg_bytes / (st_n["median"] * 1e-3) / 1e12, 3),
            "standin_TBs": round(alg_bytes / (st_s["median"] * 1e-3) / 1e12, 3),
        }), flush=True)
    ctx.close()
    wide.close()


for name in (SHAPES if args.shape == "all" else [args.shape]):
    run(name, SHAPES[name])

#!/usr/bin/env python3
"""Standalone timing of the noise measurement against decryption on the same buffers, on one GPU:

  cfg3 : exacto_bfv_noise_dev  against exacto_bfv_decrypt_dev,  n = 4096, L = 3, B = 1024, polys = 2;
  cfg5 : exacto_dbfv_noise_dev against the decryption of the same limbs (exacto_bfv_decrypt_dev with batch
         B * d, what exacto_dbfv_decrypt runs before its recomposition), n = 8192, L = 4, B = 128, d = 8.

The two calls share the phase and the inverse NTT; they differ in the last kernel, which reads the same
[items][L][n] phase and writes L words per item (noise_kernel + noise_final_kernel) where decryption writes n
words per item (decrypt_round_kernel).  HIP events on the library's stream, one warm-up call, then --reps
calls, the two alternating --rounds times; prints one JSON line per shape.  The last kernels' own times come
from a kernel trace of this script in a run of its own:
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/noise_bench.py --shape cfg3 --reps 3 --rounds 1
Bytes of the last kernel: the phase once, items * L * n * 8.
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
    "cfg3": dict(n=4096, q=Q4[:3], t=65537, gbase=0, B=1024, d=0),
    "cfg5": dict(n=8192, q=Q4, t=1040407, gbase=256, B=128, d=8),
}
HBM_LINE = 8.0e12   # bytes / s, the MI355X line DESIGN.md measures against
KEY = [1, 2, 3, 4]

ap = argparse.ArgumentParser()
ap.add_argument("--shape", choices=list(SHAPES) + ["all"], default="all")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--batch", type=int, default=0, help="override B (0: the shape's)")
args = ap.parse_args()

dev = torch.device("cuda", 0)
s = torch.cuda.current_stream()


def timed(fn, reps):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(reps):
        fn()
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def run(name, sh):
    n, q, B, d = sh["n"], sh["q"], args.batch or sh["B"], sh["d"]
    L, items = len(q), (args.batch or sh["B"]) * max(sh["d"], 1)
    ctx = HipContext(n, q, plain_modulus=sh["t"], gadget_base=sh["gbase"])
    ctx.set_stream(s.cuda_stream)
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    ct = torch.stack([torch.randint(0, qi, (items, 2, n), generator=g, dtype=torch.int64, device=dev) for qi in q],
                     dim=2).contiguous()                                  # [items][2][L][n]
    sk = torch.from_numpy(ctx.gen_secret_key(KEY, stream=1).view(np.int64)).to(dev)
    plain = torch.zeros((items, n), dtype=torch.int64, device=dev)
    plain2 = torch.zeros_like(plain)
    words = torch.zeros((B, L), dtype=torch.int64, device=dev)
    words_items = torch.zeros((items, L), dtype=torch.int64, device=dev)

    dec = lambda: ctx.bfv_decrypt_dev(ct, 2, sk, plain, items)
    if d:
        noise = lambda: ctx.dbfv_noise_dev(d, ct, sk, words, B)
    else:
        noise = lambda: ctx.bfv_noise_dev(ct, 2, sk, words, B)
    t_dec, t_noise = [], []
    for _ in range(args.rounds):
        t_dec.append(timed(dec, args.reps))
        t_noise.append(timed(noise, args.reps))
    # the by-product equals decryption, and the dBFV form equals the maximum of the per-limb values
    ctx.bfv_noise_dev(ct, 2, sk, words_items, items, plain_out=plain2)
    torch.cuda.synchronize()
    same_plain = bool(torch.equal(plain, plain2))
    w = words_items.cpu().numpy().view(np.uint64)
    per = [sum(int(x) << (64 * k) for k, x in enumerate(row)) for row in w]
    got = [sum(int(x) << (64 * k) for k, x in enumerate(row)) for row in words.cpu().numpy().view(np.uint64)]
    grp = max(d, 1)
    same_max = got == [max(per[i * grp:(i + 1) * grp]) for i in range(B)]
    td, tn = min(t_dec), min(t_noise)
    phase_bytes = items * L * n * 8
    print(json.dumps({
        "shape": name, "n": n, "L": L, "B": B, "d": d, "call": "dbfv_noise_dev" if d else "bfv_noise_dev",
        "decrypt_ms": round(td, 4), "noise_ms": round(tn, 4), "noise_over_decrypt": round(tn / td, 3),
        "decrypt_ms_rounds": [round(x, 4) for x in t_dec], "noise_ms_rounds": [round(x, 4) for x in t_noise],
        "last_kernel_bytes": phase_bytes, "hbm_line_ms_for_those_bytes": round(phase_bytes / HBM_LINE * 1e3, 4),
        "plain_out_equals_decrypt": same_plain, "noise_equals_per_item_max": same_max,
    }), flush=True)
    ctx.close()


for name in (SHAPES if args.shape == "all" else [args.shape]):
    run(name, SHAPES[name])

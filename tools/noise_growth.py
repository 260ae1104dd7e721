#!/usr/bin/env python3
"""measure_growth_factor of the reference's evaluation (src/bin/paper_repro.rs:166-201) on the device, at the
u64_dbfv preset (presets.rs:61-75: n = 4096, one 60-bit prime, t = 1040407, base 256, d = 8, p = 2^64).

The trials run as one batch: random u64 inputs from a fixed seed, dbfv_encrypt_sk -> dbfv_noise of both
inputs -> dbfv_mul -> dbfv_noise, growth = noise_out / max(noise_a, noise_b, 1) per trial; prints the
per-trial values and one JSON line with the mean and the maximum, as the reference's table has them.
--chain: also measure_unsafe_supported_depth's chain (paper_repro.rs:203-236: 5 * 3^k, mul_depth reset before
every step), with the noise and the budget after each step until decryption stops matching.
Keys and encryption noise come from the library's ChaCha streams under --seed; nothing outside the
repository is read.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from exacto_amd._ffi import HipContext, noise_budget_bits  # noqa: E402

U64_DBFV = dict(n=4096, q=[1152921504606830593], aux=[18014398509998081, 36028797018972161], t=1040407,
                gbase=256, base=256, d=8, plain=0)

ap = argparse.ArgumentParser()
ap.add_argument("--trials", type=int, default=8, help="paper_repro.rs:172")
ap.add_argument("--seed", type=int, default=2024)
ap.add_argument("--chain", action="store_true")
args = ap.parse_args()

P = U64_DBFV
ctx = HipContext(P["n"], P["q"], P["aux"], plain_modulus=P["t"], gadget_base=P["gbase"])
dargs = (P["d"], P["base"], P["plain"])
key = [args.seed, 0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9]
sk = ctx.gen_secret_key(key, stream=1)
ctx.gen_relin_key(sk, key, stream=2, resident=True)

rng = np.random.default_rng(args.seed)
a_vals = rng.integers(0, 1 << 64, size=args.trials, dtype=np.uint64)
b_vals = rng.integers(0, 1 << 64, size=args.trials, dtype=np.uint64)
ct_a = ctx.dbfv_encrypt_sk(*dargs, a_vals, sk, key, stream=3)
ct_b = ctx.dbfv_encrypt_sk(*dargs, b_vals, sk, key, stream=4)
noise_a, noise_b = ctx.dbfv_noise(P["d"], ct_a, sk), ctx.dbfv_noise(P["d"], ct_b, sk)
ct_mul, _ = ctx.dbfv_mul(*dargs, ct_a, ct_b)
noise_out = ctx.dbfv_noise(P["d"], ct_mul, sk)
dec = ctx.dbfv_decrypt(*dargs, ct_mul, sk)
growths = []
for i in range(args.trials):
    noise_in = max(noise_a[i], noise_b[i], 1)
    growths.append(noise_out[i] / noise_in)
    ok = int(dec[i]) == (int(a_vals[i]) * int(b_vals[i])) % (1 << 64)
    print(f"trial {i}: noise_a {noise_a[i]} noise_b {noise_b[i]} noise_out {noise_out[i]} growth {growths[-1]:.1f} "
          f"budget {noise_budget_bits(noise_in, P['q'], P['t'])} -> {noise_budget_bits(noise_out[i], P['q'], P['t'])} bits "
          f"decrypts {'ok' if ok else 'WRONG'}")
print(json.dumps({"preset": "u64_dbfv", "seed": args.seed, "trials": args.trials,
                  "growth_mean": round(sum(growths) / len(growths), 1), "growth_max": round(max(growths), 1),
                  "noise_in_max": max(max(noise_a), max(noise_b)), "noise_out_max": max(noise_out),
                  "half_delta_bits": ((P["q"][0] // P["t"]) // 2).bit_length()}), flush=True)

if args.chain:
    factor, expected = 3, 5
    acc = ctx.dbfv_encrypt_sk(*dargs, [expected], sk, key, stream=5)
    y = ctx.dbfv_encrypt_sk(*dargs, [factor], sk, key, stream=6)
    print(f"chain step 0: noise {ctx.dbfv_noise(P['d'], acc, sk)[0]}")
    for step in range(1, 33):
        acc, _ = ctx.dbfv_mul(*dargs, acc, y)      # depth arrays left out: mul_depth 0, as the reference resets it
        expected = (expected * factor) % (1 << 64)
        got = int(ctx.dbfv_decrypt(*dargs, acc, sk)[0])
        nz = ctx.dbfv_noise(P["d"], acc, sk)[0]
        print(f"chain step {step}: noise {nz} ({nz.bit_length()} bits) budget {noise_budget_bits(nz, P['q'], P['t'])} "
              f"decrypts {'ok' if got == expected else 'WRONG'}")
        if got != expected:
            break
ctx.close()

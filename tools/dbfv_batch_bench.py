#!/usr/bin/env python3
"""Standalone benchmark of the fused slot-packed dBFV transforms (exacto_dbfv_batch_encode_dev /
exacto_dbfv_batch_decode_dev, batch.hip: one workgroup per item looping over the d digits) against the unfused
composition, in the same process on the same GPU and the same buffers:

  composition    : the digits of every value written to a [B][d][n] buffer of the tool's own, then
                   exacto_batch_encode_dev over its B d rows in place (encode); exacto_batch_decode_dev over the
                   B d rows into that buffer, then the signed recomposition over it (decode).  The library has no
                   entry point for the digit and recomposition passes alone (launch_dbfv_digits writes Delta m
                   rows, launch_dbfv_recompose sits behind decryption), so the tool runs them as element-wise
                   torch kernels on the library's stream: two for the digits (shift into the buffer, mask in
                   place), and the centring (three), the weights, the sum and the final mask for the
                   recomposition: more passes than a hand-written composition would make.
  transform_only : exacto_batch_encode_dev / exacto_batch_decode_dev over the B d rows alone.  Any unfused
                   composition contains it, so it is the composition's lower bound whatever the digit pass costs.

Shapes: the u64 shape (n = 4096, t = 1073153, b = 256, d = 8, p = 2^64, B = 512) and the cfg4 shape (n = 4096,
t = 270337, b = 256, d = 2, p = 2^16, B = 2048); and one exacto_dbfv_mul_dev timing on the u64 batching context
(three 60-bit primes, B = 16), with the slot products per second it implies.

HIP events on the library's stream.  One warm-up call of each (then two more untimed of each), then --windows
timed windows of --reps calls each, the variants alternating, so all see the same machine state; the spread of
the composition's windows is the noise a difference has to exceed.  Every result is checked
against the fused call's before timing.  Without --shape every shape runs in a child process of its own under
`timeout`, the first failure ends the run, and the rows are written to profiles/dbfv_batch_bench.json.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Q3 = [1152921504606830593, 1152921504606748673, 1152921504606683137]
SHAPES = {
    "u64": dict(n=4096, t=1073153, base=256, d=8, p=0, B=512),
    "cfg4": dict(n=4096, t=270337, base=256, d=2, p=65536, B=2048),
    "u64_mul": dict(n=4096, t=1073153, base=256, d=8, p=0, B=16, mul=True),
}
STEP_TIMEOUT_S = 240

ap = argparse.ArgumentParser()
ap.add_argument("--shape", choices=list(SHAPES), default=None)
ap.add_argument("--reps", type=int, default=20, help="calls per timed window")
ap.add_argument("--windows", type=int, default=7, help="timed windows per variant (alternating)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dbfv_batch_bench.json"))
args = ap.parse_args()


def drive():
    rows = []
    for name in SHAPES:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--shape", name,
               "--reps", str(args.reps), "--windows", str(args.windows)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(r.stderr)
        if r.returncode != 0:
            print(f"{name}: exit status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode
        for line in r.stdout.strip().splitlines():
            print(line, flush=True)
            rows.append(json.loads(line))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")
    return 0


def stats(v):
    v = sorted(v)
    return {"min": round(v[0], 4), "median": round(v[len(v) // 2], 4), "max": round(v[-1], 4)}


def run(name, sh):
    import torch
    from exacto_amd._ffi import HipContext

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

    def alternate(variants):
        """variants: name -> call.  Warm-up, then alternating windows; name -> list of ms per call."""
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        for _ in range(2):
            for fn in variants.values():
                fn()
        times = {k: [] for k in variants}
        for _ in range(args.windows):
            for k, fn in variants.items():
                times[k].append(window(fn, args.reps))
        return times

    n, t, base, d, p, B = sh["n"], sh["t"], sh["base"], sh["d"], sh["p"], sh["B"]
    shift = base.bit_length() - 1
    assert base == 1 << shift and (p == 0 or p & (p - 1) == 0), "the tool's digit passes are shifts and masks"
    ctx = HipContext(n, Q3, plain_modulus=t)
    ctx.set_stream(s.cuda_stream)
    ctx.batch_info()                                       # tables resident before anything is timed
    g = torch.Generator(device=dev)
    g.manual_seed(17)
    values = torch.randint(-2 ** 63, 2 ** 63 - 1, (B, n), generator=g, dtype=torch.int64, device=dev)
    if p:
        values &= p - 1

    if sh.get("mul"):
        key = [21, 22, 23, 24]
        sk_host = ctx.gen_secret_key(key, stream=1)
        ctx.gen_relin_key(sk_host, key, stream=2, resident=True)
        sk = torch.from_numpy(sk_host.view("int64")).to(dev)
        other = torch.randint(-2 ** 63, 2 ** 63 - 1, (B, n), generator=g, dtype=torch.int64, device=dev)
        ca = torch.empty((B, d, 2, ctx.L, n), dtype=torch.int64, device=dev)
        cb, out = torch.empty_like(ca), torch.empty_like(ca)
        ctx.dbfv_batch_encrypt_sk_dev(d, base, p, values, sk, key, 3, ca, B)
        ctx.dbfv_batch_encrypt_sk_dev(d, base, p, other, sk, key, 4, cb, B)
        got = torch.empty((B, n), dtype=torch.int64, device=dev)
        mul = lambda: ctx.dbfv_mul_dev(d, base, p, ca, cb, out, B)
        mul()
        ctx.dbfv_batch_decrypt_dev(d, base, p, out, sk, got, B)
        torch.cuda.synchronize()
        assert torch.equal(got, values * other), "dbfv_mul of slot-packed operands: wrong products"
        st = stats(alternate({"mul": mul})["mul"])
        print(json.dumps({
            "shape": name, "n": n, "t": t, "L": ctx.L, "base": base, "d": d, "p": p, "B": B,
            "dbfv_mul_ms": st, "ms_per_ciphertext": round(st["median"] / B, 4),
            "slot_products_per_s": round(B * n / (st["median"] * 1e-3)),
            "decrypts_to_the_wrapping_products": True,
        }), flush=True)
        ctx.close()
        return

    rows = torch.empty((B, d, n), dtype=torch.int64, device=dev)        # the composition's intermediate
    pt = torch.empty((B, d, n), dtype=torch.int64, device=dev)
    out = torch.empty((B, n), dtype=torch.int64, device=dev)
    shifts = (torch.arange(d, dtype=torch.int64, device=dev) * shift).view(1, d, 1)
    half, mask = t // 2, (p - 1) if p else -1

    def comp_encode():
        torch.bitwise_right_shift(values.unsqueeze(1), shifts, out=rows)
        rows.bitwise_and_(base - 1)
        ctx.batch_encode_dev(rows, rows, B * d)

    def comp_decode():
        ctx.batch_decode_dev(pt, rows, B * d)
        c = torch.where(rows > half, rows - t, rows)
        c.bitwise_left_shift_(shifts)                      # centred b^k, wrapping in 64 bits
        torch.sum(c, dim=1, out=out)
        if p:
            out.bitwise_and_(mask)

    # correctness of every variant before anything is timed
    ctx.dbfv_batch_encode_dev(d, base, p, values, pt, B)
    comp_encode()
    torch.cuda.synchronize()
    assert torch.equal(rows, pt), "the composition's encoding differs from the fused one"
    want = out.clone()
    ctx.dbfv_batch_decode_dev(d, base, p, pt, want, B)
    comp_decode()
    torch.cuda.synchronize()
    assert torch.equal(out, want) and torch.equal(want, values), "the composition's decoding differs from the fused one"

    pairs = {
        "encode": {"composition": comp_encode,
                   "transform_only": lambda: ctx.batch_encode_dev(rows, rows, B * d),
                   "fused": lambda: ctx.dbfv_batch_encode_dev(d, base, p, values, pt, B)},
        "decode": {"composition": comp_decode,
                   "transform_only": lambda: ctx.batch_decode_dev(pt, rows, B * d),
                   "fused": lambda: ctx.dbfv_batch_decode_dev(d, base, p, pt, out, B)},
    }
    fused_bytes = 8 * n * (1 + d) * B
    for direction, variants in pairs.items():
        tm = alternate(variants)
        st = {k: stats(v) for k, v in tm.items()}
        comp, fused, lower = st["composition"], st["fused"], st["transform_only"]
        spread = (comp["max"] - comp["min"]) / comp["median"]
        print(json.dumps({
            "shape": name, "direction": direction, "n": n, "t": t, "base": base, "d": d, "p": p, "B": B,
            "fused_ms": fused, "composition_ms": comp, "transform_only_ms": lower,
            "fused_rounds": [round(x, 4) for x in tm["fused"]],
            "composition_rounds": [round(x, 4) for x in tm["composition"]],
            "transform_only_rounds": [round(x, 4) for x in tm["transform_only"]],
            "composition_spread": round(spread, 4),
            "ratio_composition_over_fused": round(comp["median"] / fused["median"], 3),
            "ratio_transform_only_over_fused": round(lower["median"] / fused["median"], 3),
            "faster_than_composition_by_more_than_spread": bool(fused["median"] < comp["median"] * (1 - spread)),
            "faster_than_transform_only": bool(fused["median"] < lower["median"]),
            "fused_algorithmic_bytes": fused_bytes,
            "fused_TBs": round(fused_bytes / (fused["median"] * 1e-3) / 1e12, 3),
        }), flush=True)
    ctx.close()


if args.shape is None:
    sys.exit(drive())
run(args.shape, SHAPES[args.shape])

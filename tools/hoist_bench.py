#!/usr/bin/env python3
"""Standalone timing of the hoisted rotations against one automorphism call per rotation, on one GPU:

  cfg3_B64_R16   : bfv_rotate_hoisted_dev against R calls of bfv_apply_automorphism_dev, n = 4096, L = 3
  cfg3_B1_R64    : the same with one ciphertext and 64 rotations
  u64_B512_R8    : u64_dbfv's ring (n = 4096, L = 1, base 256: the limb-wise multiply-accumulate)
  cfg3_lt_B64_R16: bfv_linear_transform_dev against R automorphisms + R bfv_plain_mul_dev + R - 1 bfv_add_dev

Both forms run on the same buffers in the same process.  The key set is created outside the timed region and
exacto_galois_keyset_create_dev is timed on its own (wall clock around the synchronous call, best of three).
HIP events on the library's stream, one warm-up call, then --reps calls per timing, the two forms alternating
--rounds times, best of the rounds with every round shown.  The keys are device-generated for one secret key
and the outputs of both forms are decrypt-checked once against the rotated slots (the two forms do not give
the same bits: DESIGN.md §4).  Every row also carries the library's per-family records of one call of each
form (exacto_prof_read).

Without --shape every shape runs in a child process of its own under `timeout`, the first failure ends the
run, and the rows are written to profiles/hoist_bench.json.  Nothing outside the tree is read.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Q3 = [1152921504606830593, 1152921504606748673, 1152921504606683137]
SHAPES = {
    "cfg3_B64_R16": dict(n=4096, q=Q3, t=65537, gbase=0, B=64, R=16, lt=False),
    "cfg3_B1_R64": dict(n=4096, q=Q3, t=65537, gbase=0, B=1, R=64, lt=False),
    "u64_B512_R8": dict(n=4096, q=Q3[:1], aux=[18014398509998081, 36028797018972161], t=1040407, gbase=256, B=512, R=8,
                        lt=False),
    "cfg3_lt_B64_R16": dict(n=4096, q=Q3, t=65537, gbase=0, B=64, R=16, lt=True),
}
KINDS = {0: "fwd_ntt", 1: "inv_ntt", 6: "ks32_digit_ntt", 7: "ks32_mac", 8: "ks32_crt", 15: "relin_mac"}
STEP_TIMEOUT_S = 240
KEY = [11, 22, 33, 44]

ap = argparse.ArgumentParser()
ap.add_argument("--shape", choices=list(SHAPES), default=None)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hoist_bench.json"))
args = ap.parse_args()


def drive():
    rows = []
    for name in SHAPES:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--shape", name,
               "--reps", str(args.reps), "--rounds", str(args.rounds)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(r.stderr)
        if r.returncode != 0:
            print(f"{name}: exit status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode
        row = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps({k: v for k, v in row.items() if k != "families"}), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")
    return 0


def families(ctx, call):
    import torch
    call()
    torch.cuda.synchronize()
    ctx.prof_enable(True)
    try:
        call()
        recs = {k: ctx.prof_read(k) for k in KINDS}
    finally:
        ctx.prof_enable(False)
    return {KINDS[k]: {"launches": r["launches"], "ms": round(r["ms"], 4), "units": r["polys"]}
            for k, r in recs.items() if r["launches"]}


def run(name, sh):
    import numpy as np
    import torch
    from exacto_amd import _ffi
    from exacto_amd._ffi import HipContext

    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream()
    n, q, B, R, lt, t = sh["n"], sh["q"], sh["B"], sh["R"], sh["lt"], sh["t"]
    L = len(q)
    ctx = HipContext(n, q, sh.get("aux", ()), plain_modulus=t, gadget_base=sh["gbase"])
    ctx.set_stream(s.cuda_stream)
    G = ctx.G
    batching = (t - 1) % (2 * n) == 0

    def to_dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)

    def to_host(x):
        return x.cpu().numpy().view(np.uint64)

    # one secret key, R distinct row rotations, their keys generated on the device
    sk = ctx.gen_secret_key(KEY, stream=1)
    steps = list(range(1, R + 1))
    elements = [_ffi.galois_element_rotate_rows(n, k) for k in steps]
    gks = torch.stack([to_dev(ctx.gen_galois_key(sk, e, KEY, stream=10 + r)) for r, e in enumerate(elements)])
    rng = np.random.default_rng(3)
    v = rng.integers(0, t, size=(B, n), dtype=np.uint64)
    pt = ctx.batch_encode(v) if batching else v
    ct = to_dev(ctx.encrypt_sk(pt, sk, KEY, stream=3))
    w = rng.integers(0, t, size=(R, n), dtype=np.uint64)
    pts = to_dev(ctx.batch_encode(w) if batching else w)
    torch.cuda.synchronize()

    t_create = []
    ks = None
    for _ in range(3):
        if ks is not None:
            ks.close()
        ctx.synchronize()
        t0 = time.perf_counter()
        ks = ctx.galois_keyset_dev(elements, gks, G)
        t_create.append((time.perf_counter() - t0) * 1e3)

    rot_base = torch.zeros((R, B, 2, L, n), dtype=torch.int64, device=dev)
    rot_hoist = torch.zeros((B, R, 2, L, n), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def base_rotations():
        for r in range(R):
            ctx.bfv_apply_automorphism_dev(ct, elements[r], gks[r], G, rot_base[r], B)

    if lt:
        pts_b = pts[:, None, :].expand(R, B, n).contiguous()      # bfv_plain_mul_dev takes one plaintext per item
        prod = torch.zeros((B, 2, L, n), dtype=torch.int64, device=dev)
        o0 = torch.zeros((B, 2, L, n), dtype=torch.int64, device=dev)
        o1 = torch.zeros_like(o0)
        torch.cuda.synchronize()

        def base():
            base_rotations()
            ctx.bfv_plain_mul_dev(rot_base[0], 2, pts_b[0], o0, B)
            for r in range(1, R):
                ctx.bfv_plain_mul_dev(rot_base[r], 2, pts_b[r], prod, B)
                ctx.bfv_add_dev(o0, 2, prod, 2, o0, B)

        hoisted = lambda: ctx.bfv_linear_transform_dev(ct, ks, pts, o1, B)
        calls = ("R x bfv_apply_automorphism_dev + R x bfv_plain_mul_dev + (R - 1) x bfv_add_dev",
                 "bfv_linear_transform_dev")
    else:
        base = base_rotations
        hoisted = lambda: ctx.bfv_rotate_hoisted_dev(ct, ks, rot_hoist, B)
        calls = ("R x bfv_apply_automorphism_dev", "bfv_rotate_hoisted_dev")

    def timed(fn):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(args.reps):
            fn()
        e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps

    t_base, t_h = [], []
    for _ in range(args.rounds):
        t_base.append(timed(base))
        t_h.append(timed(hoisted))

    # decrypt check, once: both forms against the plaintext they should hold
    def roll(x, k):
        h = n // 2
        return np.concatenate([np.roll(x[..., :h], -k, axis=-1), np.roll(x[..., h:], -k, axis=-1)], axis=-1)

    def auto_plain(x, e):        # sigma_e on plaintext coefficients mod t (no batching)
        idx = (np.arange(n, dtype=np.int64) * e) % (2 * n)
        out = np.zeros_like(x)
        out[..., idx % n] = np.where(idx < n, x, (t - x) % t)
        return out

    ok = True
    nb = min(B, 2)
    if lt:
        want = np.zeros((nb, n), dtype=object)
        for r, k in enumerate(steps):
            want = (want + w[r].astype(object) * roll(v[:nb], k).astype(object)) % t
        for o in (o0, o1):
            ok = ok and np.array_equal(ctx.batch_decrypt(to_host(o[:nb]), sk), want.astype(np.uint64))
    else:
        for r in (0, R - 1):
            for got in (rot_base[r, :nb], rot_hoist[:nb, r]):
                got = to_host(got.contiguous())
                if batching:
                    ok = ok and np.array_equal(ctx.batch_decrypt(got, sk), roll(v[:nb], steps[r]))
                else:
                    ok = ok and np.array_equal(ctx.bfv_decrypt(got, sk), auto_plain(v[:nb], elements[r]))
    fam = {"baseline": families(ctx, base), "hoisted": families(ctx, hoisted)}
    tb, th = min(t_base), min(t_h)
    spread = (max(t_base) - min(t_base)) / min(t_base)
    print(json.dumps({
        "shape": name, "n": n, "L": L, "B": B, "R": R, "G": G, "ks32_primes": ks.ks32_primes,
        "baseline": calls[0], "hoisted": calls[1],
        "baseline_ms": round(tb, 4), "hoisted_ms": round(th, 4), "baseline_over_hoisted": round(tb / th, 4),
        "baseline_ms_rounds": [round(x, 4) for x in t_base], "hoisted_ms_rounds": [round(x, 4) for x in t_h],
        "baseline_spread": round(spread, 4), "faster_by_more_than_spread": bool(tb / th - 1 > spread),
        "keyset_create_ms": round(min(t_create), 3), "keyset_create_ms_rounds": [round(x, 3) for x in t_create],
        "decrypt_ok": ok, "families": fam,
    }), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(run(args.shape, SHAPES[args.shape]) if args.shape else drive())

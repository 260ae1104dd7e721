#!/usr/bin/env python3
"""Standalone benchmark of the fused dBFV plaintext product (exacto_dbfv_plain_mul_dev, dbfv_plain.hip: the
plaintext lift, then one streaming kernel that forms the surviving digit pairs in registers) against the
composition of the entry points that existed before it, in the same process on the same GPU:

  composition : exacto_bfv_plain_mul_dev per surviving digit pair (i, j) over the B items (each call lifts its
                plaintext digit again: that is what the entry point does), exacto_dbfv_add_dev of the products by
                i + j, and exacto_dbfv_linear_map_dev for the fold when a high limb has a non-zero representative
                (neither timed shape has one: 16^2 = 256 and 256^8 = 2^64).  The operands are held limb-major
                ([d][B][2][L][n], [d][B][n]) for it, copies made outside the timed windows; a shared plaintext is
                expanded to one row per item there too, since exacto_bfv_plain_mul_dev has no shared form.
  dbfv_mul    : exacto_dbfv_mul_dev on MUL_B of the same ciphertexts against themselves (the route through an
                encrypted operand), per ciphertext.

Shapes: cfg3's three 60-bit primes at n = 4096, B = 512: (b = 16, d = 2, p = 256, t = 12289) and the u64
profile (b = 256, d = 8, p = 2^64, t = 1073153), each with one plaintext per item and with one shared
plaintext.  The operands are uniform residues and uniform plaintext coefficients below t: timing does not
depend on their values, and the equality of the two routes is checked on them before anything is timed.

HIP events on the library's stream.  One warm-up call of each (then two more untimed of each), then --windows
timed windows of --reps calls each, the variants alternating, so both see the same machine state; the spread
of the composition's windows is the noise a difference has to exceed.  Without --shape every shape runs in a
child process of its own under `timeout`, the first failure ends the run, and the rows are written to
profiles/dbfv_plain_bench.json.
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
    "d2": dict(n=4096, t=12289, base=16, d=2, p=256, B=512),
    "u64": dict(n=4096, t=1073153, base=256, d=8, p=0, B=512),
}
MUL_B = 16
STEP_TIMEOUT_S = 300

ap = argparse.ArgumentParser()
ap.add_argument("--shape", choices=list(SHAPES), default=None)
ap.add_argument("--reps", type=int, default=50, help="calls per timed window")
ap.add_argument("--windows", type=int, default=7, help="timed windows per variant (alternating)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dbfv_plain_bench.json"))
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


def small_reps(base, d, p):
    reps = []
    for j in range(d, 2 * d - 1):
        val = pow(base, j, (1 << 64) if p == 0 else p)
        reps.append([val // base ** k % base for k in range(d)])
    return reps


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
    ctx = HipContext(n, Q3, plain_modulus=t)
    ctx.set_stream(s.cuda_stream)
    L = ctx.L
    g = torch.Generator(device=dev)
    g.manual_seed(23)
    ct = torch.stack([torch.randint(0, q, (B, d, 2, n), generator=g, dtype=torch.int64, device=dev) for q in Q3], dim=3)
    assert ct.shape == (B, d, 2, L, n)
    ct = ct.contiguous()
    pt_own = torch.randint(0, t, (B, d, n), generator=g, dtype=torch.int64, device=dev)
    out = torch.empty_like(ct)

    reps = small_reps(base, d, p)
    live = [any(r) for r in reps]
    pairs = [(i, j) for i in range(d) for j in range(d) if i + j < d or live[i + j - d]]
    nwide = d + (max(m for m, x in enumerate(live) if x) + 1 if any(live) else 0)
    ct_limb = ct.permute(1, 0, 2, 3, 4).contiguous()                      # [d][B][2][L][n]
    wide = torch.empty((nwide, B, 2, L, n), dtype=torch.int64, device=dev)
    tmp = torch.empty((B, 2, L, n), dtype=torch.int64, device=dev)
    folded = torch.empty((d, B, 2, L, n), dtype=torch.int64, device=dev) if any(live) else None
    import numpy as np
    matrix = np.zeros((d, nwide), dtype=np.uint64)
    for i in range(d):
        matrix[i, i] = 1
        for m in range(d, nwide):
            matrix[i, m] = reps[m - d][i]

    def composition(pt_limb):
        def call():
            seen = set()
            for i, j in pairs:
                m = i + j
                if m not in seen:
                    seen.add(m)
                    ctx.bfv_plain_mul_dev(ct_limb[j], 2, pt_limb[i], wide[m], B)
                else:
                    ctx.bfv_plain_mul_dev(ct_limb[j], 2, pt_limb[i], tmp, B)
                    ctx.dbfv_add_dev(wide[m], 1, 2, tmp, 1, 2, wide[m], B)
            if folded is not None:                         # limbs as items of one ciphertext with 2 B components
                ctx.dbfv_linear_map_dev(matrix, 2 * B, wide, folded, 1)
        return call

    results = wide if folded is None else folded
    for mode in ("own", "shared"):
        pt = pt_own if mode == "own" else pt_own[:1].contiguous()
        pb = pt.shape[0]
        pt_limb = pt.expand(B, d, n).permute(1, 0, 2).contiguous()         # [d][B][n]
        fused = lambda: ctx.dbfv_plain_mul_dev(d, base, p, ct, 2, pt, pb, out, B)
        comp = composition(pt_limb)
        # the two routes give equal outputs, before anything is timed
        out.fill_(-1)
        fused()
        comp()
        torch.cuda.synchronize()
        for k in range(d):
            assert torch.equal(out[:, k], results[k]), f"the composition's limb {k} differs from the fused call's"
        tm = alternate({"composition": comp, "fused": fused})
        st = {k: stats(v) for k, v in tm.items()}
        c, f = st["composition"], st["fused"]
        spread = (c["max"] - c["min"]) / c["median"]
        # the least the call moves through HBM: every ciphertext limb read and every output limb written once, each
        # lifted plaintext row read once (the second component's read and a shared plaintext's come from cache);
        # the lift before the kernel (pb d rows scaled, transformed in place) is not counted
        min_bytes = 8 * n * L * (2 * 2 * d * B + d * pb)
        row = {
            "shape": name, "plaintext": mode, "n": n, "t": t, "L": L, "base": base, "d": d, "p": p, "B": B,
            "surviving_pairs": len(pairs), "fold": bool(any(live)),
            "fused_ms": f, "composition_ms": c,
            "fused_rounds": [round(x, 4) for x in tm["fused"]],
            "composition_rounds": [round(x, 4) for x in tm["composition"]],
            "composition_spread": round(spread, 4),
            "ratio_composition_over_fused": round(c["median"] / f["median"], 3),
            "faster_than_composition_by_more_than_spread": bool(f["median"] < c["median"] * (1 - spread)),
            "outputs_equal": True,
            "min_hbm_bytes": min_bytes,
            "fused_call_TBs": round(min_bytes / (f["median"] * 1e-3) / 1e12, 3),
            "products_64x64_per_s": round(len(pairs) * 2 * L * n * B / (f["median"] * 1e-3)),
        }
        if mode == "shared":
            # the route through an encrypted operand, on MUL_B of the ciphertexts (uniform residues time as any)
            key = [21, 22, 23, 24]
            sk_host = ctx.gen_secret_key(key, stream=1)
            ctx.gen_relin_key(sk_host, key, stream=2, resident=True)
            a = ct[:MUL_B].contiguous()
            mo = torch.empty_like(a)
            mul = lambda: ctx.dbfv_mul_dev(d, base, p, a, a, mo, MUL_B)
            ms = stats(alternate({"mul": mul})["mul"])
            row["dbfv_mul_B"] = MUL_B
            row["dbfv_mul_ms"] = ms
            row["dbfv_mul_ms_per_ciphertext"] = round(ms["median"] / MUL_B, 4)
            row["fused_ms_per_ciphertext"] = round(f["median"] / B, 5)
            row["ratio_dbfv_mul_over_fused_per_ciphertext"] = round(ms["median"] / MUL_B / (f["median"] / B), 1)
        print(json.dumps(row), flush=True)
    ctx.close()


if args.shape is None:
    sys.exit(drive())
run(args.shape, SHAPES[args.shape])

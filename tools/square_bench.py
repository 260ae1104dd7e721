#!/usr/bin/env python3
"""Standalone timing of the squares against the two-operand calls on the same buffer, on one GPU:

  cfg3      : bfv_square_and_relin_dev(a) against bfv_mul_and_relin_dev(a, a), n = 4096, L = 3, B = 1024;
  cfg4      : dbfv_square_dev(a) against dbfv_mul_dev(a, a), n = 4096, L = 3, d = 2, B = 256;
  cfg5      : the same at n = 8192, L = 4, d = 8, B = 16;
  eval_poly : exacto_eval_poly_dev of a degree-28 polynomial over cfg3's basis, B = 64, on a context with
              set_square_hook(False) (every baby step the two-operand call) against the default context
              (even baby steps on the square path).

HIP events on the library's stream, one warm-up call, then --reps calls per timing, the two calls
alternating --rounds times, best of the rounds; the outputs of the two calls are compared once.  Every row
also carries the library's own per-family records of one call of each form (exacto_prof_read: launches,
ms, units), so a row that gains little shows where the time stayed.

Without --shape every shape runs in a child process of its own under `timeout`, the first failure ends the
run, and the rows are written to profiles/square_bench.json.  Nothing outside the tree is read.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Q4 = [1152921504606830593, 1152921504606748673, 1152921504606683137, 1152921504606601217]
SHAPES = {
    "cfg3": dict(n=4096, q=Q4[:3], t=65537, gbase=0, B=1024, d=0),
    "cfg4": dict(n=4096, q=Q4[:3], t=260111, gbase=0, B=256, d=2, base=256, p=65536),
    "cfg5": dict(n=8192, q=Q4, t=1040407, gbase=256, B=16, d=8, base=256, p=0),
    "eval_poly": dict(n=4096, q=Q4[:3], t=65537, gbase=0, B=64, d=0, degree=28),
}
KINDS = {0: "fwd_ntt", 1: "inv_ntt", 2: "tensor_inv", 3: "polymul", 4: "exact_lift", 5: "exact_scale",
         6: "ks32_digit_ntt", 7: "ks32_mac", 8: "ks32_crt", 9: "dbfv_pairsum", 10: "psum_scale",
         12: "ks32_digit_sum", 13: "dbfv_combine", 14: "hps_extend", 15: "relin_mac", 16: "hps_scale"}
STEP_TIMEOUT_S = 240

ap = argparse.ArgumentParser()
ap.add_argument("--shape", choices=list(SHAPES), default=None)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--batch", type=int, default=0, help="override B (0: the shape's)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "square_bench.json"))
args = ap.parse_args()


def drive():
    rows = []
    for name in SHAPES:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--shape", name,
               "--reps", str(args.reps), "--rounds", str(args.rounds), "--batch", str(args.batch)]
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
    import torch
    from exacto_amd._ffi import HipContext

    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream()
    n, q, B, d = sh["n"], sh["q"], args.batch or sh["B"], sh["d"]
    L = len(q)

    def context():
        ctx = HipContext(n, q, plain_modulus=sh["t"], gadget_base=sh["gbase"])
        ctx.set_stream(s.cuda_stream)
        return ctx

    g = torch.Generator(device=dev)
    g.manual_seed(5)

    def uniform(*lead):
        return torch.stack([torch.randint(0, qi, lead + (n,), generator=g, dtype=torch.int64, device=dev) for qi in q],
                           dim=len(lead)).contiguous()

    def timed(fn):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(args.reps):
            fn()
        e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps

    ctx = context()
    rlk = uniform(ctx.G, 2)                     # [G][2][L][n]
    ctx.load_relin_key_dev(rlk, ctx.G)
    base_ctx = ctx
    if name == "eval_poly":
        base_ctx = context()
        base_ctx.set_square_hook(False)
        base_ctx.load_relin_key_dev(rlk, ctx.G)
        a = uniform(B, 2)
        coeffs = [(7 * i + 3) % sh["t"] or 1 for i in range(sh["degree"] + 1)]
        o0, o1 = torch.zeros_like(a), torch.zeros_like(a)
        base = lambda: base_ctx.eval_poly_dev(a, coeffs, o0, B)
        square = lambda: ctx.eval_poly_dev(a, coeffs, o1, B)
        calls = ("eval_poly_dev, set_square_hook(False)", "eval_poly_dev")
    elif d:
        a = uniform(B, d, 2)
        o0, o1 = torch.zeros_like(a), torch.zeros_like(a)
        base = lambda: ctx.dbfv_mul_dev(d, sh["base"], sh["p"], a, a, o0, B)
        square = lambda: ctx.dbfv_square_dev(d, sh["base"], sh["p"], a, o1, B)
        calls = ("dbfv_mul_dev(a, a)", "dbfv_square_dev(a)")
    else:
        a = uniform(B, 2)
        o0, o1 = torch.zeros_like(a), torch.zeros_like(a)
        base = lambda: ctx.bfv_mul_and_relin_dev(a, a, o0, B)
        square = lambda: ctx.bfv_square_and_relin_dev(a, o1, B)
        calls = ("bfv_mul_and_relin_dev(a, a)", "bfv_square_and_relin_dev(a)")
    torch.cuda.synchronize()
    t_base, t_sq = [], []
    for _ in range(args.rounds):
        t_base.append(timed(base))
        t_sq.append(timed(square))
    same = bool(torch.equal(o0, o1))
    fam = {"baseline": families(base_ctx, base), "square": families(ctx, square)}
    tb, ts = min(t_base), min(t_sq)
    print(json.dumps({
        "shape": name, "n": n, "L": L, "B": B, "d": d, "baseline": calls[0], "square": calls[1],
        "baseline_ms": round(tb, 4), "square_ms": round(ts, 4), "square_over_baseline": round(ts / tb, 4),
        "baseline_ms_rounds": [round(x, 4) for x in t_base], "square_ms_rounds": [round(x, 4) for x in t_sq],
        "baseline_spread": round((max(t_base) - min(t_base)) / min(t_base), 4),
        "outputs_equal": same, "families": fam,
    }), flush=True)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(run(args.shape, SHAPES[args.shape]) if args.shape else drive())

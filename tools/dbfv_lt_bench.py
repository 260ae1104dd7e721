#!/usr/bin/env python3
"""Standalone benchmark of the dBFV slot linear transform (exacto_dbfv_linear_transform[_prepared]_dev: the
hoisted rotations of the limbs joined with the wide plaintext product) against the composition of the entry
points that existed before it, in the same process on the same GPU:

  prepared    : exacto_dbfv_linear_transform_prepared_dev (resident lifted diagonals);
  raw         : exacto_dbfv_linear_transform_dev (the R d diagonal rows lifted on every call);
                on the limb-wise shape these two run with the fused kernel switched on
                (exacto_ctx_set_dbfv_lt_fused(ctx, 1)): they are its measurement;
  staged      : the prepared call on the staged route, the library's default, on the limb-wise shape only (on the
                31-bit key switch the prepared call is the staged route already);
  composition : exacto_bfv_rotate_hoisted_dev on the B d limbs ([B d][R] outputs), a transposing device copy to
                [B][R][d], and exacto_dbfv_plain_mul_sum_dev with K = R (which lifts the diagonals again).

Shapes, all with R = 16 row rotations (steps 0 .. 15, step 0 the identity) and uniform residues: cfg3's three
60-bit primes at n = 4096 with (b = 16, d = 2, p = 256) and with (b = 256, d = 8, p = 2^64), the 31-bit key
switch; the u64_dbfv preset's single 60-bit prime at n = 4096 with (256, 8, 2^64), the limb-wise key switch and
the fused kernel.  B d = 64 limbs, so the rotated limbs of the composition (B d R outputs) fit the default chunk.
Timing does not depend on the values, and the equality of the routes is checked before anything is timed.

HIP events on the library's stream.  One warm-up call of each (then two more untimed of each), then --windows
timed windows of --reps calls each, the routes alternating, so all see the same machine state; the spread of the
composition's windows is the noise a difference has to exceed.  Without --shape every shape runs in a child
process of its own under `timeout`, the first failure ends the run, and the rows are written to
profiles/dbfv_lt_bench.json.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R = 16
SHAPES = {
    "cfg3_d2": dict(preset="cfg3", base=16, d=2, p=256, B=32),
    "cfg3_u64": dict(preset="cfg3", base=256, d=8, p=0, B=8),
    "hps_u64": dict(preset="u64_dbfv", base=256, d=8, p=0, B=8),
}
STEP_TIMEOUT_S = 300

ap = argparse.ArgumentParser()
ap.add_argument("--shape", choices=list(SHAPES), default=None)
ap.add_argument("--reps", type=int, default=20, help="calls per timed window")
ap.add_argument("--windows", type=int, default=7, help="timed windows per route (alternating)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dbfv_lt_bench.json"))
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
    from exacto_amd import _ffi
    from exacto_amd._ffi import HipContext
    from oracle import params as P

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

    base, d, p, B = sh["base"], sh["d"], sh["p"], sh["B"]
    prm = P.cfg3_params(4096) if sh["preset"] == "cfg3" else P.u64_dbfv().bfv_params
    n, moduli = prm.ring_degree, [int(q) for q in prm.ct_basis.moduli]
    assert n == 4096
    ctx = HipContext.from_params(prm)
    ctx.set_stream(s.cuda_stream)
    L, G = ctx.L, ctx.G
    g = torch.Generator(device=dev)
    g.manual_seed(29)

    def residues(*lead):
        x = torch.stack([torch.randint(0, q, (*lead, n), generator=g, dtype=torch.int64, device=dev) for q in moduli],
                        dim=len(lead))
        return x.contiguous()

    ct = residues(B, d, 2)                                     # [B][d][2][L][n]
    gks = residues(R, G, 2)                                    # [R][G][2][L][n]
    # uniform 63-bit words: any u64 is a plaintext coefficient, and timing does not depend on them
    pts = torch.randint(0, 2 ** 63 - 1, (R, d, n), generator=g, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    elements = [_ffi.galois_element_rotate_rows(n, k) for k in range(R)]
    ks = ctx.galois_keyset_dev(elements, gks, G)
    dg = ctx.dbfv_diagonals_dev(d, pts, R)
    limbwise = ks.ks32_primes == 0
    assert not dg.fused                                        # the default is the staged route
    if limbwise:
        ctx.set_dbfv_lt_fused(True)
        dg.close()
        dg = ctx.dbfv_diagonals_dev(d, pts, R)
        assert dg.fused

    out = {k: torch.empty_like(ct) for k in ("prepared", "raw", "staged", "composition")}
    H = torch.empty((B * d, R, 2, L, n), dtype=torch.int64, device=dev)
    Ht = torch.empty((B, R, d, 2, L, n), dtype=torch.int64, device=dev)

    def prepared():
        ctx.dbfv_linear_transform_dev(d, base, p, ct, ks, dg, out["prepared"], B)

    def raw():
        ctx.dbfv_linear_transform_dev(d, base, p, ct, ks, pts, out["raw"], B)

    def staged():
        ctx.set_dbfv_lt_fused(False)
        ctx.dbfv_linear_transform_dev(d, base, p, ct, ks, dg, out["staged"], B)
        ctx.set_dbfv_lt_fused(True)

    def composition():
        ctx.bfv_rotate_hoisted_dev(ct, ks, H, B * d)
        Ht.copy_(H.view(B, d, R, 2, L, n).permute(0, 2, 1, 3, 4, 5))
        ctx.dbfv_plain_mul_sum_dev(d, base, p, Ht, R, 2, pts, 1, out["composition"], B)

    variants = {"prepared": prepared, "raw": raw, "composition": composition}
    if limbwise:
        variants["staged"] = staged
    # every route gives the composition's bits, before anything is timed
    for k, fn in variants.items():
        out[k].fill_(-1)
        fn()
    torch.cuda.synchronize()
    for k in variants:
        assert torch.equal(out[k], out["composition"]), f"{k} differs from the composition"
    tm = alternate(variants)
    st = {k: stats(v) for k, v in tm.items()}
    c = st["composition"]
    spread = (c["max"] - c["min"]) / c["median"]
    # the least a call moves through HBM: every input limb read and every output limb written once, the lifted
    # diagonals and the prepared keys (with their Shoup companions, or the 31-bit rows) read once
    key_bytes = R * G * 2 * L * n * (16 if limbwise else 4 * ks.ks32_primes)
    min_bytes = 8 * n * L * (2 * 2 * d * B + R * d) + key_bytes
    row = {
        "shape": name, "n": n, "L": L, "base": base, "d": d, "p": p, "B": B, "R": R, "gadget_digits": G,
        "ks32_primes": ks.ks32_primes, "fused_kernel": bool(dg.fused),
        "rotated_limb_bytes_of_the_composition": 8 * B * d * R * 2 * L * n,
        "composition_spread": round(spread, 4), "outputs_equal": True, "min_hbm_bytes": min_bytes,
    }
    for k in variants:
        row[k + "_ms"] = st[k]
        row[k + "_rounds"] = [round(x, 4) for x in tm[k]]
        row[k + "_min_traffic_TBs"] = round(min_bytes / (st[k]["median"] * 1e-3) / 1e12, 3)
        if k != "composition":
            row["ratio_composition_over_" + k] = round(c["median"] / st[k]["median"], 3)
            row[k + "_faster_than_composition_by_more_than_spread"] = bool(st[k]["median"] < c["median"] * (1 - spread))
    if limbwise:
        f, g_ = st["prepared"], st["staged"]
        row["ratio_staged_over_fused"] = round(g_["median"] / f["median"], 3)
        row["fused_faster_than_staged_by_more_than_spread"] = bool(f["median"] < g_["median"] * (1 - spread))
    print(json.dumps(row), flush=True)
    ks.close()
    dg.close()
    ctx.close()


if args.shape is None:
    sys.exit(drive())
run(args.shape, SHAPES[args.shape])

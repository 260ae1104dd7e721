#!/usr/bin/env python3
"""Standalone benchmark of the dBFV base change and the dBFV scalar encryption at the shapes of the
dBFV configurations (cfg5: n=8192, L=4, B=64, (256, 8) -> (16, 16); cfg4: n=4096, L=3, B=1024,
(256, 2) -> (16, 4)), each against what a caller composes without them:

  change_base : exacto_dbfv_change_base_dev (one fused kernel) against the same digit vectors built
                from exacto_rns_scalar_mul_dev + exacto_rns_add_dev, one pass per non-zero matrix entry
                (the composition gets limb-major buffers, so each of its passes is contiguous);
  encrypt_sk  : exacto_dbfv_encrypt_sk_dev (values on the device) against decomposing on the host,
                uploading the [B*d][n] digit plaintexts and exacto_encrypt_sk_dev.

HIP events on the library's stream, one warm-up call, then --reps calls; prints one JSON line per
shape.  Bytes moved by the map: (d_in + d_out) ciphertext limbs per item, each residue once.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from exacto_amd import _ffi  # noqa: E402
from exacto_amd._ffi import HipContext  # noqa: E402

Q4 = [1152921504606830593, 1152921504606748673, 1152921504606683137, 1152921504606601217]
SHAPES = {
    "cfg5": dict(n=8192, q=Q4, t=1040407, gbase=256, B=64, d=8, base=256, plain=0, new_base=16, new_d=16),
    "cfg4": dict(n=4096, q=Q4[:3], t=260111, gbase=0, B=1024, d=2, base=256, plain=65536, new_base=16, new_d=4),
}
HBM_LINE = 8.0e12   # bytes / s, the MI355X line DESIGN.md measures against
KEY = [1, 2, 3, 4]

ap = argparse.ArgumentParser()
ap.add_argument("--shape", choices=list(SHAPES) + ["all"], default="all")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--batch", type=int, default=0, help="override B (0: the shape's)")
ap.add_argument("--dense", action="store_true",
                help="also time exacto_dbfv_linear_map_dev with a dense random matrix of the same size")
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
    n, q, B, d, nd = sh["n"], sh["q"], args.batch or sh["B"], sh["d"], sh["new_d"]
    L = len(q)
    ctx = HipContext(n, q, plain_modulus=sh["t"], gadget_base=sh["gbase"])
    ctx.set_stream(s.cuda_stream)
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    x = torch.stack([torch.randint(0, qi, (B, d, 2, n), generator=g, dtype=torch.int64, device=dev) for qi in q],
                    dim=3).contiguous()                                   # [B][d][2][L][n]
    out = torch.zeros((B, nd, 2, L, n), dtype=torch.int64, device=dev)
    m = _ffi.dbfv_change_base_matrix(d, sh["base"], sh["plain"], sh["new_base"], nd)
    t_map = timed(lambda: ctx.dbfv_change_base_dev(d, sh["base"], sh["plain"], sh["new_base"], nd, x, out, B),
                  args.reps)

    t_dense = None
    if args.dense:   # every entry non-zero: d_in * d_out Shoup products per slot, inputs re-read per output limb
        md = np.random.default_rng(8).integers(2, sh["t"], size=(nd, d), dtype=np.uint64)
        t_dense = timed(lambda: ctx.dbfv_linear_map_dev(md, 2, x, out, B), args.reps)
        ctx.dbfv_change_base_dev(d, sh["base"], sh["plain"], sh["new_base"], nd, x, out, B)

    # the composition: limb-major copies, out_j = sum_i m_ji in_i by scalar_mul (+ add)
    xl = x.permute(1, 0, 2, 3, 4).contiguous()                            # [d][B][2][L][n]
    ol = torch.zeros((nd, B, 2, L, n), dtype=torch.int64, device=dev)
    tmp = torch.zeros((B, 2, L, n), dtype=torch.int64, device=dev)
    t_mod = sh["t"]

    def composed():
        for j in range(nd):
            first = True
            for i in range(d):
                c = int(m[j, i]) % t_mod
                if c == 0:
                    continue
                ctx.rns_scalar_mul_dev(xl[i], c, ol[j] if first else tmp, B * 2)
                if not first:
                    ctx.rns_add_dev(ol[j], tmp, ol[j], B * 2)
                first = False
            if first:
                ctx.rns_sub_dev(xl[0], xl[0], ol[j], B * 2)               # the reference's bfv_sub(x, x)
    t_comp = timed(composed, max(1, args.reps // 2))
    torch.cuda.synchronize()
    same = bool(torch.equal(ol.permute(1, 0, 2, 3, 4), out))
    nnz = int(np.count_nonzero(m % np.uint64(t_mod)))
    moved = (d + nd) * B * 2 * L * n * 8

    # scalar encryption
    vals = np.random.default_rng(5).integers(0, 1 << 63, size=B, dtype=np.uint64)
    sk = torch.from_numpy(ctx.gen_secret_key(KEY, stream=1).view(np.int64)).to(dev)
    ct = torch.zeros((B, d, 2, L, n), dtype=torch.int64, device=dev)
    ct2 = torch.zeros_like(ct)
    v_dev = torch.from_numpy(vals.view(np.int64)).to(dev)
    t_enc = timed(lambda: ctx.dbfv_encrypt_sk_dev(d, sh["base"], sh["plain"], v_dev, sk, KEY, 7, ct, B), args.reps)
    p = sh["plain"]
    pt_dev = torch.zeros((B * d, n), dtype=torch.int64, device=dev)

    def host_path():
        v = vals % np.uint64(p) if p else vals.copy()
        pt = np.zeros((B, d, n), dtype=np.uint64)
        for k in range(d):
            pt[:, k, 0] = v % np.uint64(sh["base"])
            v //= np.uint64(sh["base"])
        pt_dev.copy_(torch.from_numpy(pt.reshape(B * d, n).view(np.int64)))
        ctx.encrypt_sk_dev(pt_dev, sk, KEY, 7, ct2, B * d)
    t_enc_host = timed(host_path, max(1, args.reps // 2))
    torch.cuda.synchronize()
    print(json.dumps({
        "shape": name, "n": n, "L": L, "B": B, "map": f"({sh['base']},{d})->({sh['new_base']},{nd})",
        "change_base_ms": round(t_map, 4), "composed_ms": round(t_comp, 4), "nonzero_entries": nnz,
        "map_equals_composition": same, "map_bytes": moved, "map_TBs": round(moved / (t_map * 1e-3) / 1e12, 3),
        "map_frac_of_hbm_line": round(moved / (t_map * 1e-3) / HBM_LINE, 3),
        "encrypt_sk_ms": round(t_enc, 4), "host_digits_encrypt_sk_ms": round(t_enc_host, 4),
        "encrypt_equal": bool(torch.equal(ct, ct2)),
        **({"dense_map_ms": round(t_dense, 4)} if t_dense is not None else {}),
    }), flush=True)
    ctx.close()


for name in (SHAPES if args.shape == "all" else [args.shape]):
    run(name, SHAPES[name])

"""One lifetime of three contexts at the smallest shapes that reach every owner of device memory in
the host runtime (run as a child process by tests/test_gpu_alloc_balance.py with EXACTO_DEBUG_ALLOC=1:
the switch is read once per process).  The parent replays the allocation log from stderr; this
script only has to finish.

  cfg3, n = 1024 (the smallest ring with the 31-bit key-switch basis):
      bfv_mul_and_relin of 5 products in chunks of 2 (three chunks over both lanes: a lane workspace),
      then 7 products in chunks of 4 (lane 0 and lane 1 both regrow); one automorphism; a Galois key set
      of two elements, one hoisted rotation, keyset.close(); one encrypt and decrypt through the host API
  cfg4, n = 1024: one dbfv_mul of two items (psum buffers, shared extensions, the plan tables)
  u64_dbfv: one dbfv_mul (the HPS digit-sum buffers)
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from bridge import uniform_residues  # noqa: E402
from oracle import params as P  # noqa: E402
from exacto_amd._ffi import HipContext  # noqa: E402

KEY = [11, 22, 33, 44]


def cfg3():
    n = 1024
    prm = P.cfg3_params(n)
    q = prm.ct_basis.moduli
    rng = np.random.default_rng(9101)
    ctx = HipContext.from_params(prm)
    ctx.set_chunk(2)
    ctx.load_relin_key(uniform_residues(rng, (prm.gadget_digits, 2), q, n))
    ct = uniform_residues(rng, (7, 2), q, n)
    ctx.bfv_mul_and_relin(ct[:5], ct[:5])
    ctx.set_chunk(4)
    ctx.bfv_mul_and_relin(ct, ct)
    gk = uniform_residues(rng, (prm.gadget_digits, 2), q, n)
    ctx.bfv_apply_automorphism(ct, 5, gk)
    ks = ctx.galois_keyset([3, 2 * n - 1], uniform_residues(rng, (2, prm.gadget_digits, 2), q, n))
    ctx.bfv_rotate_hoisted(ct, ks)
    ks.close()
    sk = ctx.gen_secret_key(KEY, stream=1)
    pt = rng.integers(0, prm.plain_modulus, size=(1, n), dtype=np.uint64)
    assert np.array_equal(ctx.bfv_decrypt(ctx.encrypt_sk(pt, sk, KEY, stream=2), sk), pt)
    ctx.close()


def dbfv(dp, items, seed):
    prm = dp.bfv_params
    n, q, d = prm.ring_degree, prm.ct_basis.moduli, dp.num_digits
    rng = np.random.default_rng(seed)
    ctx = HipContext.from_params(prm)
    ctx.load_relin_key(uniform_residues(rng, (prm.gadget_digits, 2), q, n))
    a = uniform_residues(rng, (items, d, 2), q, n)
    b = uniform_residues(rng, (items, d, 2), q, n)
    ctx.dbfv_mul(d, dp.base, dp.plain_modulus, a, b)
    ctx.close()


def main():
    import torch   # torch's HIP runtime first, as in tests/variant_digest.py
    torch.cuda.init()
    cfg3()
    dbfv(P.cfg4_params(1024), 2, 9102)
    dbfv(P.u64_dbfv(), 1, 9103)


if __name__ == "__main__":
    main()

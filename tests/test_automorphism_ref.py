"""tests/automorphism_ref.py (the whole-batch reference of the GPU key-switch tests) against the Python
restatement of bfv_apply_automorphism, at a small ring degree."""

import numpy as np
import pytest

import automorphism_ref
from oracle import bfv as obfv, cref, params as P
from bridge import ct_to_np, np_to_ct, np_to_rlk, uniform_residues


@pytest.mark.parametrize("moduli,gbase,keys", [(P.Q3, 0, None), (P.Q4, 256, None), (P.Q3, 0, 5),
                                               ([1099509805057], 0, None)])
def test_matches_python_oracle(moduli, gbase, keys):
    assert cref.available(), "oracle/c/liboracle.so is not built: run build() of __graft_entry__.py"
    n = 64
    prm = P.BfvParamsBuilder().ring_degree(n).plain_modulus(257).ct_moduli(moduli).gadget_base(gbase).build()
    q = prm.ct_basis.moduli
    rng = np.random.default_rng(len(moduli) + (keys or 0))
    ct = uniform_residues(rng, (3, 2), q, n)
    ct[0, 1] = np.array(q, dtype=np.uint64)[:, None] - 1
    gk = uniform_residues(rng, (keys or prm.gadget_digits, 2), q, n)
    for element in (5, 2 * n - 1, 3):
        got = automorphism_ref.apply_automorphism(prm, ct, element, gk, threads=2)
        keyset = obfv.GaloisKey(np_to_rlk(gk, prm).keys, element, prm)
        for b in range(3):
            want = ct_to_np(obfv.bfv_apply_automorphism(np_to_ct(ct[b], prm), keyset))
            assert np.array_equal(got[b], want), (element, b)

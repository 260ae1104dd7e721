"""Squares on the CPU: the six entry points are exported by the built library and declared in the header,
the ctypes table and the Rust block; the symmetric dBFV plan (exacto_dbfv_mul_plan, pure host code)
against a Python restatement of dbfv_mul's index rule (dbfv/eval.rs:109-132 + reduction.rs:34-52)."""

import os
import re
import subprocess
from collections import Counter

import pytest

from exacto_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["exacto_bfv_square_no_relin", "exacto_bfv_square_no_relin_dev", "exacto_bfv_square_and_relin",
           "exacto_bfv_square_and_relin_dev", "exacto_dbfv_square", "exacto_dbfv_square_dev"]


def test_symbols_exported_and_declared():
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    with open(os.path.join(ROOT, "include", "exacto_hip.h")) as f:
        hdr = f.read()
    with open(os.path.join(ROOT, "include", "exacto_hip.rs")) as f:
        rs = f.read()
    sigs = {s[0]: s[1] for s in _ffi._SIGS}
    for name in SYMBOLS + ["exacto_dbfv_mul_plan"]:
        assert name in exported, name
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert re.search(r"pub fn " + name + r"\(", rs), name
        assert name in sigs and name in _ffi.EXPORTED_SYMBOLS, name
    # the one-operand signatures: the two-operand ones less the second ciphertext (and its count / depth)
    assert len(sigs["exacto_bfv_square_no_relin"]) == len(sigs["exacto_bfv_mul_no_relin"]) - 2
    assert len(sigs["exacto_bfv_square_and_relin"]) == len(sigs["exacto_bfv_mul_and_relin"]) - 1
    assert len(sigs["exacto_dbfv_square"]) == len(sigs["exacto_dbfv_mul"]) - 2
    for name in SYMBOLS[::2]:
        assert sigs[name] == sigs[name + "_dev"], name
    for name in ("bfv_square_no_relin", "bfv_square_and_relin", "dbfv_square"):
        assert hasattr(_ffi.HipContext, name) and hasattr(_ffi.HipContext, name + "_dev"), name
    with open(os.path.join(ROOT, "include", "exacto.hpp")) as f:
        hpp = f.read()
    for name in ("bfv_square_no_relin", "bfv_square_and_relin", "dbfv_square"):
        assert len(re.findall(r"\b" + name + r"\(const ", hpp)) >= 2, name      # batched and single


def _rule(d, base, p):
    """{limb: Counter{(i, j): coefficient}} over all ordered pairs: 1 where i + j == k, the base-`base` digit k
    of base^(i+j) mod p (p = 0: mod 2^64) where i + j >= d."""
    out = {k: Counter() for k in range(d)}
    for i in range(d):
        for j in range(d):
            s = i + j
            if s < d:
                out[s][(i, j)] += 1
                continue
            val = pow(base, s, 1 << 64) if p == 0 else pow(base, s, p)
            for k in range(d):
                c = val % base
                val //= base
                if c:
                    out[k][(i, j)] += c
    return out


@pytest.mark.parametrize("p", [65536, 0, 65537])
@pytest.mark.parametrize("d", [1, 2, 3, 8])
def test_symmetric_plan(d, p):
    base = 256
    if base ** d < (p or 1 << 64):
        with pytest.raises(_ffi.ExactoError):
            _ffi.dbfv_mul_plan(d, base, p, True)
        return
    rule = _rule(d, base, p)
    pairs, limbs = _ffi.dbfv_mul_plan(d, base, p, False)
    spairs, slimbs = _ffi.dbfv_mul_plan(d, base, p, True)
    needed = {ij for k in rule for ij in rule[k]}
    # the product plan: every needed ordered pair once, each limb's terms the rule's
    assert sorted(pairs) == sorted(needed) and len(set(pairs)) == len(pairs)
    for k in range(d):
        assert Counter({pairs[pi]: c for pi, c in limbs[k]}) == rule[k], (d, p, k)
        assert len(limbs[k]) == len(rule[k])
    # the symmetric plan: i <= j only, each needed unordered pair once
    assert all(i <= j for i, j in spairs) and len(set(spairs)) == len(spairs)
    assert set(spairs) == {(min(i, j), max(i, j)) for i, j in needed}
    for k in range(d):
        # the same number of terms per limb (the key switch's and the summed scale's bounds count terms) ...
        assert len(slimbs[k]) == len(limbs[k]), (d, p, k)
        # ... and the multiset of (unordered pair, coefficient) is the rule's over all ordered pairs
        got = Counter((spairs[pi], c) for pi, c in slimbs[k])
        want = Counter()
        for (i, j), c in rule[k].items():
            want[((min(i, j), max(i, j)), c)] += 1
        assert got == want, (d, p, k)
    if p == 65536 or p == 0:
        assert all(c == 1 for lk in slimbs for _, c in lk)     # base^j = 0 mod p for j >= d: plain sums
    full = d * d == len(needed)
    assert len(spairs) == (d * (d + 1) // 2 if full else len({(min(i, j), max(i, j)) for i, j in needed}))

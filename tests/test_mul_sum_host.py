"""The Python wrappers of bfv_mul_sum (exacto_amd/_ffi.py) on the CPU: malformed term lists are refused
before any library call, and the documented entry points exist with their signatures."""

import inspect

import numpy as np
import pytest

from exacto_amd import _ffi
from exacto_amd._ffi import HipContext


class _NoLibrary:
    """Stands in for the loaded library: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the term list was checked")


def _bare_context():
    ctx = object.__new__(HipContext)
    ctx._lib = _NoLibrary()
    ctx._h = None
    ctx.L, ctx.n = 1, 16
    return ctx


@pytest.mark.parametrize("terms,nslots,text", [
    ([(0, 0, 0), (1, 1)], 1, "term 1 is not an (ia, ib, slot) triple"),       # ragged
    ([(0, 0, 0, 0)], 1, "term 0 is not an (ia, ib, slot) triple"),
    ([(0, 0, 0), 5], 1, "term 1 is not an (ia, ib, slot) triple"),
    ([(-1, 0, 0)], 1, "ia = -1"),                                             # negative indices
    ([(0, -2, 0)], 1, "ib = -2"),
    ([(0, 0, -1)], 1, "slot = -1"),
    ([(0, 0, 0), (0, 0, 2)], 2, "slot 2 >= nslots = 2"),                      # nslots smaller than a slot
    ([(0, 0, 0.5)], 1, "slot = 0.5"),
])
def test_malformed_terms_rejected_before_the_library(terms, nslots, text):
    ctx = _bare_context()
    a = np.zeros((1, 2, 2, 1, 16), dtype=np.uint64)
    with pytest.raises(ValueError) as e:
        ctx.bfv_mul_sum(a, a, terms, nslots)
    assert text in str(e.value)
    with pytest.raises(ValueError):
        ctx.bfv_mul_sum_dev(0, 2, 0, 2, terms, nslots, 0, 1)


def test_term_arrays():
    ia, ib, sl = HipContext._mul_sum_terms([(0, 1, 0), (np.uint32(2), 3, 1)], 2)
    assert all(v.dtype == np.uint32 for v in (ia, ib, sl))
    assert ia.tolist() == [0, 2] and ib.tolist() == [1, 3] and sl.tolist() == [0, 1]


def test_signatures_and_symbols():
    assert list(inspect.signature(HipContext.bfv_mul_sum).parameters) == ["self", "a", "b", "terms", "nslots"]
    assert list(inspect.signature(HipContext.bfv_mul_sum_dev).parameters) == [
        "self", "a", "na", "b", "nb", "terms", "nslots", "out", "batch"]
    assert list(inspect.signature(HipContext.set_mul_sum_group).parameters) == ["self", "max_products"]
    assert list(inspect.signature(HipContext.mul_sum_info).parameters) == ["self"]
    for name in ("exacto_bfv_mul_sum", "exacto_bfv_mul_sum_dev", "exacto_ctx_set_mul_sum_group",
                 "exacto_bfv_mul_sum_info"):
        assert name in _ffi.EXPORTED_SYMBOLS
    sigs = dict((s[0], s[1]) for s in _ffi._SIGS)
    assert len(sigs["exacto_bfv_mul_sum"]) == 12 and sigs["exacto_bfv_mul_sum"] == sigs["exacto_bfv_mul_sum_dev"]

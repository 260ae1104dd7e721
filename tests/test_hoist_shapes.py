"""tests/hoist_shapes.py on the CPU: the case table reaches every kernel instantiation and block shape that the
dispatch it restates can select, and tests/hoist_ref.py, the reference of those cases, has no cross-item
state and treats the two crafted items as the table's docstring says."""

import re
import os

import numpy as np
import pytest

import hoist_ref
import hoist_shapes as HS
from oracle import cref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(name):
    with open(os.path.join(ROOT, "exacto_amd", "csrc", name)) as f:
        return f.read()


def test_constants_are_the_sources():
    """The constants the restated dispatch depends on, read from the kernels' sources."""
    ks32, hoist = _src("ks32.hip"), _src("hoist.hip")
    assert re.search(r"constexpr int KS_LS = (\d+);", ks32).group(1) == str(HS.KS_LS)
    for name in ("HO_LS", "HO_IG", "HO_GMAX", "HO_TPB"):
        assert re.search(rf"constexpr int {name} = (\d+);", hoist).group(1) == str(getattr(HS, name)), name
    body = ks32[ks32.index("void ks32_mac_hoist("):]
    body = body[:body.index("#undef MAC_")]
    assert "G * CLB * KS_LS * sizeof(int) > 65536" in body and "lds > 32768 ? 8 : 4" in body
    assert f"MAC_(C_, 8, {HS.RUN}, true)" in body and f"MAC_(C_, 4, {HS.RUN}, false)" in body
    assert "constexpr int IG = 4 * NW;" in ks32
    assert "guse <= HO_GMAX && Ln % HO_LS == 0" in hoist


def test_table_covers_every_block_shape():
    reachable = {HS.mac_block_shape(g, L) for g in range(1, 65) for L in range(1, 5)}
    assert reachable == {(2, 4), (4, 4), (4, 8), (6, 4), (6, 8), (3, 8), (8, 4), (8, 8)}
    covered = set()
    for name, c in HS.CASES.items():
        if c.ks32:
            prm = c.params()
            L = len(prm.ct_basis.moduli)
            assert prm.ring_degree == 1024 and HS.mac_block_shape(HS.guse_of(name, prm), L) == c.shape, name
            covered.add(c.shape)
    assert set(HS.UNREACHABLE) == {(2, 4)} and all(HS.UNREACHABLE.values())
    assert not covered & set(HS.UNREACHABLE)
    assert covered | set(HS.UNREACHABLE) == reachable
    # all rotations (not the two-key form only) at every shape, and the RUN boundary at CL = 6
    guses = {HS.guse_of(n) for n, c in HS.CASES.items() if c.ks32 and c.shape[0] == 6}
    assert {HS.RUN, HS.RUN + 1, 2 * HS.RUN + 1} <= guses
    assert {HS.guse_of(n) for n, c in HS.CASES.items() if c.ks32 and c.num_keys is not None} >= {12, 13, 25}


def test_table_covers_the_limbwise_kernels():
    seen = set()
    for name, c in HS.CASES.items():
        if c.ks32:
            continue
        prm = c.params()
        n, L, guse = prm.ring_degree, len(prm.ct_basis.moduli), HS.guse_of(name, prm)
        assert n <= 256 and HS.limbwise_kernel(guse, L, n, False) == c.shape, name
        seen.add((c.shape, False))
        if c.lt:
            assert HS.limbwise_kernel(guse, L, n, True) == "plain"
            seen.add(("plain", True))
    assert seen == {("lds", False), ("plain", False), ("plain", True)}
    assert {HS.guse_of(n) for n in HS.CASES if n.startswith("lw_keys_")} == {1, 4, 5, HS.HO_GMAX, HS.HO_GMAX + 1}


def test_launch_shapes_of_the_table():
    """Items per launch, with S = 3 on the 31-bit path (asserted against the context on the GPU)."""
    def first(name, lt=False):
        c = HS.CASES[name]
        prm = c.params()
        return HS.launch_items(c.chunk, c.B, 3 if c.ks32 else 0, lt, len(prm.ct_basis.moduli), prm.ring_degree,
                               len(c.elements(prm.ring_degree)))
    for name, c in HS.CASES.items():
        if c.launch:
            assert first(name) == c.launch, name
    for name, nw in (("k32_items_4waves", 4), ("k32_items_8waves", 8)):
        c = HS.CASES[name]
        assert c.shape[1] == nw and c.launch == 2 * (4 * nw) + 5 and c.chunk1
    c = HS.CASES["k32_lanes"]
    assert [min(3, c.B - s) for s in range(0, c.B, 3)] == [3, 3, 1] and first("k32_lanes", lt=True) == 2
    c = HS.CASES["lw_items"]
    assert c.launch == c.B == HS.HO_IG + 6 and c.chunk1
    for name in ("lw_plain_blocks", "lw_lt_blocks"):
        prm = HS.CASES[name].params()
        assert (len(prm.ct_basis.moduli) * prm.ring_degree + HS.HO_TPB - 1) // HS.HO_TPB == 3
    # an LDS block of 64 flat positions over four and over two limbs
    for name, limbs in (("lw_n16_four_limbs", 4), ("lw_n32_two_limbs", 2)):
        prm = HS.CASES[name].params()
        assert len(prm.ct_basis.moduli) == limbs and limbs * prm.ring_degree == HS.HO_LS
    n9 = HS.CASES["k32_nine"].elements(1024)
    assert len(n9) == 9 and [i for i, e in enumerate(n9) if e % 2048 == 1] == [0, 4, 8] and n9.count(3) == 2
    # every case: the two crafted items and a uniform one
    assert all(c.B >= 3 for c in HS.CASES.values())


@pytest.mark.parametrize("name", ["lw_n32_two_limbs", "lw_keys_5"])
def test_reference_has_no_cross_item_state(name):
    assert cref.available(), "oracle/c/liboracle.so is not built: run build() of __graft_entry__.py"
    prm, elements, ct, gks, _ = HS.make_inputs(name)
    whole = hoist_ref.rotate_hoisted(prm, ct, elements, gks)
    single = np.concatenate([hoist_ref.rotate_hoisted(prm, ct[b:b + 1], elements, gks) for b in range(ct.shape[0])])
    assert np.array_equal(whole, single)
    # ... and none on the order either
    assert np.array_equal(hoist_ref.rotate_hoisted(prm, ct[::-1], elements, gks), whole[::-1])


@pytest.mark.parametrize("name", ["lw_n16_four_limbs", "lw_keys_5", "lw_hps"])
def test_crafted_items_in_the_reference(name):
    assert cref.available()
    prm, elements, ct, gks, _ = HS.make_inputs(name)
    n, q = prm.ring_degree, np.array(prm.ct_basis.moduli, dtype=np.uint64)
    assert np.array_equal(ct[0], np.broadcast_to((q - np.uint64(1))[None, :, None], ct[0].shape))
    assert not ct[1, 1].any() and ct[1, 0].any() and (ct[2] != 0).any()
    want = hoist_ref.rotate_hoisted(prm, ct, elements, gks)
    assert (want < q[None, None, None, :, None]).all()
    keyed = 0
    for r, el in enumerate(elements):
        if el % (2 * n) == 1:
            assert np.array_equal(want[:, r], ct)
            continue
        keyed += 1
        perm = hoist_ref.ntt_permutation(n, el)
        assert np.array_equal(want[1, r, 0], ct[1, 0][:, perm]), (name, el)
        assert not want[1, r, 1].any(), (name, el)
        # the item of all q_l - 1 is not a fixed point of anything: both components depend on the key
        assert want[0, r, 1].any() and not np.array_equal(want[0, r, 0], ct[0, 0][:, perm])
    assert keyed == 2

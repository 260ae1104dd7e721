"""CPU: exacto_dbfv_change_base_matrix (dbfv/advanced.rs:119-130), the host half of
dbfv_change_base, against a restatement written with the oracle's digit_decompose."""

import pytest

from exacto_amd import _ffi
from oracle import dbfv as odbfv


def restated(d, base, plain, new_base, new_d):
    """advanced.rs:111-130: column i = digit_decompose((base^i mod p) as u64, new_base, new_d)."""
    p = (1 << 64) if plain == 0 else plain
    m = [[0] * d for _ in range(new_d)]
    b_pow = 1
    for i in range(d):
        digits = odbfv.digit_decompose(b_pow % p, new_base, new_d)
        for j in range(new_d):
            m[j][i] = digits[j]
        b_pow = b_pow * base % p
    return m


@pytest.mark.parametrize("src,dst", [
    ((16, 2, 256), (4, 4)),
    ((16, 2, 256), (3, 6)),        # entries of 2: 16 = 1 + 2*3 + 1*9
    ((16, 2, 256), (256, 1)),      # d_out < d_in: the excess digit of 16 is dropped
    ((256, 8, 0), (16, 16)),       # p = 2^64
    ((256, 8, 0), (65536, 4)),
])
def test_change_base_matrix(src, dst):
    base, d, plain = src
    new_base, new_d = dst
    got = _ffi.dbfv_change_base_matrix(d, base, plain, new_base, new_d)
    want = restated(d, base, plain, new_base, new_d)
    assert got.shape == (new_d, d)
    assert [[int(x) for x in row] for row in got] == want


def test_change_base_matrix_known_entries():
    m = _ffi.dbfv_change_base_matrix(2, 16, 256, 3, 6)
    assert [int(x) for x in m[:, 0]] == [1, 0, 0, 0, 0, 0]
    assert [int(x) for x in m[:, 1]] == [1, 2, 1, 0, 0, 0]
    m = _ffi.dbfv_change_base_matrix(2, 16, 256, 256, 1)
    assert [[int(x) for x in row] for row in m] == [[1, 16]]
    # p = 2^64: 256^i = 16^(2i), one 1 per column
    m = _ffi.dbfv_change_base_matrix(8, 256, 0, 16, 16)
    assert all(int(m[j, i]) == (1 if j == 2 * i else 0) for i in range(8) for j in range(16))


@pytest.mark.parametrize("args,text", [
    ((2, 16, 256, 1, 4), "new base must be >= 2"),
    ((2, 16, 256, 4, 0), "new_num_digits must be >= 1"),
    ((2, 16, 256, 4, 3), "base^digits = 64 < plain_modulus = 256"),
    ((8, 256, 0, 16, 15), "base^digits = 1152921504606846976 < plain_modulus = 18446744073709551616"),
    ((2, 1, 256, 4, 4), "base must be >= 2"),
    ((0, 16, 256, 4, 4), "num_digits must be >= 1"),
    ((1, 16, 256, 4, 4), "base^digits = 16 < plain_modulus = 256"),
])
def test_change_base_matrix_errors(args, text):
    with pytest.raises(_ffi.ExactoError) as e:
        _ffi.dbfv_change_base_matrix(*args)
    assert e.value.variant == "InvalidParam"
    assert str(e.value) == "invalid parameter: " + text

"""The dBFV hoisted rotations and linear transforms through the C++ host API (include/exacto.hpp):
tests/cpp/test_dbfv_lt.cpp compiles and links on the CPU; on the GPU it runs one shape on the fused route
(n = 64) and one on the staged route (n = 1024) on residues from a fixed generator and prints a digest of each
output, which is held here against the ctypes result on the same inputs."""

import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "test_dbfv_lt")
MASK = (1 << 64) - 1


def compile_test(out=BIN):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    lib = os.path.join(ROOT, "exacto_amd", "lib")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_dbfv_lt.cpp"), "-o", out, "-L", lib, "-lexacto_hip",
           f"-Wl,-rpath,{lib}"]
    subprocess.run(cmd, check=True)
    return out


def test_cpp_dbfv_lt_compiles_and_links(tmp_path):
    binary = compile_test(str(tmp_path / "test_dbfv_lt"))
    r = subprocess.run([binary, "host"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr


class _Lcg:
    """The generator of tests/cpp/test_dbfv_lt.cpp."""

    def __init__(self, n):
        self.x = (0x9E3779B97F4A7C15 + n) & MASK

    def words(self, count):
        out = np.empty(count, dtype=np.uint64)
        x = self.x
        for i in range(count):
            x = (x * 6364136223846793005 + 1442695040888963407) & MASK
            out[i] = x
        self.x = x
        return out

    def residues(self, rows, moduli, n):
        w = self.words(rows * len(moduli) * n).reshape(rows, len(moduli), n)
        return w % np.array(moduli, dtype=np.uint64)[None, :, None]


def _fnv(words):
    h = 1469598103934665603
    for byte in np.ascontiguousarray(words, dtype="<u8").tobytes():
        h = ((h ^ byte) * 1099511628211) & MASK
    return h


def _ctypes_digest(n):
    from exacto_amd._ffi import HipContext
    from oracle import params as P
    base, d, p = 16, 2, 251
    prm = P.BfvParamsBuilder().ring_degree(n).plain_modulus(12289).ct_moduli(P.Q3).build()
    q, G = prm.ct_basis.moduli, prm.gadget_digits
    g = _Lcg(n)
    ct = g.residues(d * 2, q, n).reshape(1, d, 2, len(q), n)
    elements = [3, 1, 2 * n - 1]
    gks = np.zeros((len(elements), G, 2, len(q), n), dtype=np.uint64)
    for r, el in enumerate(elements):
        if el != 1:
            gks[r] = g.residues(G * 2, q, n).reshape(G, 2, len(q), n)
    pts = g.words(len(elements) * d * n).reshape(len(elements), d, n)
    ctx = HipContext.from_params(prm)
    ks = ctx.galois_keyset(elements, gks)
    out, _ = ctx.dbfv_linear_transform(d, base, p, ct, ks, pts)
    return _fnv(out)


@pytest.mark.gpu
def test_cpp_dbfv_lt_against_ctypes(gpu_available, tmp_path):
    binary = BIN if os.path.exists(BIN) else compile_test(str(tmp_path / "test_dbfv_lt"))
    r = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr
    digests = dict(re.findall(r"^DIGEST (\w+) ([0-9a-f]{16})$", r.stdout, re.M))
    assert set(digests) == {"fused_n64", "staged_n1024"}
    assert int(digests["fused_n64"], 16) == _ctypes_digest(64)
    assert int(digests["staged_n1024"], 16) == _ctypes_digest(1024)

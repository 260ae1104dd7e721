"""The dBFV plaintext products through the C++ host API (include/exacto.hpp): tests/cpp/test_dbfv_plain.cpp compiles
and links on the CPU; on the GPU it encrypts n = 16 values per ciphertext at (b = 16, d = 2, p = 256) and at
(b = 256, d = 8, p = 2^64), applies public values with dbfv_batch_plain_mul / dbfv_plain_mul_sum / dbfv_plain_add /
dbfv_plain_sub, decrypts and compares every slot, then checks the error strings."""

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "test_dbfv_plain")


def compile_test(out=BIN):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    lib = os.path.join(ROOT, "exacto_amd", "lib")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_dbfv_plain.cpp"), "-o", out, "-L", lib, "-lexacto_hip",
           f"-Wl,-rpath,{lib}"]
    subprocess.run(cmd, check=True)
    return out


def test_cpp_dbfv_plain_compiles_and_links(tmp_path):
    binary = compile_test(str(tmp_path / "test_dbfv_plain"))
    r = subprocess.run([binary, "host"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_dbfv_plain_slot_products(gpu_available, tmp_path):
    binary = BIN if os.path.exists(BIN) else compile_test(str(tmp_path / "test_dbfv_plain"))
    r = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr

"""The squares of the C++ host API (include/exacto.hpp): compiles and links on the CPU; on the GPU
tests/cpp/test_square.cpp runs keygen -> encrypt 3 and 5 -> bfv_square_and_relin -> decrypt at compact_bfv
(9 and 25 mod t, the two-operand call bit for bit) and dbfv_square at u64_dbfv (x^2 mod 2^64)."""

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "test_square")


def compile_test(out=BIN):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    lib = os.path.join(ROOT, "exacto_amd", "lib")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_square.cpp"), "-o", out, "-L", lib, "-lexacto_hip",
           f"-Wl,-rpath,{lib}"]
    subprocess.run(cmd, check=True)
    return out


def test_cpp_square_compiles_and_links(tmp_path):
    binary = compile_test(str(tmp_path / "test_square"))
    r = subprocess.run([binary, "host"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_square_decrypts(gpu_available, tmp_path):
    binary = BIN if os.path.exists(BIN) else compile_test(str(tmp_path / "test_square"))
    r = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr

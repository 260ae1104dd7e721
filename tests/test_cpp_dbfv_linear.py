"""The dBFV surface of the C++ host API (include/exacto.hpp) beyond the product: compiles on the
CPU; on the GPU tests/cpp/test_dbfv_linear.cpp runs keygen -> encrypt -> change_base -> div_by_base
-> decrypt at compact_dbfv and checks the values and the DbfvParams each step returns."""

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "test_dbfv_linear")


def compile_test(out=BIN):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    lib = os.path.join(ROOT, "exacto_amd", "lib")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_dbfv_linear.cpp"), "-o", out, "-L", lib, "-lexacto_hip",
           f"-Wl,-rpath,{lib}"]
    subprocess.run(cmd, check=True)
    return out


def test_cpp_dbfv_linear_compiles(tmp_path):
    compile_test(str(tmp_path / "test_dbfv_linear"))


@pytest.mark.gpu
def test_cpp_dbfv_circuit(gpu_available, tmp_path):
    binary = BIN if os.path.exists(BIN) else compile_test(str(tmp_path / "test_dbfv_linear"))
    r = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr

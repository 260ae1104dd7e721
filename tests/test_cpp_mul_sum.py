"""bfv_mul_sum of the C++ host API (include/exacto.hpp): compiles and links on the CPU; on the GPU
tests/cpp/test_mul_sum.cpp runs keygen -> encrypt three pairs of scalars -> bfv_mul_sum -> decrypt at
compact_bfv and checks sum x_k y_k mod t, the composition with bfv_mul_and_relin + bfv_add bit for bit,
a sum of squares and the error mapping."""

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "test_mul_sum")


def compile_test(out=BIN):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    lib = os.path.join(ROOT, "exacto_amd", "lib")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_mul_sum.cpp"), "-o", out, "-L", lib, "-lexacto_hip",
           f"-Wl,-rpath,{lib}"]
    subprocess.run(cmd, check=True)
    return out


def test_cpp_mul_sum_compiles_and_links(tmp_path):
    binary = compile_test(str(tmp_path / "test_mul_sum"))
    r = subprocess.run([binary, "host"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_mul_sum_dot_product(gpu_available, tmp_path):
    binary = BIN if os.path.exists(BIN) else compile_test(str(tmp_path / "test_mul_sum"))
    r = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr

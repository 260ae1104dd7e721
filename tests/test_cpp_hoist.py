"""Hoisted rotations through the C++ host API (include/exacto.hpp): tests/cpp/test_hoist.cpp compiles, links and
checks galois_ntt_permutation on the CPU (a permutation, perm_k o perm_k' the table of k k', the errors); on
the GPU it runs keygen -> batch_encrypt_sk -> bfv_rotate_hoisted / bfv_linear_transform -> batch_decrypt at
cfg3's basis with n = 1024 on a GaloisKeySet of three row rotations and the row swap."""

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "test_hoist")


def compile_test(out=BIN):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    lib = os.path.join(ROOT, "exacto_amd", "lib")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_hoist.cpp"), "-o", out, "-L", lib, "-lexacto_hip",
           f"-Wl,-rpath,{lib}"]
    subprocess.run(cmd, check=True)
    return out


def test_cpp_hoist_compiles_and_links(tmp_path):
    binary = compile_test(str(tmp_path / "test_hoist"))
    r = subprocess.run([binary, "host"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_hoist_rotations(gpu_available, tmp_path):
    binary = BIN if os.path.exists(BIN) else compile_test(str(tmp_path / "test_hoist"))
    r = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr

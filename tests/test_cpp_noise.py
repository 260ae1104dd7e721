"""The noise measurement of the C++ host API (include/exacto.hpp: bfv_noise_inf, max_limb_noise,
noise_budget_bits): compiles on the CPU, where the host-only word and budget helpers also run; on the GPU
tests/cpp/test_noise.cpp runs keygen -> dbfv_encrypt_sk -> max_limb_noise -> dbfv_mul -> max_limb_noise at
compact_dbfv and asserts growth and a positive budget before (paper_repro.rs:166-201, 238-281)."""

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "test_noise")


def compile_test(out=BIN):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    lib = os.path.join(ROOT, "exacto_amd", "lib")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_noise.cpp"), "-o", out, "-L", lib, "-lexacto_hip",
           f"-Wl,-rpath,{lib}"]
    subprocess.run(cmd, check=True)
    return out


def test_cpp_noise_compiles_and_host_helpers(tmp_path):
    binary = compile_test(str(tmp_path / "test_noise"))
    r = subprocess.run([binary, "host"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_noise_growth(gpu_available, tmp_path):
    binary = BIN if os.path.exists(BIN) else compile_test(str(tmp_path / "test_noise"))
    r = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr

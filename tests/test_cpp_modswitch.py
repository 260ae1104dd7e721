"""Modulus switching through the C++ host API (include/exacto.hpp: mod_switch, mod_switch_drop_prime,
lower_secret_key): compiles on the CPU, where the host-only level predicate also runs; on the GPU
tests/cpp/test_modswitch.cpp runs encrypt -> (multiply) -> mod_switch -> decrypt / noise under the lower
parameters at cfg3's primes, the reference-mode function and the ModulusMismatch / InvalidParam cases."""

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "test_modswitch")


def compile_test(out=BIN):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    lib = os.path.join(ROOT, "exacto_amd", "lib")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_modswitch.cpp"), "-o", out, "-L", lib, "-lexacto_hip",
           f"-Wl,-rpath,{lib}"]
    subprocess.run(cmd, check=True)
    return out


def test_cpp_modswitch_compiles_and_host_helpers(tmp_path):
    binary = compile_test(str(tmp_path / "test_modswitch"))
    r = subprocess.run([binary, "host"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_modswitch_end_to_end(gpu_available, tmp_path):
    binary = BIN if os.path.exists(BIN) else compile_test(str(tmp_path / "test_modswitch"))
    r = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr

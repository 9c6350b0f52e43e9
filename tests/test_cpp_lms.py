"""The C++ surface of the LMS / NLMS adaptive filter bank (sdsp::lms_bank, include/sdsp/lms.h): a program compiled with g++ and
clang++ under the project's warning flags; on the GPU it streams blocks through the bank, checks that a known 8-tap system is identified
within the f32 bound of tests/test_lms_host.py and that e matches a double loop computed in the program."""
import subprocess

import pytest

from conftest import ROOT

SRC = ROOT / "tests" / "cpp" / "test_lms.cpp"
FLAGS = ["-std=c++17", "-O2", "-Wall", "-Wextra", "-Wpedantic", "-Wconversion", "-Werror", f"-I{ROOT / 'include'}"]


def _compile(cxx, out):
    import simpledsp_amd
    simpledsp_amd.load()  # builds libsdsp_hip.so if needed
    lib = ROOT / "simpledsp_amd" / "lib"
    out.parent.mkdir(parents=True, exist_ok=True)
    r = subprocess.run([cxx, *FLAGS, str(SRC), "-o", str(out), f"-L{lib}", "-lsdsp_hip", f"-Wl,-rpath,{lib}",
                        "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return out


@pytest.mark.parametrize("cxx", ["g++", "/opt/rocm/lib/llvm/bin/clang++"])
def test_lms_bank_compiles_warning_free(cxx, tmp_path):
    _compile(cxx, tmp_path / "test_lms")


@pytest.mark.gpu
def test_lms_bank_identifies_a_known_system_on_gpu(tmp_path):
    exe = _compile("g++", tmp_path / "test_lms")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")

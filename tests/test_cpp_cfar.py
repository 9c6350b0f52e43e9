"""The C++ surface of the CFAR detector bank (sdsp::cfar_bank, include/sdsp/cfar.h): a program compiled with g++ and clang++ under the
project's warning flags; on the GPU it streams exponential noise with injected targets through CA, GO and OS banks in blocks and checks
that every threshold and decision equals a loop computed in the program, bit for bit, and that every target is found."""
import subprocess

import pytest

from conftest import ROOT

SRC = ROOT / "tests" / "cpp" / "test_cfar.cpp"
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
def test_cfar_bank_compiles_warning_free(cxx, tmp_path):
    _compile(cxx, tmp_path / "test_cfar")


@pytest.mark.gpu
def test_cfar_bank_finds_targets_on_gpu(tmp_path):
    exe = _compile("g++", tmp_path / "test_cfar")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")

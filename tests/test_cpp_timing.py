"""The C++ surface of the symbol-timing recovery bank (sdsp::timing_bank, include/sdsp/timing.h): a program compiled with g++ and
clang++ under the project's warning flags; on the GPU it streams blocks of noisy QPSK rows through the bank and checks every count,
symbol, err, period and the final state against the contract's recursion computed in the program in the bank's precision."""
import subprocess

import pytest

from conftest import ROOT

SRC = ROOT / "tests" / "cpp" / "test_timing.cpp"
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
def test_timing_bank_compiles_warning_free(cxx, tmp_path):
    _compile(cxx, tmp_path / "test_timing")


@pytest.mark.gpu
def test_timing_bank_equals_the_contract_loop_on_gpu(tmp_path):
    exe = _compile("g++", tmp_path / "test_timing")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")
